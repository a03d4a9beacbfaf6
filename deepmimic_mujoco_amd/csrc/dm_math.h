// dm_math.h — the small device helpers whose arithmetic is the same in the humanoid engine (dm_kernels.hip) and the G1 engine
// (dm_g1_math.h), defined once.  Look-alikes that add in another order or divide where the other multiplies stay in their engine
// (DESIGN.md §4).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

namespace {

// Compile-time loop with early exit: f(integral_constant<int, I>) returns false to stop.  Guarantees static register indices
// for per-lane arrays (a rolled loop would put them in scratch).
template <int I, int N>
struct StaticFor {
  template <class F>
  static __device__ __forceinline__ void run(F &&f) {
    if constexpr (I < N) {
      if (f(std::integral_constant<int, I>{})) StaticFor<I + 1, N>::run(f);
    }
  }
};

__device__ __forceinline__ float rl(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 64 lanes, uniform in every lane: four DPP steps inside each row of 16, the four row sums through v_readlane
// (~12 instructions; six LDS-permute round trips would sit in every dependent chain that reduces)
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  return (rl(v, 0) + rl(v, 16)) + (rl(v, 32) + rl(v, 48));
}

__device__ __forceinline__ void cross3(float *r, const float *a, const float *b) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <class F>   // fp32, and fp64 in the G1 pose chain
__device__ __forceinline__ void quat_mul(F *r, const F *a, const F *b) {
  const F w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const F x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const F y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const F z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
template <class F>
__device__ __forceinline__ void quat2mat(F *m, const F *q) {
  const F w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
__device__ __forceinline__ void quat_normalize(float *q) {
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < 1e-15f) { q[0] = 1; q[1] = q[2] = q[3] = 0; }   // mjMINVAL
  else { float i = 1.0f / n; q[0] *= i; q[1] *= i; q[2] *= i; q[3] *= i; }
}
__device__ __forceinline__ void mat_vec(float *r, const float *m, const float *v) {
  float x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
  float y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
  float z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
// py3dtf.Quaternion(x,y,z,w).to_rpy() restated: standard ZYX, no normalisation
__device__ __forceinline__ void quat_to_rpy(const float *q, float *rpy) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  rpy[0] = atan2f(2 * (w * x + y * z), 1 - 2 * (x * x + y * y));
  rpy[1] = asinf(fminf(fmaxf(2 * (w * y - z * x), -1.f), 1.f));
  rpy[2] = atan2f(2 * (w * z + x * y), 1 - 2 * (y * y + z * z));
}

}  // namespace
