// 32 x 32 MFMA tiles over packed fp32 weights: the accumulator type, the operand-order weight packing and the k-loop that the
// rollout forward (dm_policy.hip) and the fused [256,128] learner (dm_ppo_mlp.hip) share; dm_ppo.hip takes the accumulator type.
// Operand layout: file comment of dm_policy.hip.
#ifndef DM_POL_TILE_H
#define DM_POL_TILE_H
#include <hip/hip_runtime.h>

namespace {

constexpr int POL_R = 32;          // batch rows per workgroup
constexpr int POL_PAD = 4;         // LDS row padding in floats: keeps 16-byte alignment and spreads rows over the banks

typedef float pol_f16v __attribute__((ext_vector_type(16)));

// acc += X[32 x 8 (kb1 - kb0)] W^T for one 32-neuron tile; xs = LDS activations (row stride sx), P = the tile's packed
// weights (64 float4 per k-block of 8).
template <int U>
__device__ __forceinline__ void pol_load(const float4 *p, const float *xrow, int kb, float4 (&w)[U], float4 (&a)[U]) {
#pragma unroll
  for (int u = 0; u < U; u++) w[u] = p[(size_t)(kb + u) * 64];
#pragma unroll
  for (int u = 0; u < U; u++) a[u] = *reinterpret_cast<const float4 *>(xrow + (kb + u) * 8);
}
template <int U>
__device__ __forceinline__ void pol_mfma(const float4 (&w)[U], const float4 (&a)[U], pol_f16v &acc) {
#pragma unroll
  for (int u = 0; u < U; u++) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, w[u].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, w[u].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, w[u].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, w[u].w, acc, 0, 0, 0);
  }
}
// first weight batch of a tile, issued early (before the barrier that publishes the tile's activations: the weight
// stream does not depend on them), consumed by pol_tile_pre
template <int U>
__device__ __forceinline__ void pol_prefetch(const float4 *P, int lane, int kb0, float4 (&w)[U]) {
#pragma unroll
  for (int u = 0; u < U; u++) w[u] = P[(size_t)(kb0 + u) * 64 + lane];
}
template <int U, bool PRE>
__device__ __forceinline__ void pol_tile_impl(const float *xs, int sx, const float4 *P, int lane, int kb0, int kb1, pol_f16v &acc,
                                              float4 (&wA)[U]) {
  const float *xrow = xs + (lane & 31) * sx + 4 * (lane >> 5);
  const float4 *p = P + lane;
  const int nb = (kb1 - kb0) / U;
  // ping-pong over two register sets (no copies): the loads of batch it + 1 are in flight under the 4 U MFMAs of batch
  // it, and the MFMAs wait only for their own batch (s_waitcnt vmcnt(U))
  float4 aA[U], wB[U], aB[U];
  if (nb > 0) {
    if (PRE) {
#pragma unroll
      for (int u = 0; u < U; u++) aA[u] = *reinterpret_cast<const float4 *>(xrow + (kb0 + u) * 8);
    } else {
      pol_load<U>(p, xrow, kb0, wA, aA);
    }
  }
  int it = 0;
  for (; it + 2 <= nb; it += 2) {
    pol_load<U>(p, xrow, kb0 + (it + 1) * U, wB, aB);
    pol_mfma<U>(wA, aA, acc);
    if (it + 2 < nb) pol_load<U>(p, xrow, kb0 + (it + 2) * U, wA, aA);
    pol_mfma<U>(wB, aB, acc);
  }
  if (it < nb) pol_mfma<U>(wA, aA, acc);
  for (int kb = kb0 + nb * U; kb < kb1; kb++) {
    const float4 w = p[(size_t)kb * 64];
    const float4 a = *reinterpret_cast<const float4 *>(xrow + kb * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
  }
}
template <int U>
__device__ __forceinline__ void pol_tile(const float *xs, int sx, const float4 *P, int lane, int kb0, int kb1, pol_f16v &acc) {
  float4 wA[U];
  pol_tile_impl<U, false>(xs, sx, P, lane, kb0, kb1, acc, wA);
}
// the first batch's weights (kb0 .. kb0 + U - 1; requires kb1 - kb0 >= U) were fetched by pol_prefetch<U>
template <int U>
__device__ __forceinline__ void pol_tile_pre(const float *xs, int sx, const float4 *P, int lane, int kb0, int kb1, pol_f16v &acc,
                                             float4 (&wpre)[U]) {
  pol_tile_impl<U, true>(xs, sx, P, lane, kb0, kb1, acc, wpre);
}

// W (element (o, k) at W[o so + k sk]; nn.Linear [O x K] row-major is so = K, sk = 1, its transpose so = 1, sk = O) ->
// P[tile][k-block][lane] float4 = W(32 tile + (lane & 31), 8 kb + 4 (lane >> 5) + 0..3), zero outside O x K
__device__ __forceinline__ void pol_pack_one(const float *W, int O, int K, int so, int sk, int tiles, int KB, float4 *P, int i) {
  if (i >= tiles * KB * 64) return;
  const int lane = i & 63, kb = (i >> 6) % KB, to = (i >> 6) / KB;
  const int o = to * 32 + (lane & 31), k = kb * 8 + 4 * (lane >> 5);
  float v[4];
#pragma unroll
  for (int c = 0; c < 4; c++) v[c] = (o < O && k + c < K) ? W[(size_t)o * so + (size_t)(k + c) * sk] : 0.f;
  P[i] = make_float4(v[0], v[1], v[2], v[3]);
}

inline int pol_dp(int D) { return (D + 7) & ~7; }
inline bool pol_dims_ok(int D, int H1, int H2, int A) {
  return D >= 1 && H1 >= 32 && H2 >= 32 && (H1 % 32) == 0 && (H2 % 32) == 0 && A >= 1 && A <= 32;
}

}  // namespace
#endif
