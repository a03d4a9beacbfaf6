// What the wide learners (dm_ppo_wide.hip: bf16 operands; dm_ppo_wide3.hip: split-bf16 operands) share: the operand / accumulator
// vector types of v_mfma_f32_32x32x16_bf16, the bf16 rounding of their stores and the FRAGMENT ORDER of every matrix they stream.
// Fragment order of a matrix M[N][K] (N % 32 == 0, K % 16 == 0) that feeds v_mfma_f32_32x32x16_bf16 as the operand with row / column
// index n and reduction index k: element (n, k) lives at ((((n >> 5) * (K >> 4) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (n & 31)) * 8
// + (k & 7)) — tile of 32 rows, k-step of 16, then the 64 lanes' 16-byte fragments in lane order.  A wave's load of one fragment is
// base + lane * 16 bytes: eight full 128-byte lines.
#ifndef DM_WIDE_FRAG_H
#define DM_WIDE_FRAG_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef short wide_b8 __attribute__((ext_vector_type(8)));      // 8 bf16 = one MFMA operand fragment (4 VGPRs)
typedef float wide_f16 __attribute__((ext_vector_type(16)));    // 32 x 32 accumulator: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)

// round to nearest even WITHOUT the NaN branch of bf16_rne (dm_bf16.h): kept apart, merging them changes dm_ppo_wide.hip's instructions
__device__ __forceinline__ unsigned short wide_f2bf(float x) {
  unsigned u = __float_as_uint(x);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
// two floats -> two bf16 in one dword (low half = a): gfx950's v_cvt_pk_bf16_f32, round to nearest even like wide_f2bf
typedef __bf16 wide_bf2 __attribute__((ext_vector_type(2)));
typedef float wide_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned wide_pk2(float a, float b) {
  const wide_f2 v = {a, b};
  const wide_bf2 r = __builtin_convertvector(v, wide_bf2);
  return *reinterpret_cast<const unsigned *>(&r);
}
__device__ __forceinline__ int wide_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
// fragment order (file header): element index of (n, k) in a matrix with K / 16 = nks k-steps
__device__ __forceinline__ size_t wide_frag(int n, int k, int nks) {
  return ((((size_t)(n >> 5) * nks + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (n & 31)) << 3) + (k & 7);
}
// the fragment of tile t, k-step ks for this lane
__device__ __forceinline__ wide_b8 wide_ldfrag(const unsigned short *M, int t, int ks, int nks, int lane) {
  return *reinterpret_cast<const wide_b8 *>(M + ((((size_t)t * nks + ks) * 64 + lane) << 3));
}

}  // namespace
#endif
