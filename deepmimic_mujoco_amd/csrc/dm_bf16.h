// bf16 storage of the rollout buffer's obs / act arrays (PPO(buffer_dtype=torch.bfloat16)): the narrowing stores of the rollout
// side (dm_policy_forward_bf16, dm_rollout_store_bf16) and the widening row reads of the learner's gather (dm_ppo_gather_bf16,
// dm_flat_adam_step_gather_bf16).  Only the natural 2-byte alignment of a bf16 array is assumed anywhere: row t of a sub-batch
// slice, or row idx[r] of a flattened buffer with an odd row length (D = 67), starts at an arbitrary element.
#ifndef DM_BF16_H
#define DM_BF16_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// fp32 -> bf16, round to nearest even, bit for bit torch.Tensor.to(torch.bfloat16): the integer-add rounding carries correctly into
// the exponent (1.99609375 + 2^-9 -> 2.0, the largest finite values -> inf), treats fp32 denormals like any other value whatever
// the wave's denormal mode, and NaN is answered separately (the add would turn payloads >= 0x7FFF8000 into +-0 / inf): quiet NaN
// 0x7FC0, as PyTorch does.
__device__ __forceinline__ unsigned bf16_rne(float x) {
  const unsigned u = __float_as_uint(x);
  const unsigned r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  return (x != x) ? 0x7fc0u : r;
}
__device__ __forceinline__ float bf16_widen(unsigned short b) { return __uint_as_float((unsigned)b << 16); }   // exact

// dst[0 .. n) <- bf16(src[0 .. n)) by the nt threads of a group (t = 0 .. nt - 1).  The range is contiguous, so it goes out as
// packed pairs, one aligned dword store per lane (a wave's store covers 256 contiguous bytes), with a scalar element in front when
// dst sits at an odd element and one behind when what remains is odd.
__device__ __forceinline__ void bf16_store_range(unsigned short *dst, const float *src, int n, int t, int nt) {
  const int head = (int)((reinterpret_cast<uintptr_t>(dst) >> 1) & 1u) & (n > 0 ? 1 : 0);
  const int pairs = (n - head) >> 1;
  if (t == 0 && head) dst[0] = (unsigned short)bf16_rne(src[0]);
  unsigned *d2 = reinterpret_cast<unsigned *>(dst + head);
  const float *s2 = src + head;
  for (int i = t; i < pairs; i += nt) d2[i] = bf16_rne(s2[2 * i]) | (bf16_rne(s2[2 * i + 1]) << 16);
  if (t == nt - 1 && head + 2 * pairs < n) dst[n - 1] = (unsigned short)bf16_rne(src[n - 1]);
}

// Gather side.  A row of n bf16 (134 bytes at D = 67) starts at a 2-byte aligned address.  Chosen: 16-byte loads (8 elements per
// lane) for everything from the row's first 16-byte boundary on, 2-byte loads for the <= 7 elements in front of that boundary and the
// <= 7 behind the last whole 16 bytes — no byte outside the row is read.  The pieces meet in LDS (ds_write_b128 for the body), and
// after one barrier lane c widens element c and stores it, so the fp32 stores (twice the bytes of the loads) stay coalesced exactly
// as in the fp32 gather.  For D = 67 a row costs 8 or 9 wide loads and <= 14 narrow ones in one load instruction each, instead of
// 67 two-byte loads over two waves.
constexpr int BF16_ROW_MAX = 1024;                 // longest row (D or A) the staged gather takes
constexpr int BF16_STAGE = BF16_ROW_MAX + 16;      // staging elements per row: the row plus the shift that aligns its body

// stage (16-byte aligned, BF16_STAGE elements) <- row; returns the offset o such that element c is stage[o + c].  t = 0 .. 127.
__device__ __forceinline__ int bf16_row_to_lds(const unsigned short *row, int n, int t, unsigned short *stage) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 1) & 7u);
  int head = (8 - mis) & 7;
  if (head > n) head = n;
  const int o = (8 - head) & 7;                    // body chunk j lands at stage[8 * (j + (head ? 1 : 0))]
  const int nb = (n - head) >> 3, tail = n - head - 8 * nb;
  const uint4 *body = reinterpret_cast<const uint4 *>(row + head);
  uint4 *sbody = reinterpret_cast<uint4 *>(stage + o + head);
  for (int j = t; j < nb; j += 128) sbody[j] = body[j];
  if (t < head) stage[o + t] = row[t];
  const int u = t - 64;                            // the tail on the second wave: no lane does more than one narrow load
  if (u >= 0 && u < tail) stage[o + head + 8 * nb + u] = row[head + 8 * nb + u];
  return o;
}

}  // namespace
#endif
