// Device helpers the three PPO learner files share (dm_ppo.hip, dm_ppo_mlp.hip, dm_ppo_wide.hip): the wave / block sums, the two
// forms of the minibatch advantage statistics and the fast tanh of the fused learners.
#ifndef DM_PPO_COMMON_H
#define DM_PPO_COMMON_H
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float ppo_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// block-wide sum of `v`, result valid in thread 0.  A wave butterfly, then thread 0 adds the waves: NOT sac_block_sum (dm_sac.hip),
// which is a fixed-order LDS tree whose result every thread reads.
__device__ __forceinline__ float ppo_block_sum(float v, float *red) {
  v = ppo_wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float s = 0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) s += red[i];
  return s;
}

// stats[0] = mean(adv), stats[1] = 1 / (std_unbiased(adv) + 1e-8); also clears the accumulators of the main kernel
__device__ __forceinline__ void ppo_prepare_body(const float *adv, int B, int normalize, float *stats, float *out8, float *grad_log_std,
                                                 int A) {
  __shared__ float red[16];
  float s = 0;
  for (int i = threadIdx.x; i < B; i += blockDim.x) s += adv[i];
  const float tot = ppo_block_sum(s, red);
  __shared__ float mean_s;
  if (threadIdx.x == 0) mean_s = tot / (float)B;
  __syncthreads();
  const float mean = mean_s;
  float q = 0;
  for (int i = threadIdx.x; i < B; i += blockDim.x) { const float d = adv[i] - mean; q += d * d; }
  const float qq = ppo_block_sum(q, red);
  if (threadIdx.x == 0) {
    if (normalize && B > 1) { stats[0] = mean; stats[1] = 1.0f / (sqrtf(qq / (float)(B - 1)) + 1e-8f); }
    else { stats[0] = 0.f; stats[1] = 1.f; }
  }
  if (threadIdx.x < 8) out8[threadIdx.x] = 0.f;
  if (grad_log_std && (int)threadIdx.x < A) grad_log_std[threadIdx.x] = 0.f;
}

// Advantage statistics of the minibatch by ONE block of 256 threads (stats[0] = mean, stats[1] = 1 / (std_unbiased + 1e-8)), as
// ppo_prepare_body, but with every load of the block in flight at once: the values are read into registers by independent
// loads instead of 2 x B / 256 dependent round trips — this block is the critical path of the launch.  B <= 8192.
__device__ __forceinline__ void mlp_adv_stats(const float *adv, int B, int normalize, float *stats, float *out8) {
  __shared__ float red[16];
  __shared__ float mean_s;
  constexpr int ITEMS = 32;
  float v[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    const int i = threadIdx.x + k * 256;
    v[k] = (i < B) ? adv[i] : 0.f;
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < ITEMS; k++) s += v[k];
  const float tot = ppo_block_sum(s, red);
  if (threadIdx.x == 0) mean_s = tot / (float)B;
  __syncthreads();
  const float mean = mean_s;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < ITEMS; k++) { const float d = v[k] - mean; q += ((int)threadIdx.x + k * 256 < B) ? d * d : 0.f; }
  const float qq = ppo_block_sum(q, red);
  if (threadIdx.x == 0) {
    if (normalize && B > 1) { stats[0] = mean; stats[1] = 1.0f / (sqrtf(qq / (float)(B - 1)) + 1e-8f); }
    else { stats[0] = 0.f; stats[1] = 1.f; }
  }
  if (threadIdx.x < 8) out8[threadIdx.x] = 0.f;
}

// tanh(x) = 1 - 2 / (1 + e^{2x}) on the hardware exp / rcp: absolute error ~1e-7 (the accurate tanhf costs ~40 instructions
// and a fused forward evaluates 12 k of them per workgroup).  Not lt_tanh (dm_ppo.hip), which switches to a polynomial near 0.
__device__ __forceinline__ float ppo_fast_tanh(float x) { return 1.f - __fdividef(2.f, 1.f + __expf(2.f * x)); }

}  // namespace
#endif
