// dm_eval.hip — episode bookkeeping of a batched evaluation (evaluation.BatchEvaluator): one launch after every env step.
// Every env runs ONE episode.  The kernel adds the step into the episode sums of the envs still alive, retires the envs whose
// episode ended on this step (done flag, or max_steps reached) and rebuilds the ascending list of the envs that are still alive,
// which dm_step_active takes as its slot list: finished envs are not launched any more.
#include "dm_launch.h"

namespace {

constexpr int EV_BLOCK = 1024;            // one workgroup; n is walked in chunks of EV_BLOCK envs
constexpr int EV_WAVES = EV_BLOCK / 64;

// One workgroup: the compaction is a scan over all envs, and a few thousand envs are a few chunks.  No global atomics: the
// position of an env in env_ids is the number of live envs before it, so the list is the same on every run.
__global__ void __launch_bounds__(EV_BLOCK) eval_advance_kernel(int n, int terms_dim, int max_steps, const float *rew, const uint8_t *done,
                                                                const int32_t *reason, const float *terms, const float *obs, int obs_dim,
                                                                uint8_t *alive, int32_t *ep_len, double *ep_ret, double *ep_terms,
                                                                int32_t *ep_reason, float *last_obs, int32_t *env_ids, int32_t *count) {
  __shared__ int wave_total[EV_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int live_before = 0;                    // live envs of the chunks already walked (the same value in every thread)
  for (int base = 0; base < n; base += EV_BLOCK) {
    const int i = base + tid;
    bool live = false;
    if (i < n && alive[i]) {              // rows of finished envs are stale under compaction: neither read nor written
      const int len = ep_len[i] + 1;
      ep_len[i] = len;
      ep_ret[i] += (double)rew[i];
      if (terms)
        for (int k = 0; k < terms_dim; k++) ep_terms[(size_t)i * terms_dim + k] += (double)terms[(size_t)i * terms_dim + k];
      const bool d = done[i] != 0;
      if (d || len == max_steps) {        // done wins when both fall on this step
        ep_reason[i] = d ? reason[i] : DM_EVAL_TRUNCATED;
        if (obs && last_obs)
          for (int k = 0; k < obs_dim; k++) last_obs[(size_t)i * obs_dim + k] = obs[(size_t)i * obs_dim + k];
        alive[i] = 0;
      } else {
        live = true;
      }
    }
    const unsigned long long ballot = __ballot(live);
    if (lane == 0) wave_total[wave] = __popcll(ballot);
    __syncthreads();
    int before = live_before, chunk = 0;
    for (int w = 0; w < EV_WAVES; w++) {
      const int t = wave_total[w];
      if (w < wave) before += t;
      chunk += t;
    }
    if (live) env_ids[before + __popcll(ballot & ((1ull << lane) - 1ull))] = i;     // before + rank <= i < n
    live_before += chunk;
    __syncthreads();                      // wave_total is rewritten by the next chunk
  }
  for (int i = live_before + tid; i < n; i += EV_BLOCK) env_ids[i] = -1;
  if (tid == 0) count[0] = live_before;
}

}  // namespace

extern "C" int dm_eval_advance(int n, int terms_dim, int max_steps, const float *rew, const uint8_t *done, const int32_t *reason,
                               const float *terms, const float *obs, int obs_dim, uint8_t *alive, int32_t *ep_len, double *ep_ret,
                               double *ep_terms, int32_t *ep_reason, float *last_obs, int32_t *env_ids, int32_t *count, int device,
                               void *stream) {
  if (n < 1 || max_steps < 1 || device < 0 || !rew || !done || !reason || !alive || !ep_len || !ep_ret || !ep_reason || !env_ids || !count)
    return DM_EINVAL;
  if (terms && (terms_dim < 1 || !ep_terms)) return DM_EINVAL;
  if (obs && last_obs && obs_dim < 1) return DM_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return DM_EHIP;
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(EV_BLOCK), 0, (hipStream_t)stream, n, terms_dim, max_steps, rew, done, reason, terms,
                     obs, obs_dim, alive, ep_len, ep_ret, ep_terms, ep_reason, last_obs, env_ids, count);
  return dm_launch_status();
}
