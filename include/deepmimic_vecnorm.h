/* VecNormalize C ABI (csrc/dm_vecnorm.hip, part of libdeepmimic_hip.so); Python side: deepmimic_mujoco_amd/vec_normalize.py.
 *
 * SB3's VecNormalize [EXT] for a batch of N envs with D observation columns: running mean / variance of the observations and of the
 * discounted returns (RunningMeanStd: fp64, mean 0, var 1, count 1e-4 at the start), and the two clipped transforms
 *   normalize_obs(x)    = float32(clip((x - mean) / sqrt(var + epsilon), -clip_obs, clip_obs))
 *   normalize_reward(r) = float32(clip(r / sqrt(ret_var + epsilon), -clip_reward, clip_reward))
 * with every operation before the final cast in fp64.  The engines are not known here.  All pointers are device pointers owned by
 * the caller; every call only enqueues kernels on `stream` (no host synchronisation, no atomics, fixed reduction order: two runs are
 * bit-identical and a captured hipGraph replays what eager execution computes) and returns 0 or a negative code.
 */
#ifndef DEEPMIMIC_VECNORM_H
#define DEEPMIMIC_VECNORM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_VECNORM_OK 0
#define DM_VECNORM_EINVAL (-22) /* = DM_EINVAL of include/deepmimic_hip.h */
#define DM_VECNORM_EHIP (-5)    /* = DM_EHIP */

typedef struct DmVecNorm {
    int32_t N, D, device;                      /* envs, observation columns (both >= 1), HIP device */
    int32_t training, norm_obs, norm_reward;   /* SB3's three flags */
    double gamma, epsilon, clip_obs, clip_reward;
    double* obs_mean;      /* [D] */
    double* obs_var;       /* [D] */
    double* obs_count;     /* [1] */
    double* ret_stats;     /* [3] mean, var, count of the discounted returns */
    double* returns;       /* [N] */
    double* scratch;       /* dm_vecnorm_scratch_bytes(N, D) bytes: per-chunk moments, rewritten by every training call */
    int64_t scratch_bytes; /* what `scratch` holds */
} DmVecNorm;

/* Bytes of DmVecNorm.scratch for N envs and D columns; negative for N < 1 or D < 1. */
long long dm_vecnorm_scratch_bytes(int N, int D);

/* SB3's step_wait after the inner step returned obs [N, D], rew [N], done uint8 [N], tobs [N, D] (terminal observations):
 * training and norm_obs: obs_rms.update(obs); obs_out = normalize_obs(obs) with the statistics just updated; training:
 * returns = returns * gamma + rew, ret_rms.update(returns) (also when norm_reward is 0); rew_out = normalize_reward(rew);
 * tobs_out rows of done envs = normalize_obs(tobs), the other rows are copied through; returns[done] = 0.  Each output pointer
 * equals its input pointer (in place) or names memory disjoint from every input.  tobs and tobs_out may both be NULL (no terminal
 * observations).  Three launches when training (per-chunk moments; merge in ascending chunk order and update; normalise), one
 * otherwise: then the statistics are not written at all. */
int dm_vecnorm_step(const DmVecNorm* vn, const float* obs, const float* rew, const uint8_t* done, const float* tobs, float* obs_out,
                    float* rew_out, float* tobs_out, void* stream);

/* SB3's reset: returns = 0; training and norm_obs: obs_rms.update(obs); obs_out = normalize_obs(obs).  At most three launches. */
int dm_vecnorm_reset(const DmVecNorm* vn, const float* obs, float* obs_out, void* stream);

/* The frozen transform of n rows (any n >= 1, not tied to N): obs_out [n, D] = normalize_obs(obs) and / or rew_out [n] =
 * normalize_reward(rew); a NULL pair is skipped, at least one pair is given.  One launch; reads the statistics, writes none, and
 * touches neither returns nor scratch (both may be NULL here). */
int dm_vecnorm_apply(const DmVecNorm* vn, int n, const float* obs, float* obs_out, const float* rew, float* rew_out, void* stream);

/* All three return DM_VECNORM_EINVAL before any HIP call for a NULL struct or required pointer, N < 1, D < 1, n < 1, a scratch
 * smaller than dm_vecnorm_scratch_bytes(N, D), gamma outside [0, 1], epsilon < 0 or a clip <= 0 (NaN included); the reason is kept
 * per host thread. */
const char* dm_vecnorm_last_error(void);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
/* For the translation units of the library that apply the transform inside a kernel of their own (csrc/dm_vecnorm.hip, and
 * dm_sac_gather_norm of csrc/dm_sac.hip: include/deepmimic_sac_norm.h): the ONE statement of it and of the struct checks, so that
 * what a replay minibatch gets is bit for bit what dm_vecnorm_apply gives.  `scale` is sqrt(var + epsilon), formed once per column
 * by the caller; the reward passes mean 0.  fp64 to the end: one rounding, at the cast. */
__device__ __forceinline__ float dm_vn_norm_one(double x, double mean, double scale, double clip) {
  double y = (x - mean) / scale;
  y = y < -clip ? -clip : (y > clip ? clip : y);
  return (float)y;
}

/* Why the fields every entry point reads are refused, or NULL when they are fine (`returns` and `scratch` are not looked at). */
static inline const char* dm_vn_struct_error(const DmVecNorm* v) {
  if (!v) return "null DmVecNorm";
  if (v->N < 1 || v->D < 1) return "N < 1 or D < 1";
  if (v->device < 0) return "device < 0";
  if (!v->obs_mean || !v->obs_var || !v->obs_count || !v->ret_stats) return "null statistics pointer in DmVecNorm";
  if (!(v->gamma >= 0.0 && v->gamma <= 1.0)) return "gamma outside [0, 1]";
  if (!(v->epsilon >= 0.0)) return "epsilon < 0";
  if (!(v->clip_obs > 0.0) || !(v->clip_reward > 0.0)) return "clip_obs or clip_reward <= 0";
  return 0;
}
#endif
#endif
