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

/* ---- One set of running statistics over several ranks.  Beside the running statistics above, which the kernels go on
 * reading, a rank keeps two more fp64 moment sets laid out obs mean [D] | obs var [D] | obs count | ret mean, var, count:
 * `base`, what every rank agreed on at the last synchronisation (at the start RunningMeanStd's mean 0, var 1, count 1e-4), and
 * `acc`, what this rank alone has seen since (empty: all zero).  Every merge of two sets is dm_vn_merge below: SB3's
 * update_from_moments, with a set of count 0 skipped exactly. */
typedef struct DmVecNormSync {
    int32_t world, rank; /* ranks (>= 1), this rank in [0, world) */
    double* base;        /* [2 D + 4] */
    double* acc;         /* [2 D + 4] */
    double* gather;      /* [world, 2 D + 4]: the buffer of the one all-reduce (sum) between sync_pack and sync_merge */
} DmVecNormSync;

/* dm_vecnorm_step / dm_vecnorm_reset with the statistics kept as above; same arguments and aliasing rules.  Training: the batch
 * moments of the N rows (the same per-chunk launch), then acc = merge(acc, batch) and running = merge(base, acc), then the
 * transform with `running`: three launches; one otherwise.  `base` is only read. */
int dm_vecnorm_step_sync(const DmVecNorm* vn, const float* obs, const float* rew, const uint8_t* done, const float* tobs,
                         float* obs_out, float* rew_out, float* tobs_out, const DmVecNormSync* sync, void* stream);
int dm_vecnorm_reset_sync(const DmVecNorm* vn, const float* obs, float* obs_out, const DmVecNormSync* sync, void* stream);

/* The two launches around the collective.  pack: row `rank` of gather = acc, every other row = 0, so that a sum over the ranks
 * gathers (adding zeros is exact).  merge: base = merge(base, row 0, row 1, ..., row world - 1) in that order, acc = empty,
 * running = base.  After it the 2 D + 4 doubles of `running` are bit-identical on every rank.  One launch each; of vn they read
 * N (unused), D, device and the four statistics pointers. */
int dm_vecnorm_sync_pack(const DmVecNorm* vn, const DmVecNormSync* sync, void* stream);
int dm_vecnorm_sync_merge(const DmVecNorm* vn, const DmVecNormSync* sync, void* stream);

/* All of them return DM_VECNORM_EINVAL before any HIP call for a NULL struct or required pointer, N < 1, D < 1, n < 1, a scratch
 * smaller than dm_vecnorm_scratch_bytes(N, D), gamma outside [0, 1], epsilon < 0 or a clip <= 0 (NaN included), and the four
 * entry points with a DmVecNormSync also for a NULL descriptor, a NULL pointer in it, world < 1 or rank outside [0, world); the
 * reason is kept per host thread. */
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

/* The ONE merge of two moment sets (mean, population variance, count), a <- merge(a, b): RunningMeanStd.update_from_moments with b
 * as the batch.  A set of count 0 is skipped exactly: the other operand comes through bit for bit.  Not contracted into fused
 * multiply-adds, so that every kernel that inlines it rounds alike. */
__device__ __forceinline__ void dm_vn_merge(double& mean, double& var, double& count, double mb, double vb, double nb) {
#pragma clang fp contract(off)
  if (nb == 0.0) return;
  if (count == 0.0) {
    mean = mb;
    var = vb;
    count = nb;
    return;
  }
  const double d = mb - mean, tot = count + nb;
  const double new_var = (var * count + vb * nb + d * d * count * nb / tot) / tot;
  mean = mean + d * nb / tot;
  var = new_var;
  count = tot;
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

static inline const char* dm_vn_sync_error(const DmVecNormSync* y) {
  if (!y) return "null DmVecNormSync";
  if (y->world < 1) return "world < 1";
  if (y->rank < 0 || y->rank >= y->world) return "rank outside [0, world)";
  if (!y->base || !y->acc || !y->gather) return "null pointer in DmVecNormSync";
  return 0;
}
#endif
#endif
