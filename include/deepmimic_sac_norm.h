/* SAC's replay minibatch with SB3's VecNormalize applied at sample time (csrc/dm_sac.hip, part of libdeepmimic_hip.so); Python side:
 * deepmimic_mujoco_amd/sac.py, SAC(env, normalizer=HipVecNormalize(env)).
 *
 * SB3's ReplayBuffer._get_samples with a VecNormalize env [EXT]: the ring holds raw transitions, every sampled minibatch is
 * normalised with the statistics of that moment.  The entry point below is dm_sac_gather of include/deepmimic_hip.h (same draw,
 * same rows, same idx_out, same five layouts, one launch of B blocks) whose observation and next-observation columns go through
 * normalize_obs and whose reward goes through normalize_reward of include/deepmimic_vecnorm.h, with the same expression as
 * dm_vecnorm_apply: the outputs are bit for bit those of dm_sac_gather followed by dm_vecnorm_apply on obs2 and rew.  The action
 * columns of xq and `done` are copied through.  With norm_obs == 0 (norm_reward == 0) that half is a plain copy.
 *
 * What a captured hipGraph keeps: vn's flags norm_obs / norm_reward, epsilon and the two clips are launch arguments (values of the
 * moment of the capture; capture again after changing one), the statistics are read through vn->obs_mean, vn->obs_var and
 * vn->ret_stats when the kernel executes, so a replay sees the statistics of its moment.  vn->training, gamma, returns and scratch
 * are not read; nothing of vn is written.
 */
#ifndef DEEPMIMIC_SAC_NORM_H
#define DEEPMIMIC_SAC_NORM_H
#include "deepmimic_vecnorm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Returns 0, DM_VECNORM_EINVAL before any HIP call (a NULL vn or pointer other than idx_out, B, N, D or A < 1, vn->D != D, or a
 * field of vn that dm_vecnorm_apply refuses), or DM_VECNORM_EHIP if the launch was refused. */
int dm_sac_gather_norm(int B, int N, int D, int A, unsigned long long seed, const unsigned* counter, const unsigned* ring,
                       const float* r_obs, const float* r_act, const float* r_rew, const float* r_done, const float* r_next,
                       float* obs2, float* xq, float* xpi, float* xt, float* rew, float* done, int* idx_out, const DmVecNorm* vn,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
