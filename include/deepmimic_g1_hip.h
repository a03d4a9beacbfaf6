/*
 * deepmimic_g1_hip.h — C-ABI of the Unitree G1 engine inside libdeepmimic_hip.so (MI355X / gfx950).
 *
 * Second robot of the reference: DPEnv(robot="unitree_g1") (src/deepmimic_env.py:272-484 with the unitree_g1 branches
 * at :204-211, :244-246, :303-307, :348-351, :426-433; model src/mujoco/humanoid_deepmimic/envs/asset/
 * deepmimic_unitree_g1.xml).  Same conventions as deepmimic_hip.h: plain pointers and sizes, 0 or a negative DM_E* code,
 * caller-owned DEVICE buffers unless the name says host_, stream-ordered on the hipStream_t passed as void*.
 *
 * The model argument is `struct DmModel` of include/dm_model.h compiled with -DDM_ROBOT_G1 (nq 44, nv 43, 94 geoms, the
 * trailing G1 fields: friction loss, mesh hull vertices, task constants); model_bytes must equal its sizeof.
 */
#ifndef DEEPMIMIC_G1_HIP_H
#define DEEPMIMIC_G1_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DmG1Engine *DmG1Handle;

#define DMG1_NQ 44
#define DMG1_NV 43
#define DMG1_NU 37
#define DMG1_NACT 23   /* policy actions: the 14 hand motors are held at 0 (src/deepmimic_env.py:303-307) */
#define DMG1_NOBS 85   /* qpos[7:] 37 | 0.1 qvel[6:] 37 | torso 8 | foot contacts 2 | phase 1 (src/deepmimic_env.py:33-45) */
#define DMG1_NOBS_COMBINED 98 /* DPCombinedEnv: 82 + extra contacts 8 + phase 1 + player-action obs 7 (src/combined_env.py:495-505) */
#define DMG1_NBODY 39
#define DMG1_NGEOM 94
#define DMG1_MAXCON 48  /* contact slots per forward evaluation (MuJoCo: nconmax 200, xml :10) */
#define DMG1_MAXROW 256 /* constraint rows per forward evaluation: 37 friction-loss + limits + 4 per contact */
#define DMG1_DEBUG_STRIDE 1024
#define DMG1_MAX_CLIPS 8   /* clip slots per engine (as DM_MAX_CLIPS of deepmimic_hip.h) */

/* Integrator selector (DmG1Config.integrator): the constants of deepmimic_hip.h */
#ifndef DM_CFG_INT_MODEL
#define DM_CFG_INT_MODEL 0
#define DM_CFG_INT_EULER 1
#define DM_CFG_INT_RK4 2
#endif

typedef struct DmG1Config {
  int32_t num_envs;
  int32_t max_ep_length;   /* 1000 (DPEnvConfig.MAX_EP_LENGTH) */
  float vel_obs_scale;     /* 0.1 */
  float high_z;            /* 2.0; low_z comes from the model (RobotConfig.low_z = 0.4) */
  float obs_bound;         /* 100.0 */
  uint64_t seed;
  int32_t auto_reset;
  int32_t device;
  int32_t task;            /* 0: DPEnv (src/deepmimic_env.py); 1: DPCombinedEnv (src/combined_env.py:101-533) as the reference runs
                            * it: clips 0, 1, 2 = walk, run, getup_facedown_towalk, per-env motion 0 walk 1 run 2 getup 3 to_getup,
                            * obs 98, terms 8 (the five imitation terms, imitation_reward, task_reward, debug_n_bad_angles),
                            * max_ep_length 2000 */
  int32_t amnesty_steps;   /* 150 (DPCombinedEnvConfig.AMNESTY_STEPS, combined_env.py:34) */
  int32_t to_getup_len;    /* 180 (MTToGetup.length, combined_env.py:97) */
  int32_t pipeline;        /* how dmg1_step runs: 0 (default) = split pipeline from 512 envs up, else monolithic; 1 = monolithic (one wave
                            * runs its env's whole step); 2 = split (per evaluation a per-env launch and a batch-wide narrowphase launch with
                            * one wave per colliding PAIR; ~135 KB of device memory per env).  Same results either way. */
  int32_t integrator;      /* DmConfig.integrator's meaning and constants: DM_CFG_INT_MODEL (default) = <option integrator> of the
                            * model (RK4, xml :7; a model struct with DM_INT_EULER steps with Euler); DM_CFG_INT_EULER = MuJoCo's
                            * semi-implicit Euler with implicit joint damping [EXT mj_Euler]: one forward evaluation per step
                            * instead of four; DM_CFG_INT_RK4.  Any other value: dmg1_create returns DM_EINVAL and
                            * dmg1_last_error(NULL) says why. */
} DmG1Config;

void dmg1_default_config(DmG1Config *cfg);
size_t dmg1_model_sizeof(void);

/* Replaces MujocoEnv.__init__(xml, 6) (src/deepmimic_env.py:301) for robot="unitree_g1", one instance per batch. */
int dmg1_create(const void *model, size_t model_bytes, const DmG1Config *cfg, DmG1Handle *out);
int dmg1_destroy(DmG1Handle h);
/* Text of the handle's last failure; with a NULL handle, why the last dmg1_create failed ("null handle" before any did). */
const char *dmg1_last_error(DmG1Handle h);

/* Replaces DPEnv.load_mocap (src/deepmimic_env.py:321-324): HOST float64 tables of MocapDM(robot="unitree_g1"):
 * qpos[L*44], qvel[L*43], body_xpos[L*39*3], geom_xpos[L*94*3].  flags: 1 floor motion, 2 acyclical motion
 * (src/config.py:36-37), 4 the "run" roll / pitch rule (src/deepmimic_env.py:426-433).  clip_id 0..DMG1_MAX_CLIPS-1; the
 * DPCombinedEnv task reads slots 0, 1, 2 = walk, run, getup. */
int dmg1_load_clip(DmG1Handle h, int clip_id, int L, const double *host_qpos, const double *host_qvel, const double *host_body_xpos,
                   const double *host_geom_xpos, int flags);

/* Replaces DPEnv.reset() / reset_model(idx_init) (src/deepmimic_env.py:496-510).  mask NULL = all envs; idx_init NULL =
 * random frame (reference_state_init).  obs_out float[N*85]. */
int dmg1_reset(DmG1Handle h, const uint8_t *mask, const int32_t *idx_init, float *obs_out, void *stream);

/* Replaces DPEnv.step(action) for every env (src/deepmimic_env.py:335-484) plus the VecEnv worker's auto-reset.
 * actions float[N*23] (scaled by 20 and padded with 14 zeros inside, :348-351); obs float[N*85]; rew float[N]; done uint8[N];
 * terms float[N*5]; reason int32[N] (DM_REASON_* of deepmimic_hip.h, 8 = run angle rule); terminal_obs float[N*85].
 * terms, reason, terminal_obs may be NULL.
 * Launches per step.  Monolithic pipeline: one g1_step_kernel (RK4: its wave runs 4 evaluations) or one g1_step_euler_kernel (1
 * evaluation), + 1 evaluation at the reset state of an env that ended.  Split pipeline: RK4 6 g1_env_kernel + 5 g1_pair_kernel (4 RK
 * stages + the evaluation at the reset state), Euler 3 g1_env_euler_kernel + 2 g1_pair_kernel (the evaluation + the one at the
 * reset state).  From 512 envs up one g1_schedule_kernel goes in front. */
int dmg1_step(DmG1Handle h, const float *actions, float *obs, float *rew, uint8_t *done, float *terms, int32_t *reason,
              float *terminal_obs, void *stream);

/* dmg1_step over a slot list, for runs in which envs drop out (evaluation.BatchEvaluator(compact="all")): the contract of
 * dm_step_active (deepmimic_hip.h).  Slot s < nslots steps env env_ids[s] (device int32[>= nslots]); an entry outside
 * [0, num_envs) — the -1 padding of dm_eval_advance — ends that slot's workgroup at once, in every launch of the step, so a padded
 * list may be launched with an nslots that is only an upper bound of the live entries.  An env listed twice is a caller's error.  No
 * auto-reset, whatever DmG1Config.auto_reset says: an env that is done keeps its terminal state (and its reset count), and an env
 * that is not listed is not launched: its state row, counters, motion / clip slot and output rows are neither read nor written.
 * actions, obs, rew, done, terms, reason are the full [num_envs, ...] arrays of dmg1_step, indexed by ENV; terms and reason may be
 * NULL.  The pipeline is the one dmg1_step takes for the engine (DmG1Config.pipeline and num_envs), never a function of nslots:
 * an env's trajectory does not depend on how many others are still listed, nor on the order of the list.  The grids are nslots
 * workgroups (the pair kernel's persistent grid is sized from nslots).  From 512 envs up the listed envs are launched
 * longest-first like dmg1_step's (the permuted list goes to a buffer of the engine; env_ids is only read).  The per-env work
 * estimates behind that order are updated for the stepped envs only.  1 <= nslots <= num_envs; a null handle, actions, env_ids, obs,
 * rew or done, or an nslots outside that range, returns DM_EINVAL, sets the dmg1_last_error text and launches nothing. */
int dmg1_step_active(DmG1Handle h, const float *actions, const int32_t *env_ids, int nslots, float *obs, float *rew, uint8_t *done,
                     float *terms, int32_t *reason, void *stream);
/* on = 0: dmg1_step_active launches its slots in the caller's order (no longest-first pass); default 1.  Result-neutral. */
int dmg1_set_active_schedule(DmG1Handle h, int on);

/* Replaces DPEnv.step(action, force_state=(qpos, qvel)) (src/deepmimic_env.py:355-357).  qpos float[N*44], qvel float[N*43]. */
int dmg1_step_forced(DmG1Handle h, const float *qpos, const float *qvel, float *obs, float *rew, uint8_t *done,
                     float *terms, int32_t *reason, void *stream);

/* MujocoEnv.set_state (+ sim.forward) / sim.get_state for all N envs; qacc_warmstart may be NULL. */
int dmg1_set_state(DmG1Handle h, const float *qpos, const float *qvel, const float *qacc_warmstart, int run_forward,
                   void *stream);
int dmg1_get_state(DmG1Handle h, float *qpos, float *qvel, float *qacc_warmstart, void *stream);
int dmg1_get_counters(DmG1Handle h, int32_t *idx_curr, int32_t *episode_length, float *episode_reward, void *stream);
int dmg1_set_counters(DmG1Handle h, const int32_t *idx_curr, const int32_t *episode_length, void *stream);

/* Row width of the obs buffers for the configured task (85 / 98); per-env motion id of the DPCombinedEnv task
 * (env.current_motion_mocap, combined_env.py:190; under that task dmg1_get/set_counters' idx_curr is current_motion_n_steps). */
/* Replaces: gym.Env.seed() / VecEnv.seed() (random.seed for reference_state_init, src/deepmimic_env.py:313): re-keys the
 * counter-based generator of the random-frame (RSI) resets.  Takes effect from the next launch. */
int dmg1_set_seed(DmG1Handle h, uint64_t seed);
int dmg1_obs_dim(DmG1Handle h);
int dmg1_get_motion(DmG1Handle h, int32_t *motion, void *stream);
/* DPEnv task: per-env clip id (one `DPEnv(motion=...)` per SubprocVecEnv worker in the reference; multi-clip batches as in
 * BASELINE config 5) — the same state slot as the motion id of the combined task.  clip_ids device int32[N]. */
int dmg1_set_env_clips(DmG1Handle h, const int32_t *clip_ids, void *stream);
int dmg1_get_env_clips(DmG1Handle h, int32_t *clip_ids, void *stream);
int dmg1_set_motion(DmG1Handle h, const int32_t *motion, void *stream);

/* Parity-test hook: per-env dump of the last forward evaluation, float[N*DMG1_DEBUG_STRIDE] (NULL switches it off):
 *  [0:117) xpos | [117:160) qacc_smooth | [160:203) qacc | 203 ncon | 204 nefc | 205 solver_iter | 206 nlimit | 207 overflow |
 *  [208:208+48*9) per contact: dist, geom1, geom2, pos3, normal3 | [640:640+256) efc_force |
 *  after a step, per RK stage k = 0..3: 1000+k contacts, 1004+k rows (low byte), 1012+k a 24-bit hash of the stage's contact
 *  list h <- (131 h + 97 geom1 + geom2 + 1) mod 2^24 (the oracle keeps the same: "stage_chash<k>"); under the Euler integrator
 *  the step has stage 0 only and the entries of k = 1..3 are written as 0 |
 *  1008 broadphase survivors, 1009 / 1010 / 1011 of them analytic, plane - mesh and MPR pairs |
 *  [900:916) per-phase clock sums of the diagnostic build (-DG1_PROFILE) */
#define DMG1_DBG_XPOS 0
#define DMG1_DBG_QACC_SMOOTH 117
#define DMG1_DBG_QACC 160
#define DMG1_DBG_NCON 203
#define DMG1_DBG_NEFC 204
#define DMG1_DBG_SOLVER_ITER 205
#define DMG1_DBG_NLIMIT 206
#define DMG1_DBG_OVERFLOW 207
#define DMG1_DBG_CONTACT 208        /* DMG1_MAXCON records of DMG1_DBG_CONTACT_STRIDE floats */
#define DMG1_DBG_CONTACT_STRIDE 9
#define DMG1_DBG_EFC_FORCE 640      /* DMG1_MAXROW floats */
#define DMG1_DBG_PROF 900
#define DMG1_DBG_STAGE_NCON 1000
#define DMG1_DBG_STAGE_NEFC 1004
#define DMG1_DBG_NSURV 1008
#define DMG1_DBG_PAIR_CLASS 1009    /* analytic, plane - mesh, MPR */
#define DMG1_DBG_STAGE_CHASH 1012
int dmg1_set_debug(DmG1Handle h, float *debug);

/* Diagnostics of the split pipeline: per round r = 0..5 of the LAST dmg1_step or dmg1_step_active, whichever came last,
 * host_out[4 r + 0 / 1 / 2] = tickets of support-query pairs (MPR, plane-mesh), of analytic pairs, and tickets pulled.
 * Synchronises the device.  Zeros when monolithic, and for the rounds that did not run (an Euler step has rounds 0..2, of which
 * 0 and 1 file tickets). */
int dmg1_queue_counters(DmG1Handle h, int32_t *host_out24);

/* Test hooks of the separating-direction cache of the MPR pairs (result-neutral by design; tests/test_g1_pair_cover_gpu.py).
 * dmg1_set_null_cache: on != 0 makes every later launch of the monolithic kernel run np_convex without its cache (the pair
 * kernel of the split pipeline keeps its own).  dmg1_sep_cache_entries: host_out[0] = live entries (pair id >= 0) of the
 * monolithic kernel's 16-entry-per-env cache, host_out[1] = of the split pipeline's one-entry-per-(env, pair) cache (0 when
 * monolithic).  Synchronises the device. */
int dmg1_set_null_cache(DmG1Handle h, int on);
int dmg1_sep_cache_entries(DmG1Handle h, int32_t *host_out2);

/* Kernel time of the last dmg1_step or dmg1_step_active (whichever came last) in ms (HIP events on the launch stream), or < 0. */
float dmg1_last_kernel_ms(DmG1Handle h);

#ifdef __cplusplus
}
#endif
#endif
