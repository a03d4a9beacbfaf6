// dm_abi.hip — host side of libdeepmimic_hip.so: the C-ABI of include/deepmimic_hip.h.
// Builds the fp32 device tables from DmModel, owns the per-env HBM state rows and
// the clip tables, and launches the fused step kernel (dm_kernels.hip).
#include "../../include/deepmimic_hip.h"
#include "dm_tables_host.h"   // check_model, build_tables, pack_clip; dm_host.h: DmHost, HIPCHK, DM_DEVICE, DM_LAUNCH

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "dm_kernels.hip"

struct DmEngine : DmHost {
  DmConfig cfg;
  DmModel model;
  int N = 0;
  DmDev *dT = nullptr;
  float *dState = nullptr;
  float *dArScratch = nullptr;
  float *dClipRows[DM_MAX_CLIPS] = {nullptr};
  float *dClipReset[DM_MAX_CLIPS] = {nullptr};
  int clipL[DM_MAX_CLIPS] = {0};
  int clipFlags[DM_MAX_CLIPS] = {0};
  float *debug = nullptr;
  int32_t *dOrder = nullptr;   // slot -> env permutation for dm_step (longest-first)
  int32_t *dCost = nullptr;    // per-env work estimate written by dm_step
  static constexpr int NEV = 512;              // ring of event pairs: one per dm_step while timing is on
  hipEvent_t ev0[NEV] = {}, ev1[NEV] = {};
  long nrec = 0;                               // launches recorded since dm_enable_timing(1)
  long nlaunch = 0;                            // launches since dm_enable_timing
  int stride = 1;                              // every stride-th launch carries an event pair
  int waves = 0;                               // 0: kernel variant from the batch size; 2 / 3: forced (env DM_WAVES, experiments)
  bool timing = false;
  float last_ms = 0;
};

extern "C" void dm_default_config(DmConfig *c) {
  memset(c, 0, sizeof(*c));
  c->num_envs = 1;
  c->max_ep_length = 1000;   // src/deepmimic_env.py:260
  c->vel_obs_scale = 0.1f;   // :261
  c->low_z = 0.7f;           // src/config.py:13
  c->high_z = 2.0f;          // src/deepmimic_env.py:423
  c->w_pose = 0.75f; c->w_vel = 0.1f; c->w_end_eff = 0.15f; c->w_com = 0.0f; c->w_joint_limit = -0.1f;  // :400-404
  c->obs_bound = 100.0f;     // :465
  c->seed = 1234;
  c->auto_reset = 1;
  c->device = 0;
  c->lpt_schedule = 1;
  c->task = DM_TASK_DPENV;
  c->amnesty_steps = 150;    // src/combined_env.py:34
  c->to_getup_len = 180;     // :97
  c->integrator = DM_CFG_INT_MODEL;   // the XML's (RK4, xml :9)
}

// Everything dm_create puts on the device.  On failure e->err says why and the caller deletes e, which frees what was made.
static int dm_init(DmEngine *e) {
  const DmModel &m = e->model;
  if (check_model(m, e->err) != DM_OK) return DM_EINVAL;
  DM_DEVICE(e);
  DmDev T;
  build_tables(m, T);
  HIPCHK(e, e->alloc(&e->dT, 1));
  HIPCHK(e, e->upload(e->dT, &T, 1));
  const size_t N = (size_t)e->N;
  std::vector<float> init(N * DMK_STATE_STRIDE, 0.f);
  for (size_t i = 0; i < N; i++)
    for (int k = 0; k < DM_NQ; k++) init[i * DMK_STATE_STRIDE + DMS_QPOS + k] = (float)m.qpos0[k];
  HIPCHK(e, e->alloc(&e->dState, init.size()));
  HIPCHK(e, e->upload(e->dState, init.data(), init.size()));
  HIPCHK(e, e->alloc(&e->dArScratch, N * DMK_MAXROW * DMK_MAXROW));
  HIPCHK(e, e->alloc(&e->dCost, N));
  HIPCHK(e, e->fill(e->dCost, 0, N * sizeof(int32_t)));
  std::vector<int32_t> ident(N);
  for (size_t i = 0; i < N; i++) ident[i] = (int32_t)i;
  HIPCHK(e, e->alloc(&e->dOrder, N));
  HIPCHK(e, e->upload(e->dOrder, ident.data(), N));   // until the first dm_step schedules
  for (int i = 0; i < DmEngine::NEV; i++) { HIPCHK(e, e->event(&e->ev0[i])); HIPCHK(e, e->event(&e->ev1[i])); }
  return DM_OK;
}

extern "C" int dm_create(const DmModel *model, const DmConfig *cfg, DmHandle *out) {
  if (!model || !cfg || !out || cfg->num_envs < 1) return DM_EINVAL;
  if (!dm_have_device()) return DM_ENODEV;
  DmEngine *e = new DmEngine();
  e->cfg = *cfg;
  e->model = *model;
  e->device = cfg->device;
  e->N = cfg->num_envs;
  if (const char *w = getenv("DM_WAVES")) e->waves = atoi(w);
  const int rc = dm_init(e);
  if (rc != DM_OK) { fprintf(stderr, "dm_create: %s\n", e->err.c_str()); delete e; return rc; }
  *out = e;
  return DM_OK;
}

extern "C" int dm_destroy(DmHandle e) { return dm_destroy_engine(e); }

extern "C" const char *dm_last_error(DmHandle e) { return e ? e->err.c_str() : "null handle"; }
extern "C" int dm_num_envs(DmHandle e) { return e ? e->N : DM_EINVAL; }
extern "C" int dm_obs_dim(DmHandle e) { return e ? (e->cfg.task == DM_TASK_COMBINED ? DM_NOBS_COMBINED : DM_NOBS) : DM_EINVAL; }
extern "C" int dm_terms_dim(DmHandle e) { return e ? (e->cfg.task == DM_TASK_COMBINED ? 8 : 5) : DM_EINVAL; }

extern "C" int dm_load_clip(DmHandle e, int clip_id, int L, const double *qpos, const double *qvel,
                            const double *body_xpos, const double *geom_xpos) {
  if (!e || clip_id < 0 || clip_id >= DM_MAX_CLIPS || L < 1 || !qpos || !qvel || !body_xpos || !geom_xpos)
    return dm_fail(e, DM_EINVAL, "dm_load_clip: bad argument");
  DM_DEVICE(e);
  std::vector<float> rows((size_t)L * DMK_CLIP_ROW, 0.f), reset((size_t)L * DMK_RESET_ROW, 0.f);
  pack_clip(e->model, L, qpos, qvel, body_xpos, geom_xpos, rows.data(), reset.data());
  e->clipL[clip_id] = 0;   // an empty slot if the reload fails
  HIPCHK(e, e->reload({{&e->dClipRows[clip_id], &rows}, {&e->dClipReset[clip_id], &reset}}));
  e->clipL[clip_id] = L;
  return DM_OK;
}

__global__ void dm_schedule_kernel(const int32_t *cost, int32_t *order, int n);

__global__ void dm_set_clip_kernel(float *state, const int32_t *ids, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) reinterpret_cast<int *>(state + (size_t)i * DMK_STATE_STRIDE)[DMS_CLIP] = ids ? ids[i] : 0;
}
__global__ void dm_get_clip_kernel(const float *state, int32_t *ids, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ids[i] = reinterpret_cast<const int *>(state + (size_t)i * DMK_STATE_STRIDE)[DMS_CLIP];
}
__global__ void dm_counters_kernel(float *state, int n, int32_t *idx, int32_t *len, float *rew, const int32_t *sidx,
                                   const int32_t *slen) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int *si = reinterpret_cast<int *>(state + (size_t)i * DMK_STATE_STRIDE);
  if (sidx) si[DMS_IDX] = sidx[i];
  if (slen) si[DMS_EPLEN] = slen[i];
  if (idx) idx[i] = si[DMS_IDX];
  if (len) len[i] = si[DMS_EPLEN];
  if (rew) rew[i] = state[(size_t)i * DMK_STATE_STRIDE + DMS_EPREW];
}
__global__ void dm_get_state_kernel(const float *state, const int32_t *ids, int n, int N, float *qpos, float *qvel,
                                    float *warm, float *ctrl) {
  int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= n) return;
  int env = ids ? ids[slot] : slot;
  if (env < 0 || env >= N) return;
  const float *st = state + (size_t)env * DMK_STATE_STRIDE;
  if (qpos && lane < DM_NQ) qpos[(size_t)slot * DM_NQ + lane] = st[DMS_QPOS + lane];
  if (qvel && lane < DM_NV) qvel[(size_t)slot * DM_NV + lane] = st[DMS_QVEL + lane];
  if (warm && lane < DM_NV) warm[(size_t)slot * DM_NV + lane] = st[DMS_WARM + lane];
  if (ctrl && lane < DM_NU) ctrl[(size_t)slot * DM_NU + lane] = st[DMS_CTRL + lane];
}

extern "C" int dm_get_env_clips(DmHandle e, int32_t *clip_ids, void *stream) {
  if (!e || !clip_ids) return DM_EINVAL;
  DM_DEVICE(e);
  DM_LAUNCH(e, dm_get_clip_kernel, dim3((e->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->dState, clip_ids, e->N);
  return DM_OK;
}

extern "C" int dm_set_clip_flags(DmHandle e, int clip_id, int flags) {
  if (!e || clip_id < 0 || clip_id >= DM_MAX_CLIPS) return DM_EINVAL;
  e->clipFlags[clip_id] = flags;
  return DM_OK;
}

extern "C" int dm_set_env_clips(DmHandle e, const int32_t *clip_ids, void *stream) {
  if (!e) return DM_EINVAL;
  DM_DEVICE(e);
  DM_LAUNCH(e, dm_set_clip_kernel, dim3((e->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->dState, clip_ids, e->N);
  return DM_OK;
}

static void fill_launch(DmEngine *e, DmLaunch &P, int mode) {
  memset(&P, 0, sizeof(P));
  P.T = e->dT;
  P.state = e->dState;
  P.ar_scratch = e->dArScratch;
  for (int i = 0; i < DM_MAX_CLIPS; i++) { P.clips[i].rows = e->dClipRows[i]; P.clips[i].reset = e->dClipReset[i]; P.clips[i].L = e->clipL[i]; P.clips[i].flags = e->clipFlags[i]; }
  P.N = e->N; P.mode = mode; P.auto_reset = e->cfg.auto_reset; P.max_ep_length = e->cfg.max_ep_length;
  P.vel_obs_scale = e->cfg.vel_obs_scale; P.low_z = e->cfg.low_z; P.high_z = e->cfg.high_z; P.obs_bound = e->cfg.obs_bound;
  P.w_pose = e->cfg.w_pose; P.w_vel = e->cfg.w_vel; P.w_ee = e->cfg.w_end_eff; P.w_com = e->cfg.w_com; P.w_jl = e->cfg.w_joint_limit;
  P.seed = e->cfg.seed;
  P.amnesty_steps = e->cfg.amnesty_steps; P.to_getup_len = e->cfg.to_getup_len;
  P.integrator = e->cfg.integrator == DM_CFG_INT_EULER ? DM_INT_EULER : e->cfg.integrator == DM_CFG_INT_RK4 ? DM_INT_RK4 : e->model.integrator;
  P.f8 = e->cfg.stale_contact_slots ? 1 : 0;
  P.debug = e->debug;
}

// variant_n: the batch size the two- / three-wave choice is made for (0: nslots)
static int launch(DmEngine *e, DmLaunch &P, int nslots, void *stream, int variant_n = 0) {
  P.nslots = nslots;
  if (const char *why = dm_clips_missing(e->clipL, e->cfg.task == DM_TASK_COMBINED, false)) return dm_fail(e, DM_EINVAL, why);
  DM_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int evi = (int)(e->nrec % DmEngine::NEV);
  const bool rec = e->timing && (e->nlaunch++ % e->stride) == 0;
  if (rec) HIPCHK(e, hipEventRecord(e->ev0[evi], s));
  const dim3 grid((P.nslots + DMK_ENVS_PER_BLOCK - 1) / DMK_ENVS_PER_BLOCK), block(64 * DMK_ENVS_PER_BLOCK);
  // three waves per SIMD (168 VGPRs): faster than the two-wave build from 3 072 envs up since r2 (per-stage laundering of
  // the lane id: no hoisted lane-compare masks spilled across the stage loop): 13.4 vs 12.9 M at 4 096 envs, 21.4 vs
  // 17.5 M at 65 536
  const bool three_waves = e->waves == 3 || (e->waves == 0 && (variant_n > 0 ? variant_n : P.nslots) >= 3072);
  if (e->cfg.task == DM_TASK_COMBINED) {
    if (three_waves) DM_LAUNCH(e, dm_step_combined_kernel_w3, grid, block, 0, s, P);
    else DM_LAUNCH(e, dm_step_combined_kernel, grid, block, 0, s, P);
  } else if (three_waves) {
    DM_LAUNCH(e, dm_step_kernel_w3, grid, block, 0, s, P);
  } else {
    DM_LAUNCH(e, dm_step_kernel, grid, block, 0, s, P);
  }
  if (rec) { HIPCHK(e, hipEventRecord(e->ev1[evi], s)); e->nrec++; }
  return DM_OK;
}
// the longest-first launch order of a step from this state: the work estimates of the last dm_step
static int schedule(DmEngine *e, DmLaunch &P, void *stream) {
  if (!e->cfg.lpt_schedule) return DM_OK;
  DM_DEVICE(e);
  DM_LAUNCH(e, dm_schedule_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, e->dCost, e->dOrder, e->N);
  P.env_ids = e->dOrder;
  return DM_OK;
}

extern "C" int dm_reset(DmHandle e, const uint8_t *mask, const int32_t *idx_init, float *obs_out, void *stream) {
  if (!e) return DM_EINVAL;
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_RESET);
  P.mask = mask; P.idx_init = idx_init; P.obs = obs_out;
  return launch(e, P, e->N, stream);
}

extern "C" int dm_step(DmHandle e, const float *actions, float *obs, float *rew, uint8_t *done, float *terms,
                       int32_t *reason, float *terminal_obs, void *stream) {
  if (!e || !actions || !obs || !rew || !done) return dm_fail(e, DM_EINVAL, "dm_step: null buffer");
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_STEP);
  P.actions = actions; P.obs = obs; P.rew = rew; P.done = done; P.terms = terms; P.reason = reason; P.terminal_obs = terminal_obs;
  P.cost = e->dCost;
  const int rc = schedule(e, P, stream);
  return rc != DM_OK ? rc : launch(e, P, e->N, stream);
}

extern "C" int dm_step_active(DmHandle e, const float *actions, const int32_t *env_ids, int nslots, float *obs, float *rew,
                              uint8_t *done, float *terms, int32_t *reason, void *stream) {
  if (!e || !actions || !env_ids || !obs || !rew || !done || nslots < 1 || nslots > e->N) return dm_fail(e, DM_EINVAL, "dm_step_active: bad argument");
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_STEP);
  P.actions = actions; P.obs = obs; P.rew = rew; P.done = done; P.terms = terms; P.reason = reason;
  P.cost = e->dCost;
  P.auto_reset = 0;                      // a finished env keeps its terminal state
  P.env_ids = env_ids;                   // the caller's order: no longest-first schedule
  return launch(e, P, nslots, stream, e->N);   // the kernel variant of the whole batch, however few envs are left
}

extern "C" int dm_physics_step(DmHandle e, const float *actions, void *stream) {
  if (!e || !actions) return dm_fail(e, DM_EINVAL, "dm_physics_step: null buffer");
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_PHYSICS);
  P.actions = actions;
  P.auto_reset = 0;
  const int rc = schedule(e, P, stream);   // same launch order as a dm_step from this state
  return rc != DM_OK ? rc : launch(e, P, e->N, stream);
}

extern "C" int dm_step_forced(DmHandle e, const float *qpos, const float *qvel, float *obs, float *rew, uint8_t *done,
                              float *terms, int32_t *reason, void *stream) {
  if (!e || !qpos || !qvel || !obs || !rew || !done) return dm_fail(e, DM_EINVAL, "dm_step_forced: null buffer");
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_FORCED);
  P.in_qpos = qpos; P.in_qvel = qvel; P.obs = obs; P.rew = rew; P.done = done; P.terms = terms; P.reason = reason;
  P.auto_reset = 0;
  return launch(e, P, e->N, stream);
}

extern "C" int dm_set_state(DmHandle e, const int32_t *env_ids, int n, const float *qpos, const float *qvel,
                            const float *warm, const float *ctrl, int run_forward, void *stream) {
  if (!e || !qpos || !qvel || n < 1 || n > e->N) return dm_fail(e, DM_EINVAL, "dm_set_state: bad argument");
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_SETSTATE);
  P.env_ids = env_ids; P.in_qpos = qpos; P.in_qvel = qvel; P.in_warm = warm; P.in_ctrl = ctrl; P.run_forward = run_forward;
  return launch(e, P, n, stream);
}

extern "C" int dm_forward(DmHandle e, const int32_t *env_ids, int n, void *stream) {
  if (!e || n < 1 || n > e->N) return dm_fail(e, DM_EINVAL, "dm_forward: bad argument");
  DmLaunch P;
  fill_launch(e, P, DMK_MODE_SETSTATE);
  P.env_ids = env_ids; P.run_forward = 1;     // in_qpos == null: state is kept
  return launch(e, P, n, stream);
}

extern "C" int dm_get_state(DmHandle e, const int32_t *env_ids, int n, float *qpos, float *qvel, float *warm,
                            float *ctrl, void *stream) {
  if (!e || n < 1 || n > e->N) return dm_fail(e, DM_EINVAL, "dm_get_state: bad argument");
  DM_DEVICE(e);
  DM_LAUNCH(e, dm_get_state_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, e->dState, env_ids, n, e->N, qpos, qvel, warm, ctrl);
  return DM_OK;
}

extern "C" int dm_get_counters(DmHandle e, int32_t *idx, int32_t *len, float *rew, void *stream) {
  if (!e) return DM_EINVAL;
  DM_DEVICE(e);
  DM_LAUNCH(e, dm_counters_kernel, dim3((e->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->dState, e->N, idx, len, rew,
                     (const int32_t *)nullptr, (const int32_t *)nullptr);
  return DM_OK;
}
extern "C" int dm_set_counters(DmHandle e, const int32_t *idx, const int32_t *len, void *stream) {
  if (!e) return DM_EINVAL;
  DM_DEVICE(e);
  DM_LAUNCH(e, dm_counters_kernel, dim3((e->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->dState, e->N,
                     (int32_t *)nullptr, (int32_t *)nullptr, (float *)nullptr, idx, len);
  return DM_OK;
}

// Bucket sort of the per-env work estimates, heaviest first (one 1024-thread block; N <= 65536 in practice).
__global__ void dm_schedule_kernel(const int32_t *cost, int32_t *order, int n) {
  __shared__ int hist[256];
  __shared__ int base[256];
  const int tid = threadIdx.x;
  if (tid < 256) hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    int b = cost[i] >> 5;
    b = 255 - (b > 255 ? 255 : (b < 0 ? 0 : b));
    atomicAdd(&hist[b], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int b = 0; b < 256; b++) { base[b] = acc; acc += hist[b]; }
  }
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    int b = cost[i] >> 5;
    b = 255 - (b > 255 ? 255 : (b < 0 ? 0 : b));
    order[atomicAdd(&base[b], 1)] = i;
  }
}

extern "C" int dm_get_work(DmHandle e, int32_t *work_out, void *stream) {
  if (!e || !work_out) return DM_EINVAL;
  DM_DEVICE(e);
  HIPCHK(e, hipMemcpyAsync(work_out, e->dCost, e->N * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DM_OK;
}

extern "C" int dm_set_seed(DmHandle e, uint64_t seed) {
  if (!e) return DM_EINVAL;
  e->cfg.seed = seed;
  return DM_OK;
}

extern "C" int dm_set_debug(DmHandle e, float *buf) {
  if (!e) return DM_EINVAL;
  e->debug = buf;
  return DM_OK;
}

extern "C" int dm_fill_random_actions(DmHandle e, float *actions, uint32_t step_index, void *stream) {
  if (!e || !actions) return DM_EINVAL;
  DM_DEVICE(e);
  int n = e->N * DM_NU;
  DM_LAUNCH(e, dm_fill_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, actions, e->N, e->cfg.seed, step_index);
  return DM_OK;
}

extern "C" int dm_enable_timing(DmHandle e, int enable) {
  if (!e) return DM_EINVAL;
  e->timing = enable != 0;
  e->stride = enable > 1 ? enable : 1;
  e->nrec = 0;
  e->nlaunch = 0;
  return DM_OK;
}
extern "C" int dm_last_step_ms(DmHandle e, float *ms) {
  if (!e || !ms || !e->timing || e->nrec < 1) return DM_EINVAL;
  const int i = (int)((e->nrec - 1) % DmEngine::NEV);
  DM_DEVICE(e);
  HIPCHK(e, hipEventSynchronize(e->ev1[i]));
  HIPCHK(e, hipEventElapsedTime(ms, e->ev0[i], e->ev1[i]));
  return DM_OK;
}
extern "C" int dm_mean_step_ms(DmHandle e, float *ms, int32_t *count) {
  if (!e || !ms || !e->timing || e->nrec < 1) return DM_EINVAL;
  const long n = e->nrec < DmEngine::NEV ? e->nrec : DmEngine::NEV;
  DM_DEVICE(e);
  double acc = 0;
  for (long k = 0; k < n; k++) {
    const int i = (int)((e->nrec - 1 - k) % DmEngine::NEV);
    float t = 0;
    HIPCHK(e, hipEventSynchronize(e->ev1[i]));
    HIPCHK(e, hipEventElapsedTime(&t, e->ev0[i], e->ev1[i]));
    acc += t;
  }
  *ms = (float)(acc / (double)n);
  if (count) *count = (int32_t)n;
  return DM_OK;
}
