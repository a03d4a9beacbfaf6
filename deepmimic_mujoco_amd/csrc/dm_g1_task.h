// dm_g1_task.h — what a step does around its forward evaluations: entry by launch mode, RK4 / Euler bookkeeping, the task layer of
// DPEnv(robot="unitree_g1") and DPCombinedEnv with the in-kernel auto-reset, and the write-back of the state row.
#pragma once
#include "dm_g1_device.h"
#include "dm_g1_math.h"
#include "dm_g1_dynamics.h"
#include "dm_rng.h"

namespace g1 {

// What a step carries from one evaluation to the next besides the LDS working set (registers in the monolithic kernel, a few
// words of the env's HBM slot between the launches of the split pipeline)
struct StepCtx {
  int idx_curr, ep_len, rcnt, motion, clip_id, reason, work, stage;   // stage: RK4 stage of the evaluation about to run / in flight
  unsigned stage_ncon, stage_nefc_lo;                                  // byte i = count at RK stage i (debug)
  float ep_rew, reward;
  bool sim_err, done, after_reset;
  ClipDev clip;
};

// The draw of reset number X.rcnt of an env (reference-state initialisation), for reset() without idx_init and for the auto-reset.
// DPEnv: a random frame of the env's clip.  DPCombinedEnv.reset(rsi=True) (combined_env.py:219-227): walk beyond the amnesty or
// getup, at a random frame.  Sets X.idx_curr (and X.motion, X.clip under the combined task); returns the clip frame to reset to.
__device__ __forceinline__ int rsi_draw(const Launch &P, const int env, StepCtx &X) {
  if (P.task != 0) {
    X.motion = (dm_hash32(P.seed, env, X.rcnt, 0x5EED) & 1) ? 2 : 0;
    X.clip = P.clips[X.motion];
    X.idx_curr = (int)(dm_hash32(P.seed, env, X.rcnt, 0x5EEE) % (uint32_t)X.clip.L) + (X.motion == 0 ? P.amnesty_steps + 10 : 0);
    return X.idx_curr % X.clip.L;
  }
  X.idx_curr = (int)(dm_hash32(P.seed, env, X.rcnt, 0x5EED) % (uint32_t)X.clip.L);
  return X.idx_curr;
}
__device__ __forceinline__ void load_reset_row(const ClipDev &clip, const int fi, const int lane) {
  const float *rr = clip.reset + (size_t)fi * RESET_ROW;
  if (lane < NQ) S.qpos[lane] = rr[RR_QPOS + lane];
  if (lane < NV) S.qvel[lane] = rr[RR_QVEL + lane];
}

// Loads the env's state row, applies the launch mode (action / forced state / reset state) and runs mj_checkPos / mj_checkVel.
// false: this env has nothing (more) to do in this launch.
__device__ __forceinline__ bool step_enter(const Launch &P, const Dev &T, const int env, const int lane, StepCtx &X) {
  const int mode = P.mode;
  if (mode == MODE_RESET && P.mask && !P.mask[env]) return false;
  float *st = P.state + (size_t)env * STATE;
  int *sti = (int *)st;
  X.idx_curr = sti[S_IDX]; X.ep_len = sti[S_EPLEN]; X.rcnt = sti[S_RCNT];
  X.ep_rew = st[S_EPREW];
  // TASK (DPCombinedEnv, src/combined_env.py): per-env motion 0 walk, 1 run, 2 getup, 3 to_getup; idx_curr is then the
  // unwrapped current_motion_n_steps
  const bool TASK = P.task != 0;
  X.motion = TASK ? sti[S_MOTION] : 0;
  X.motion = (X.motion < 0 || X.motion > 3) ? 0 : X.motion;
  // DPEnv task: the same slot holds the env's clip id (dmg1_set_env_clips; one DPEnv(motion=...) per worker in the reference)
  X.clip_id = TASK ? 0 : sti[S_MOTION];
  X.clip_id = (X.clip_id < 0 || X.clip_id >= DMG1_MAX_CLIPS) ? 0 : X.clip_id;
  if (TASK && (P.clips[0].L < 1 || P.clips[1].L < 1 || P.clips[2].L < 2)) return false;   // walk, run, getup all needed
  if (TASK) X.idx_curr = X.idx_curr < 0 ? 0 : X.idx_curr;
  if (lane < NQ) S.qpos[lane] = st[S_QPOS + lane];
  if (lane < NV) { S.qvel[lane] = st[S_QVEL + lane]; S.warm[lane] = st[S_WARM + lane]; }
  if (lane < NU) S.ctrl[lane] = st[S_CTRL + lane];
  SYNC();
  X.clip = P.clips[TASK ? (X.motion == 3 ? 2 : X.motion) : X.clip_id];
  if (X.clip.L < 1) return false;   // no clip loaded under this env's clip id
  if (mode == MODE_STEP) {
    if (lane < NU) S.ctrl[lane] = (lane < NACT) ? P.actions[(size_t)env * NACT + lane] * T.action_scale : 0.f;   // :348-351
  } else if (mode == MODE_FORCED || mode == MODE_SETSTATE) {
    if (P.in_qpos) {
      if (lane < NQ) S.qpos[lane] = P.in_qpos[(size_t)env * NQ + lane];
      if (lane < NV) S.qvel[lane] = P.in_qvel[(size_t)env * NV + lane];
    }
    if (mode == MODE_SETSTATE && P.in_warm && lane < NV) S.warm[lane] = P.in_warm[(size_t)env * NV + lane];
  } else if (mode == MODE_RESET) {
    int fi;
    if (!P.idx_init) fi = rsi_draw(P, env, X);
    else if (TASK) {   // idx_init keeps the motion
      X.idx_curr = P.idx_init[env] < 0 ? 0 : P.idx_init[env];
      fi = (X.motion == 3) ? 1 : X.idx_curr % X.clip.L;
    } else {
      fi = P.idx_init[env];
      fi = fi < 0 ? 0 : (fi >= X.clip.L ? X.clip.L - 1 : fi);
      X.idx_curr = fi;
    }
    load_reset_row(X.clip, fi, lane);
    X.ep_len = 0; X.ep_rew = 0; X.rcnt++;
  }
  SYNC();
  if (mode == MODE_SETSTATE && !P.run_forward) {
    if (lane < NQ) st[S_QPOS + lane] = S.qpos[lane];
    if (lane < NV) { st[S_QVEL + lane] = S.qvel[lane]; st[S_WARM + lane] = S.warm[lane]; }
    return false;
  }

  X.sim_err = false; X.done = false; X.after_reset = false;
  X.reason = 0; X.stage_ncon = 0; X.stage_nefc_lo = 0; X.work = 0; X.reward = 0; X.stage = 0;
  if (mode == MODE_STEP || mode == MODE_FORCED) {   // mj_checkPos / mj_checkVel
    const float a = (lane < NQ) ? S.qpos[lane] : 0.f, b = (lane < NV) ? S.qvel[lane] : 0.f;
    X.sim_err = __any(!(fabsf(a) <= MAXVALF) || !(fabsf(b) <= MAXVALF));
  }
  return true;
}

// MODE_STEP, after the evaluation of RK stage stage ([EXT] mj_step with mj_RungeKutta(4): A = (1/2, 1/2, 1), B = (1/6, 1/3, 1/3,
// 1/6)): accumulates, then leaves either the next stage's state in LDS (true: evaluate again) or the step's final state (false).
__device__ __forceinline__ bool rk_advance(const Launch &P, const Dev &T, const int env, const int lane, StepCtx &X) {
  const float h = T.timestep;
  const float Bw = (X.stage == 0 || X.stage == 3) ? 1.f / 6 : 1.f / 3;
  X.stage_ncon |= ((unsigned)S.info[0] & 0xFF) << (8 * X.stage); X.stage_nefc_lo |= ((unsigned)S.info[1] & 0xFF) << (8 * X.stage);
  if (P.debug) {   // 24-bit hash of the stage's contact list (geom pairs in order): the parity tests hold the index SETS bit-exact
    unsigned hsh = 0;
    for (int c = 0; c < S.info[0]; c++) hsh = (hsh * 131u + (unsigned)S.u.co.c_g1[c] * 97u + (unsigned)S.u.co.c_g2[c] + 1u) & 0xFFFFFFu;
    if (lane == 0) P.debug[(size_t)env * DMG1_DEBUG_STRIDE + DMG1_DBG_STAGE_CHASH + X.stage] = (float)hsh;
  }
  if (X.stage == 0) {
    const bool badv = (lane < NV) && !(fabsf(S.qacc[lane]) <= MAXVALF);   // mj_checkAcc
    X.sim_err = __any(badv);
    if (!X.sim_err) {
      if (lane < NQ) S.x0q[lane] = S.qpos[lane];
      if (lane < NV) { S.x0v[lane] = S.qvel[lane]; S.accq[lane] = 0.f; S.accv[lane] = 0.f; }
    }
  }
  if (!X.sim_err) {
    float dq = 0, dv = 0;
    if (lane < NV) {
      S.accq[lane] += Bw * S.qvel[lane]; S.accv[lane] += Bw * S.qacc[lane];
      const float a = (X.stage == 2) ? 1.f : 0.5f;
      dq = a * S.qvel[lane]; dv = a * S.qacc[lane];
    }
    SYNC();
    if (X.stage < 3) {
      if (lane < NV) S.tmp[lane] = dq;
      SYNC();
      integrate_pos(T, S.tmp, 1.0, true, lane);
      if (lane < NV) S.qvel[lane] = S.x0v[lane] + h * dv;
      SYNC();
      X.stage++;
      return true;
    }
    if (lane < NV) S.qvel[lane] = S.x0v[lane] + h * S.accv[lane];
    integrate_pos(T, S.accq, 1.0, false, lane);
    SYNC();
  }
  return false;
}

// MODE_STEP under DM_INT_EULER, after the step's one evaluation ([EXT] mj_step with mj_Euler): the bookkeeping of RK stage 0, then
// qvel += h qacc' with the joint damping implicit (euler_damped_qacc) and qpos integrated with the NEW qvel.  S.qacc and S.warm stay
// the evaluation's (MuJoCo's warm start is forward's qacc, not qacc'); the derived arrays the task layer reads are those of the
// pre-step pose.  Only the Euler kernels (template argument of the kernel bodies, dm_g1.hip) call it.  euler_integrate is out of
// line and does not take the StepCtx (whose address must not escape: it lives in registers); it returns mj_checkAcc's verdict.
__device__ __noinline__ bool euler_integrate(const Launch &P, const Dev &T, const int env, const int lane) {
  if (P.debug) {   // the contact hash of rk_advance, before anything reuses the contact arrays; the RK stages that do not exist read 0
    unsigned hsh = 0;
    for (int c = 0; c < S.info[0]; c++) hsh = (hsh * 131u + (unsigned)S.u.co.c_g1[c] * 97u + (unsigned)S.u.co.c_g2[c] + 1u) & 0xFFFFFFu;
    if (lane < 4) P.debug[(size_t)env * DMG1_DEBUG_STRIDE + DMG1_DBG_STAGE_CHASH + lane] = (lane == 0) ? (float)hsh : 0.f;
  }
  const bool badv = (lane < NV) && !(fabsf(S.qacc[lane]) <= MAXVALF);   // mj_checkAcc
  const bool sim_err = __any(badv);
  if (!sim_err) {
    if (lane < NQ) S.x0q[lane] = S.qpos[lane];
    euler_damped_qacc(T, P.qm + (size_t)env * QM_STRIDE, lane);
    if (lane < NV) S.qvel[lane] += T.timestep * S.tmp[lane];
    SYNC();
    integrate_pos(T, S.qvel, 1.0, false, lane);
    SYNC();
  }
  return sim_err;
}
// The stage-0 bookkeeping of rk_advance, then the step's final state.  Always false: no further evaluation.
__device__ __forceinline__ bool euler_advance(const Launch &P, const Dev &T, const int env, const int lane, StepCtx &X) {
  X.stage_ncon |= (unsigned)S.info[0] & 0xFF; X.stage_nefc_lo |= (unsigned)S.info[1] & 0xFF;
  X.sim_err = euler_integrate(P, T, env, lane);
  return false;
}

// ---------------------------------------------------------------------------------- phases of task_and_finish, in its order
// What the observation and the imitation reward leave for the phases behind them.  TaskObs: obs[lane], obs[64 + lane] | motion
// length, clip frame.  TaskRew: roll, pitch, yaw of the root in the state and in the clip frame | joint error summed over the reward
// joints and this lane's | the clip row of the frame
struct TaskObs { float a, b; int Lm, frame; };
struct TaskRew { float rc[3], rt[3], dsum, adiff; const float *cr; };

// Torso features and the observation of the last evaluation (_get_obs).  The derived arrays are those of that evaluation.
__device__ __forceinline__ void task_observation(const Launch &P, const Dev &T, const int lane, const StepCtx &X, TaskObs &O) {
  const bool TASK = P.task != 0;
  const int NOBS_T = TASK ? NOBS_C : NOBS;
  const float Sc = P.vel_obs_scale;
  const int tb = T.torso_body;
  float rpy[3], tq[4] = {S.xquat[tb][0], S.xquat[tb][1], S.xquat[tb][2], S.xquat[tb][3]};
  quat_to_rpy(tq, rpy);
  const float *cv = S.cvel[tb];
  float sy, cy;
  sincosf(-rpy[2], &sy, &cy);
  const float tor[8] = {rpy[0] * Sc, rpy[1] * Sc, (cy * cv[3] - sy * cv[4]) * Sc, (sy * cv[3] + cy * cv[4]) * Sc, cv[5] * Sc,
                        cv[0] * Sc, cv[1] * Sc, cv[2] * Sc};
  float rf = 0, lf = 0;
  unsigned xc = 0;   // bit k: extra-contact geom k (foot spheres, src/config.py:19-20) touches the floor
  for (int c = 0; c < S.info[0]; c++) {
    const int g1 = S.u.co.c_g1[c], g2 = S.u.co.c_g2[c];
    const bool fl = g1 == T.floor_geom || g2 == T.floor_geom;
    if ((g1 == T.rfoot_geom || g2 == T.rfoot_geom) && fl) rf = 1;
    if ((g1 == T.lfoot_geom || g2 == T.lfoot_geom) && fl) lf = 1;
    if (fl) for (int k = 0; k < 8; k++) if (g1 == T.extra_geom[k] || g2 == T.extra_geom[k]) xc |= 1u << k;
  }
  // motion length / frame: to_getup is a 180-step pseudo clip whose target is frame 1 of getup (combined_env.py:67-99)
  const int Lm = (TASK && X.motion == 3) ? P.to_getup_len : X.clip.L;
  const int frame = TASK ? ((X.motion == 3) ? 1 : X.idx_curr % X.clip.L) : X.idx_curr;
  float ph = TASK ? (float)(X.idx_curr % Lm) / (float)Lm : (float)X.idx_curr / (float)X.clip.L;
  ph = fminf(fmaxf(ph, 0.f), 1.f);
  auto obs_at = [&](int i) -> float {
    if (i < 37) return S.qpos[7 + i];
    if (i < 74) return S.qvel[6 + i - 37] * Sc;
    if (i < 82) return tor[i - 74];
    if (!TASK) return (i == 82) ? rf : (i == 83) ? lf : ph;
    // DPCombinedEnv._get_obs (:495-505): extra contacts (:27), phase, get_player_action_obs with PAWalk
    // (heading (1,0,0) in the yaw-aligned torso frame, one-hot index 0), pa_getup_state
    if (i < 90) return (float)((xc >> (i - 82)) & 1u);
    if (i == 90) return ph;
    if (i == 91) return cy;
    if (i == 92) return sy;
    if (i == 93) return 1.f;
    if (i == 96) return (X.motion == 3) ? 1.f : 0.f;
    if (i == 97) return (X.motion == 2) ? 1.f : 0.f;
    return 0.f;
  };
  O.a = obs_at(lane);
  if (lane < NOBS_T - 64) O.b = obs_at(64 + lane);
  O.Lm = Lm; O.frame = frame;
}

// calc_imitation_reward, unitree_g1 branch (:193-256): terms[0..4] and X.reward
__device__ __forceinline__ void imitation_reward(const Dev &T, const int lane, StepCtx &X, const int frame, float (&terms)[8], TaskRew &R) {
  const float *cr = X.clip.rows + (size_t)frame * CLIP_ROW;
  float e_cfg = 0, e_vel = 0, adiff = 0;
  int viol = 0;
  if (lane < NREW) {
    const int qi = T.rew_q[lane], vi = T.rew_v[lane];
    const float q = S.qpos[qi];
    e_cfg = fabsf(q - cr[CR_QPOS + lane]);
    adiff = e_cfg;
    e_vel = fabsf(cr[CR_QVEL + lane] - S.qvel[vi]);
    const int k = vi;
    viol = (q <= T.d_lo[k] * 0.99f) + (q >= T.d_hi[k] * 0.99f);
  }
  e_cfg = wave_sum(e_cfg); e_vel = wave_sum(e_vel);
  const float dsum = e_cfg;
  const float nviol = wave_sum((float)viol);
  float cq[4] = {S.qpos[3], S.qpos[4], S.qpos[5], S.qpos[6]}, tqq[4] = {cr[CR_ROOTQ], cr[CR_ROOTQ + 1], cr[CR_ROOTQ + 2], cr[CR_ROOTQ + 3]};
  quat_to_rpy(cq, R.rc);
  quat_to_rpy(tqq, R.rt);
  e_cfg += fabsf(R.rc[1] - R.rt[1]);
  float ee = 0;
  for (int e = 0; e < 4; e++) {
    const int g = T.ee_geom[e];
    for (int i = 0; i < 3; i++) { const float df = S.gpos[g][i] - cr[CR_EE + 3 * e + i]; ee += df * df; }
  }
  float cc[3];
  for (int i = 0; i < 3; i++) cc[i] = wave_sum((lane < NB) ? T.b_mass[lane] * S.xpos[lane][i] : 0.f) * T.total_mass_inv;
  const float *tc = X.clip.com + (size_t)frame * COM_ROW;
  float ce = 0;
  for (int i = 0; i < 3; i++) { const float df = tc[i] - cc[i]; ce += df * df; }
  terms[0] = expf(-e_cfg); terms[1] = expf(-0.1f * e_vel); terms[2] = expf(-40.f * ee); terms[3] = expf(-10.f * ce);
  terms[4] = nviol / (float)NREW;
  X.reward = 0.75f * terms[0] + 0.1f * terms[1] + 0.15f * terms[2] + 0.0f * terms[3] - 0.1f * terms[4];
  R.dsum = dsum; R.adiff = adiff; R.cr = cr;
}

// DPEnv termination (:418-442) and the frame counter.  zc: height of the centre of mass.
__device__ __forceinline__ void dpenv_termination(const Launch &P, const Dev &T, StepCtx &X, const TaskRew &R, const float zc) {
  if (!(X.clip.flags & 1)) {
    X.done = (zc < T.low_z) || (zc > P.high_z);
    X.reason = (zc < T.low_z) ? 1 : 2;
  }
  if (X.clip.flags & 4) {
    const float mx = 60.f * 3.14159265358979f / 180.f;
    if (fabsf(R.rc[0] - R.rt[0]) > mx || fabsf(R.rc[1] - R.rt[1]) > mx) { X.done = true; X.reason = 8; }
  }
  if (P.max_ep_length != 0 && X.ep_len >= P.max_ep_length) { X.done = true; X.reason = 3; }
  if ((X.clip.flags & 2) && X.idx_curr + 1 == X.clip.L) { X.done = true; X.reason = 4; }
  X.idx_curr = (X.idx_curr + 1) % X.clip.L;
}

// DPCombinedEnv: task reward (combined_env.py:338-354), motion state machine + termination (:393-445); terms[5..7]
__device__ __forceinline__ void combined_reward_and_motion(const Launch &P, const Dev &T, StepCtx &X, const TaskRew &R, const float zc, const int Lm,
                                                           float (&terms)[8]) {
  const float ALIM = 0.2617993877991494f, MAX_ANGLE = 1.0471975511965976f;   // deg2rad(15), deg2rad(60)
  const float *cr = R.cr;
  const float adiff = R.adiff;
  const float droll = fabsf(R.rc[0] - R.rt[0]), dpitch = fabsf(R.rc[1] - R.rt[1]);
  float imitation = X.reward, task_r = 0.f;
  if (X.motion == 0 || X.motion == 1) {   // heading + velocity error against the clip's root velocity
    const float ex = cr[CR_ROOTV] - S.qvel[0], ey = cr[CR_ROOTV + 1] - S.qvel[1];
    task_r = expf(-sqrtf(ex * ex + ey * ey) * 10.f);
  }
  if (X.motion == 3) { imitation = 0.f; task_r = expf(-(R.dsum + dpitch + droll) / 5.f) / 3.f; }
  // imitation * 0.7f + task_r * 0.3f, spelled as the FMA the compiler's contraction formed while this was one function: which of the
  // two products is fused decides the last bit, and the recording (tests/test_g1_step_bits_gpu.py) holds this one
  X.reward = fmaf(imitation, 0.7f, task_r * 0.3f);
  const unsigned long long badm = __ballot(adiff > ALIM);
  const bool all_close = !__any(!(adiff < ALIM));   // lanes >= 23 carry 0
  terms[5] = imitation; terms[6] = task_r;
  terms[7] = (float)(__popcll(badm) + (dpitch > ALIM ? 1 : 0) + (droll > ALIM ? 1 : 0));   // debug_n_bad_angles
  X.done = false; X.reason = 0;
  if (X.idx_curr >= Lm - 1) {   // out of time; :396 compares PlayerAction objects by identity: getup always hands over to run
    if (X.motion == 2) { X.motion = 1; X.idx_curr = 0; }
    if (X.motion == 3) { X.motion = 2; X.idx_curr = 0; }
  }
  if (dpitch < ALIM && droll < ALIM && all_close && X.motion == 3) { X.motion = 2; X.idx_curr = 0; }
  if (X.motion == 0 || X.motion == 1) {
    const bool fallen = (zc < T.low_z) || (zc > P.high_z) || (droll > MAX_ANGLE) || (dpitch > MAX_ANGLE);
    if (fallen) {
      if (!(X.idx_curr > P.amnesty_steps)) { X.done = true; X.reason = 7; }
      X.motion = 3; X.idx_curr = 0;
    }
  }
  if (P.max_ep_length != 0 && X.ep_len >= P.max_ep_length) { X.done = true; X.reason = 3; }
  X.clip = P.clips[X.motion == 3 ? 2 : X.motion];
  X.idx_curr += 1;   // :454 (not wrapped)
}

// The debug row of the last evaluation (include/deepmimic_g1_hip.h: DMG1_DBG_*)
__device__ __forceinline__ void debug_row(const Launch &P, const int env, const int lane, const StepCtx &X) {
  float *dbg = P.debug + (size_t)env * DMG1_DEBUG_STRIDE;
  for (int i = lane; i < NB * 3; i += 64) dbg[DMG1_DBG_XPOS + i] = (&S.xpos[0][0])[i];
  if (lane < NV) { dbg[DMG1_DBG_QACC_SMOOTH + lane] = S.qas[lane]; dbg[DMG1_DBG_QACC + lane] = S.qacc[lane]; }
  if (lane == 0) {
    dbg[DMG1_DBG_NSURV] = (float)S.info[5];
    for (int i = 0; i < 3; i++) dbg[DMG1_DBG_PAIR_CLASS + i] = (float)((S.info[6] >> (8 * i)) & 0xFF);
    dbg[DMG1_DBG_NCON] = S.info[0]; dbg[DMG1_DBG_NEFC] = S.info[1]; dbg[DMG1_DBG_SOLVER_ITER] = S.info[3]; dbg[DMG1_DBG_NLIMIT] = S.info[2];
    dbg[DMG1_DBG_OVERFLOW] = S.info[4];
    for (int i = 0; i < 4; i++) {
      dbg[DMG1_DBG_STAGE_NCON + i] = (float)((X.stage_ncon >> (8 * i)) & 0xFF);
      dbg[DMG1_DBG_STAGE_NEFC + i] = (float)((X.stage_nefc_lo >> (8 * i)) & 0xFF);
    }
  }
  if (lane < MAXCON) {
    float *o = dbg + DMG1_DBG_CONTACT + DMG1_DBG_CONTACT_STRIDE * lane;
    const bool on = lane < S.info[0];
    o[0] = on ? S.u.co.c_dist[lane] : 0.f; o[1] = on ? (float)S.u.co.c_g1[lane] : -1.f; o[2] = on ? (float)S.u.co.c_g2[lane] : -1.f;
    for (int i = 0; i < 3; i++) { o[3 + i] = on ? S.u.co.c_pos[lane][i] : 0.f; o[6 + i] = on ? S.u.co.c_frame[lane][i] : 0.f; }
  }
  for (int r = lane; r < MAXROW; r += 64) dbg[DMG1_DBG_EFC_FORCE + r] = (r < S.info[1]) ? P.rows[(size_t)env * 5 * MAXROW + 2 * MAXROW + r] : 0.f;
}

// reward, done, reason and terms of the step
__device__ __forceinline__ void task_outputs(const Launch &P, const int env, const int lane, const StepCtx &X, const float (&terms)[8]) {
  const int NTERMS = P.task != 0 ? 8 : 5;
  if (P.rew && lane == 0) P.rew[env] = X.reward;
  if (P.done && lane == 0) P.done[env] = X.done ? 1 : 0;
  if (P.reason && lane == 0) P.reason[env] = X.reason;
  if (P.terms && lane < NTERMS) P.terms[(size_t)env * NTERMS + lane] = (lane == 0) ? terms[0] : (lane == 1) ? terms[1] : (lane == 2) ? terms[2]
                                                          : (lane == 3) ? terms[3] : (lane == 4) ? terms[4] : (lane == 5) ? terms[5] : (lane == 6) ? terms[6] : terms[7];
}
__device__ __forceinline__ void write_obs(float *out, const Launch &P, const int env, const int lane, const TaskObs &O) {
  const int NOBS_T = P.task != 0 ? NOBS_C : NOBS;
  out[(size_t)env * NOBS_T + lane] = O.a;
  if (lane < NOBS_T - 64) out[(size_t)env * NOBS_T + 64 + lane] = O.b;
}

// VecEnv auto-reset inside the step: the terminal observation goes out, the env takes its next draw's state and counters
__device__ __forceinline__ void auto_reset(const Launch &P, const int env, const int lane, StepCtx &X, const TaskObs &O) {
  if (P.terminal_obs) write_obs(P.terminal_obs, P, env, lane, O);
  const int fi = rsi_draw(P, env, X);
  X.rcnt++;
  SYNC();
  load_reset_row(X.clip, fi, lane);
  X.ep_len = 0; X.ep_rew = 0;
  SYNC();
  X.after_reset = true;
  X.sim_err = false;
}

// Task layer of the last evaluation (observation, reward, termination, counters, outputs; SURVEY F6: the derived arrays are those
// of the LAST forward evaluation).  true: the env was reset inside the step (VecEnv auto-reset) and needs one more forward
// evaluation at the reset state (set_state -> sim.forward) before its observation can be written.
__device__ __forceinline__ bool task_and_finish(const Launch &P, const Dev &T, const int env, const int lane, StepCtx &X) {
  const int mode = P.mode;
  const bool task_pass = !X.after_reset && (mode == MODE_STEP || mode == MODE_FORCED);
  TaskObs O = {0, 0, 0, 0};
  float terms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (X.sim_err) {
    X.reward = 0; X.done = true; X.reason = 5;
    SYNC();
    if (lane < NQ) S.qpos[lane] = T.qpos0[lane];
    if (lane < NV) { S.qvel[lane] = 0; S.warm[lane] = 0; }
    if (lane < NU) S.ctrl[lane] = 0;
    SYNC();
  } else {
    task_observation(P, T, lane, X, O);
    if (task_pass) {
      TaskRew R;
      imitation_reward(T, lane, X, O.frame, terms, R);
      // ---- termination (:418-442)
      const float zc = wave_sum((lane < NB) ? T.b_mass[lane] * S.xipos[lane][2] : 0.f) * T.total_mass_inv;
      if (P.task != 0) combined_reward_and_motion(P, T, X, R, zc, O.Lm, terms);
      else dpenv_termination(P, T, X, R, zc);
      X.ep_rew += X.reward;
      X.ep_len += 1;
      // :465 reads `np.max(obs) > 100 or np.min(obs) < -100`, which a NaN passes (the oracle restates it literally).  Written
      // here as "not inside the bound" ON PURPOSE, so that a NaN ends the episode with zeros like any other divergence instead of
      // reaching the policy; with finite values the two agree, and mj_checkPos / Vel / Acc catch a NaN state before this line.
      const bool ob = !(fabsf(O.a) <= P.obs_bound) || !(fabsf(O.b) <= P.obs_bound);
      if (__any(ob)) {
        O.a = 0; O.b = 0; X.reward = 0; X.done = true; X.reason = 6;
        for (int i = 0; i < 8; i++) terms[i] = 0;
      }
    }
  }
  if (P.debug && !X.after_reset) debug_row(P, env, lane, X);
  if (task_pass) {
    task_outputs(P, env, lane, X, terms);
    if (X.done && P.auto_reset && mode == MODE_STEP) {
      auto_reset(P, env, lane, X, O);
      return true;   // one more forward evaluation at the reset state (set_state -> sim.forward)
    }
  }
  if (P.obs) write_obs(P.obs, P, env, lane, O);
  return false;
}

__device__ __forceinline__ void step_write_back(const Launch &P, const int env, const int lane, const StepCtx &X) {
  const int mode = P.mode;
  const bool TASK = P.task != 0;
  float *st = P.state + (size_t)env * STATE;
  int *sti = (int *)st;
  if (lane < NQ) st[S_QPOS + lane] = S.qpos[lane];
  if (lane < NV) { st[S_QVEL + lane] = S.qvel[lane]; st[S_WARM + lane] = S.warm[lane]; }
  if (lane < NU) st[S_CTRL + lane] = S.ctrl[lane];
  if (lane == 0) { sti[S_IDX] = X.idx_curr; sti[S_EPLEN] = X.ep_len; st[S_EPREW] = X.ep_rew; sti[S_RCNT] = X.rcnt; if (TASK) sti[S_MOTION] = X.motion; }
  if (P.cost && mode == MODE_STEP && lane == 0) P.cost[env] = X.work;
}

}  // namespace g1
