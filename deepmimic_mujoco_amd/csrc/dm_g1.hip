// dm_g1.hip — Unitree G1 engine (second robot of the reference: DPEnv(robot="unitree_g1"), src/deepmimic_env.py:272-484;
// model deepmimic_unitree_g1.xml: nq 44, nv 43, 39 bodies, 94 geoms of which 46 collide, 32 convex meshes, friction loss).
//
// Same mapping as the humanoid3d kernel: ONE 64-lane wavefront per environment, all per-env intermediates in LDS, lanes changing
// role per phase.  The dof tree is walked through tables (the row solves of the constraint stage through the compile-time topology,
// dm_g1_topology.h), the Jacobian rows and A = J M^-1 J^T live in a per-env global scratch (L2), and the narrowphase runs
// wave-uniform in fp64: analytic routines for the pairs MuJoCo has them for, libccd's
// Minkowski Portal Refinement (restated from its published algorithm, as MuJoCo 2.x's mjc_Convex uses it) for everything that
// involves a cylinder or a mesh, with the support mapping of a mesh evaluated by all 64 lanes over its hull vertices.  Everything
// else is fp32.  Checked against oracle/libdm_oracle_g1.so (tests/test_g1_gpu.py) and a bit-for-bit recording
// (tests/test_g1_step_bits_gpu.py).
//
// This file is the translation unit and holds what ties the layers together: the forward evaluation and the monolithic collision
// stage, the step kernels of the two pipelines, the small kernels and the host C ABI.  The layers are headers:
//   dm_g1_device.h      dimensions, layouts, Dev, Lds, Launch
//   dm_g1_math.h        small math, wave reductions
//   dm_g1_dynamics.h    kinematics .. fwd_smooth, integrate_pos
//   dm_g1_narrow.h      broadphase, narrowphase of one pair
//   dm_g1_constraint.h  constraint rows, projection, PGS
//   dm_g1_task.h        step_enter, rk_advance / euler_advance, task_and_finish, step_write_back
#include "dm_g1_device.h"
#include "dm_g1_math.h"
#include "dm_g1_dynamics.h"
#include "dm_g1_narrow.h"
#include "dm_g1_constraint.h"
#include "dm_g1_task.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dm_g1_tables_host.h"   // g1_check_model, g1_build_tables, g1_build_meshes, g1_pack_clip; dm_host.h: DmHost, HIPCHK, DM_DEVICE, DM_LAUNCH

namespace g1 {

// [EXT] mj_collision of the monolithic kernel: the survivors one after the other on this wave
__device__ __noinline__ int collide(const Dev &T, const Launch &P, const int env, const int lane) {
  int overflow = 0;
  int nsurv = broadphase(T, MAXSURV, overflow, lane);
  if (P.skip & SKIP_NARROW) nsurv = 0;
  SYNC();
  PROF(3);
  int ncon = 0, n_pm = 0, n_an = 0, n_mpr = 0;
  const NpStage W = {S.u.co.geo, S.u.co.geoi, reinterpret_cast<Con *>(&S.u.co.rc[0][0]), S.u.co.poly[0], S.u.co.poly[1],
                     reinterpret_cast<Sup *>(&S.u.co.mpr_ps[0][0])};
  const MeshPtrs M = {P.mesh_vert, P.mesh_oidx, P.mesh_clus};
  for (int s = 0; s < nsurv; s++) {
    const int p = S.u.co.surv[s];
    const int g1 = T.p_g1[p], g2 = T.p_g2[p];
    stage_geo(T, W, g1, 0, lane);
    stage_geo(T, W, g2, 1, lane);
    SYNC();
    const int cls = pair_class(W.geoi[0][0], W.geoi[1][0]);
    n_an += cls == 0; n_pm += cls == 1; n_mpr += cls == 2;
    const int n = narrow_pair<false>(M, W, P.sepc + (size_t)env * (4 * SEPC + 4), false, p, P.skip, lane);
    SYNC();
    PROF(cls == 1 ? 5 : (cls == 0 ? 4 : 6));
    for (int k = 0; k < n; k++) {
      if (ncon >= MAXCON) { overflow = 1; continue; }
      if (lane == 0) {
        contact_record(W.rc[k], S.u.co.c_dist[ncon], S.u.co.c_pos[ncon], S.u.co.c_frame[ncon]);
        S.u.co.c_g1[ncon] = g1; S.u.co.c_g2[ncon] = g2;
        S.u.co.c_mu[ncon] = fmaxf(T.g_mu[g1], T.g_mu[g2]);
      }
      ncon++;
    }
    SYNC();
  }
  SYNC();
  if (lane == 0) { S.info[0] = ncon; S.info[4] = overflow; S.info[5] = nsurv; S.info[6] = n_an | (n_pm << 8) | (n_mpr << 16); }
  return ncon;
}

// One forward evaluation = a per-env first half (poses, inertia, factorisation, smooth dynamics), the collision stage, and a
// per-env second half (constraint rows, A, PGS).  The monolithic kernel runs all three on the env's wave; the split pipeline runs
// the halves in g1_env_kernel and the narrowphase of ALL envs' pairs in g1_pair_kernel (one wave per pair).
// EULER: the kernels of the Euler integrator, which keep the unfactored M (park_m) for the step's second factorisation.
template <bool EULER>
__device__ __forceinline__ void forward_pre(const Launch &P, const Dev &T, const int env, const int lane, const bool qlo) {
  PROF(15);
  kinematics(T, lane, qlo);
  com_pos(T, lane);
  PROF(0);
  crb_factor(T, lane);
  if constexpr (EULER) park_m(P, T, env, lane);
  PROF(1);
  fwd_smooth(T, lane);   // before the collision stage: its scratch shares LDS with the contact arrays
  PROF(2);
}
__device__ __noinline__ void project_constraint(const Dev &T, const float *JT, float *BT, float *AR, const float *RW, const int nefc, const int lane) {
  project_constraint_body(T, JT, BT, AR, RW, nefc, lane);
}
__device__ __noinline__ void fwd_constraint(const Dev &T, const float *JT, const float *BT, const float *AR, float *RW, const int nefc, const int lane,
                                             const int max_iter) {
  fwd_constraint_body(T, JT, BT, AR, RW, nefc, lane, max_iter);
}

template <bool INL>   // INL: the two constraint phases inlined (split env kernel) / called out of line (monolithic kernel)
__device__ __forceinline__ void forward_post(const Launch &P, const Dev &T, const int env, const int lane, const int ncon) {
  float *JT = P.jt + (size_t)env * 44 * MAXROW, *BT = P.bt + (size_t)env * 44 * MAXROW, *AR = P.ar + (size_t)env * MAXROW * MAXROW;
  float *RW = P.rows + (size_t)env * 5 * MAXROW;
  int nefc = 0;
  PROF(7);
  if (!(P.skip & SKIP_ROWS)) nefc = make_constraint(T, JT, RW, ncon, lane);
  else { if (lane == 0) { S.info[1] = 0; S.info[2] = 0; } SYNC(); }
  PROF(8);
  if (!(P.skip & SKIP_PROJECT)) { if (INL) project_constraint_body(T, JT, BT, AR, RW, nefc, lane); else project_constraint(T, JT, BT, AR, RW, nefc, lane); }
  PROF(9);
  if (P.skip & SKIP_SOLVE) nefc = 0;
  if (INL) fwd_constraint_body(T, JT, BT, AR, RW, nefc, lane, (P.skip & SKIP_PGS) ? 0 : T.iterations);
  else fwd_constraint(T, JT, BT, AR, RW, nefc, lane, (P.skip & SKIP_PGS) ? 0 : T.iterations);
  PROF(10);
}
template <bool EULER>
__device__ __noinline__ void forward(const Launch &P, const Dev &T, const int env, const int lane, const bool qlo) {
  forward_pre<EULER>(P, T, env, lane, qlo);
  int ncon = 0;
  if (!(P.skip & SKIP_COLLIDE)) ncon = collide(T, P, env, lane);
  else { if (lane == 0) { S.info[0] = 0; S.info[4] = 0; } SYNC(); }
  forward_post<false>(P, T, env, lane, ncon);
}

// The monolithic kernel: one wave runs the whole step (or the single evaluation of the other modes) of its env.  The integrator is a
// template argument and each has its own kernels (g1_step_kernel / g1_step_euler_kernel, g1_env_kernel / g1_env_euler_kernel): the
// RK4 kernels keep the register allocation and scratch they had before the Euler option existed.
template <bool EULER>
__device__ __forceinline__ void step_kernel_body(const Launch &P) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= P.nslots) return;
  const int env = (P.order && P.mode == MODE_STEP) ? P.order[blockIdx.x] : (int)blockIdx.x;
  if ((unsigned)env >= (unsigned)P.N) return;   // a slot without an env (-1 of a padded list): nothing is read or written
  const Dev &T = *P.T;
  const int mode = P.mode;
#ifdef G1_PROFILE
  if (lane == 0) for (int i = 0; i < 16; i++) S.prof[i] = 0;
  S.prof_t = clock64();
#endif
  StepCtx X;
  if (!step_enter(P, T, env, lane, X)) return;
  for (;;) {
    if (!X.sim_err) {
      forward<EULER>(P, T, env, lane, mode == MODE_STEP && !X.after_reset && X.stage > 0);   // the only call site: the evaluation is ~20 k instructions
      X.work += 4000 + S.info[1] * (8 + 6 * S.info[3]) + 3000 * ((S.info[6] >> 16) & 0xFF);   // fixed part, rows x sweeps, MPR pairs
      if (mode == MODE_STEP && !X.after_reset) {
        if (EULER ? euler_advance(P, T, env, lane, X) : rk_advance(P, T, env, lane, X)) continue;
      } else if (mode == MODE_FORCED && !X.after_reset) {
        const bool badv = (lane < NV) && !(fabsf(S.qacc[lane]) <= MAXVALF);
        X.sim_err = __any(badv);
      }
    }
    if (task_and_finish(P, T, env, lane, X)) continue;
    break;
  }
#ifdef G1_PROFILE
  PROF(14);
  SYNC();
  if (P.debug && lane < 16) P.debug[(size_t)env * DMG1_DEBUG_STRIDE + DMG1_DBG_PROF + lane] = (float)S.prof[lane];
#endif
  step_write_back(P, env, lane, X);
}
extern "C" __global__ void __launch_bounds__(64, 2) g1_step_kernel(Launch P) { step_kernel_body<false>(P); }
extern "C" __global__ void __launch_bounds__(64, 2) g1_step_euler_kernel(Launch P) { step_kernel_body<true>(P); }   // MODE_STEP only

// ------------------------------------------------------------------------------------------ split pipeline (MODE_STEP)
// At 4 096 envs the monolithic launch lasts as long as its heaviest env (18 M cycles against a 4.1 M mean, 70 % of it MPR pairs run
// one after the other on that env's wave).  The split pipeline balances the collision stage across the BATCH: per evaluation
//   g1_env_kernel   (one wave per env, longest-first): [second half of the previous evaluation: contacts of the pair kernel ->
//                   constraint rows, A, PGS; RK4 bookkeeping / task layer] then [first half of the next one: poses, inertia,
//                   factorisation, smooth dynamics, broadphase]; the survivors' staged geoms go to the pair queue
//   g1_pair_kernel  (persistent waves pulling tickets, support-query pairs first): narrowphase of ONE pair per ticket, four waves
//                   per SIMD (its own register budget and 1.8 KB of LDS) instead of two
// so an RK4 step is 6 env launches + 5 pair launches (4 RK stages + the evaluation at the reset state of envs that ended) and an
// Euler step (g1_env_euler_kernel) 3 + 2 (the evaluation + the one at the reset state).  Between
// launches an env keeps the non-union head of its LDS working set and its StepCtx in an HBM slot (14.3 KB each way: ~0.12 ms per
// step at 4 096 envs).  Arithmetic and order of operations are those of the monolithic kernel: trajectories are bit-identical
// (tests/test_g1_gpu.py); only the separating-direction cache differs (one entry per (env, pair); result-neutral either way).
constexpr int WS_HEAD = (int)offsetof(Lds, u);
static_assert(WS_HEAD % 16 == 0, "the head of the working set is copied in 16-byte words");
constexpr int WS_CTX_OFF = WS_HEAD, WS_BYTES = ((WS_HEAD + 128 + 255) / 256) * 256;
enum { WC_IDX = 0, WC_EPLEN, WC_RCNT, WC_MOTION, WC_CLIPID, WC_REASON, WC_WORK, WC_STAGE, WC_SNCON, WC_SNEFC, WC_EPREW, WC_REWARD, WC_FLAGS,
       WC_FINISHED = 15 };

__device__ __forceinline__ void ws_save(char *ws, const StepCtx &X, const int lane) {
  SYNC();
  uint4 *dst = reinterpret_cast<uint4 *>(ws);
  const uint4 *src = reinterpret_cast<const uint4 *>(&S);
  for (int i = lane; i < WS_HEAD / 16; i += 64) dst[i] = src[i];
  if (lane == 0) {
    int *w = reinterpret_cast<int *>(ws + WS_CTX_OFF);
    w[WC_IDX] = X.idx_curr; w[WC_EPLEN] = X.ep_len; w[WC_RCNT] = X.rcnt; w[WC_MOTION] = X.motion; w[WC_CLIPID] = X.clip_id;
    w[WC_REASON] = X.reason; w[WC_WORK] = X.work; w[WC_STAGE] = X.stage; w[WC_SNCON] = (int)X.stage_ncon; w[WC_SNEFC] = (int)X.stage_nefc_lo;
    w[WC_EPREW] = __float_as_int(X.ep_rew); w[WC_REWARD] = __float_as_int(X.reward);
    w[WC_FLAGS] = (X.sim_err ? 1 : 0) | (X.done ? 2 : 0) | (X.after_reset ? 4 : 0);
    w[WC_FINISHED] = 0;
  }
}
__device__ __forceinline__ void ws_load(const Launch &P, const char *ws, StepCtx &X, const int lane) {
  const uint4 *src = reinterpret_cast<const uint4 *>(ws);
  uint4 *dst = reinterpret_cast<uint4 *>(&S);
  for (int i = lane; i < WS_HEAD / 16; i += 64) dst[i] = src[i];
  const int *w = reinterpret_cast<const int *>(ws + WS_CTX_OFF);
  X.idx_curr = w[WC_IDX]; X.ep_len = w[WC_EPLEN]; X.rcnt = w[WC_RCNT]; X.motion = w[WC_MOTION]; X.clip_id = w[WC_CLIPID];
  X.reason = w[WC_REASON]; X.work = w[WC_WORK]; X.stage = w[WC_STAGE]; X.stage_ncon = (unsigned)w[WC_SNCON]; X.stage_nefc_lo = (unsigned)w[WC_SNEFC];
  X.ep_rew = __int_as_float(w[WC_EPREW]); X.reward = __int_as_float(w[WC_REWARD]);
  const int fl = w[WC_FLAGS];
  X.sim_err = fl & 1; X.done = (fl >> 1) & 1; X.after_reset = (fl >> 2) & 1;
  X.clip = P.clips[P.task ? (X.motion == 3 ? 2 : X.motion) : X.clip_id];
  SYNC();
}

// broadphase of the evaluation; the survivors (canonical order) go to the env's block of the pair queue: pair ids, staged geoms, and
// one ticket each in the list of their cost class
__device__ __forceinline__ void emit_pairs(const Dev &T, const Launch &P, const int env, const int lane) {
  int overflow = 0;
  const int nsurv = broadphase(T, PAIRCAP, overflow, lane);
  SYNC();
  PROF(3);
  const size_t base = (size_t)env * PAIRCAP;
  int32_t *ctr = P.qctr + 4 * P.round, *tickA = P.tick, *tickB = P.tick + (size_t)P.N * PAIRCAP;
  int n_an = 0, n_pm = 0, n_mpr = 0;
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int b = 0; b < nsurv; b += 64) {
    const int s = b + lane;
    const bool on = s < nsurv;
    int cls = 0;
    if (on) {
      const int p = S.u.co.surv[s];
      cls = pair_class(T.g_type[T.p_g1[p]], T.g_type[T.p_g2[p]]);
      P.pq_pair[base + s] = p;
    }
    const unsigned long long mh = __ballot(on && cls != 0), ml = __ballot(on && cls == 0);
    n_mpr += __popcll(__ballot(on && cls == 2)); n_pm += __popcll(__ballot(on && cls == 1)); n_an += __popcll(ml);
    int bh = 0, bl = 0;
    if (lane == 0) {
      if (mh) bh = atomicAdd(&ctr[0], __popcll(mh));
      if (ml) bl = atomicAdd(&ctr[1], __popcll(ml));
    }
    bh = __builtin_amdgcn_readfirstlane(bh); bl = __builtin_amdgcn_readfirstlane(bl);
    if (on) {
      if (cls != 0) tickA[bh + __popcll(mh & lt)] = (env << 8) | s;
      else tickB[bl + __popcll(ml & lt)] = (env << 8) | s;
    }
  }
  for (int s = 0; s < nsurv; s++) {
    const int p = S.u.co.surv[s];
    const int g = lane < 18 ? T.p_g1[p] : T.p_g2[p];
    if (lane < 36) P.pq_geo[(base + s) * 36 + lane] = geo_entry(T, g, lane < 18 ? lane : lane - 18);
  }
  if (lane == 0) { S.info[4] = overflow; S.info[5] = nsurv; S.info[6] = n_an | (n_pm << 8) | (n_mpr << 16); }
}

// the contacts the pair kernel found, in canonical order (survivor order, then the routine's order), into the contact arrays
__device__ __forceinline__ int gather_contacts(const Dev &T, const Launch &P, const int env, const int lane) {
  const int nsurv = S.info[5];
  int overflow = S.info[4], ncon = 0;
  const size_t base = (size_t)env * PAIRCAP;
  for (int b = 0; b < nsurv; b += 64) {
    const int s = b + lane;
    const bool on = s < nsurv;
    const int n = on ? P.pq_cnt[base + s] : 0;
    int incl = n;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    const int off = ncon + incl - n;
    if (n > 0) {
      const int p = P.pq_pair[base + s];
      const int g1 = T.p_g1[p], g2 = T.p_g2[p];
      const float mu = fmaxf(T.g_mu[g1], T.g_mu[g2]);
      for (int k = 0; k < n; k++) {
        const int c = off + k;
        if (c >= MAXCON) break;
        const float4 *r = reinterpret_cast<const float4 *>(P.pq_con + ((base + s) * 8 + k) * 16);
        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
        S.u.co.c_dist[c] = r0.x;
        S.u.co.c_pos[c][0] = r0.y; S.u.co.c_pos[c][1] = r0.z; S.u.co.c_pos[c][2] = r0.w;
        float *fr = S.u.co.c_frame[c];
        fr[0] = r1.x; fr[1] = r1.y; fr[2] = r1.z; fr[3] = r1.w; fr[4] = r2.x; fr[5] = r2.y; fr[6] = r2.z; fr[7] = r2.w; fr[8] = r3.x;
        S.u.co.c_g1[c] = g1; S.u.co.c_g2[c] = g2; S.u.co.c_mu[c] = mu;
      }
    }
    ncon += __shfl(incl, 63);
  }
  if (ncon > MAXCON) { overflow = 1; ncon = MAXCON; }
  SYNC();
  if (lane == 0) { S.info[0] = ncon; S.info[4] = overflow; }
  SYNC();
  return ncon;
}

template <bool EULER>
__device__ __forceinline__ void env_kernel_body(const Launch &P) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= P.nslots) return;
  const int env = P.order ? P.order[blockIdx.x] : (int)blockIdx.x;
  if ((unsigned)env >= (unsigned)P.N) return;   // a slot without an env, in every round: not even its working-set slot is touched
  const Dev &T = *P.T;
  char *ws = P.ws + (size_t)env * WS_BYTES;
  int *wctx = reinterpret_cast<int *>(ws + WS_CTX_OFF);
  StepCtx X;
#ifdef G1_PROFILE   // per-phase stamps of the split pipeline: accumulated over the rounds in the working set, written out by the last one
#define G1_PROF_OUT() do { SYNC(); if (P.debug && lane < 16) P.debug[(size_t)env * DMG1_DEBUG_STRIDE + DMG1_DBG_PROF + lane] = (float)S.prof[lane]; } while (0)
  if (P.round == 0) { if (lane == 0) for (int i = 0; i < 18; i++) S.prof[i] = 0; S.prof_t = clock64(); }
#else
#define G1_PROF_OUT() do {} while (0)
#endif
  if (P.round == 0) {
    if (!step_enter(P, T, env, lane, X)) { if (lane == 0) wctx[WC_FINISHED] = 1; return; }
    if (X.sim_err) {   // mj_checkPos / mj_checkVel failed: no evaluation, the task layer reports the error (and may reset the env)
      if (!task_and_finish(P, T, env, lane, X)) { step_write_back(P, env, lane, X); if (lane == 0) wctx[WC_FINISHED] = 1; return; }
    }
  } else {
    if (wctx[WC_FINISHED]) return;
    ws_load(P, ws, X, lane);
#ifdef G1_PROFILE
    S.prof_t = clock64();      // (the time between the launches is not this env's)
#endif
    const int ncon = gather_contacts(T, P, env, lane);            // second half of the evaluation in flight
    PROF(13);                  // split pipeline: working-set reload is before the stamp; 13 = gather
    forward_post<true>(P, T, env, lane, ncon);
    // cost of this env in g1_env_kernel (the sort key of the next step's longest-first order): its pairs run in the other kernel, so
    // only the per-evaluation fixed part and rows x sweeps count — a row step costs about twice as much beyond 128 rows (A from L2)
    X.work = (X.work >> 1) + 16000 + S.info[1] * (24 + (S.info[1] > 128 ? 14 : 6) * S.info[3]);   // (later evaluations weigh more: as dm_kernels.hip)
    bool again = false;
    if (!X.after_reset) again = EULER ? euler_advance(P, T, env, lane, X) : rk_advance(P, T, env, lane, X);
    if (!again && !task_and_finish(P, T, env, lane, X)) { PROF(14); G1_PROF_OUT(); step_write_back(P, env, lane, X); if (lane == 0) wctx[WC_FINISHED] = 1; return; }
    PROF(14);
  }
  forward_pre<EULER>(P, T, env, lane, !X.after_reset && X.stage > 0);     // first half of the next evaluation
  emit_pairs(T, P, env, lane);
  PROF(4);                     // split pipeline: 3 = broadphase (inside), 4 = tickets + staged geoms
  ws_save(ws, X, lane);
}
extern "C" __global__ void __launch_bounds__(64, 2) g1_env_kernel(Launch P) { env_kernel_body<false>(P); }
extern "C" __global__ void __launch_bounds__(64, 2) g1_env_euler_kernel(Launch P) { env_kernel_body<true>(P); }

// Narrowphase of the split pipeline: persistent one-wave workgroups pull tickets (support-query pairs first: they cost ~10 x an
// analytic pair) until the queue is empty; one ticket = one (env, pair): its staged geoms in, its contacts out.
// (Pulling the NEXT ticket while this one's narrowphase runs — queue head and ticket word prefetched — was 11 % SLOWER, 486 against
// 436 us per launch: a wave inside a long MPR ticket then sits on a reserved ticket that an idle wave could have taken.  Filing the
// geoms' integer records with the pair to save the table look-ups gained nothing either: those tables are L1 / scalar-cache hits.)
#ifndef G1_PAIR_WAVES
#define G1_PAIR_WAVES 2   // waves per SIMD of the pair kernel (VGPR budget 256: no spills; 168 at 3 spilled 34 and measured 2 % slower)
#endif
extern "C" __global__ void __launch_bounds__(64, G1_PAIR_WAVES) g1_pair_kernel(PairLaunch Q) {
  __shared__ NpLds Wl;
  const int lane = threadIdx.x;
  const Dev &T = *Q.T;
  const NpStage W = {Wl.geo, Wl.geoi, reinterpret_cast<Con *>(&Wl.rc[0][0]), Wl.poly[0], Wl.poly[1], reinterpret_cast<Sup *>(&Wl.mpr_ps[0][0])};
  const MeshPtrs M = {Q.mesh_vert, Q.mesh_oidx, Q.mesh_clus};
  const int nA = Q.qctr[0], nB = Q.qctr[1];      // written by the env launch in front of this one
  for (;;) {   // every wave leaves as soon as the queue is empty
    int t = 0;
    if (lane == 0) t = atomicAdd(&Q.qctr[2], 1);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= nA + nB) break;
    const int tk = t < nA ? Q.tick[t] : Q.tick[(size_t)Q.N * PAIRCAP + (t - nA)];
    const int env = tk >> 8, s = tk & 255;
    const size_t slot = (size_t)env * PAIRCAP + s;
    const int p = Q.pq_pair[slot];
    if (lane < 36) Wl.geo[lane / 18][lane % 18] = Q.pq_geo[slot * 36 + lane];
    if (lane == 0) { stage_geoi(T, W, T.p_g1[p], 0); stage_geoi(T, W, T.p_g2[p], 1); }
    SYNC();
    const int n = narrow_pair<true>(M, W, Q.sepc2 + ((size_t)env * 1024 + p) * 4, true, p, 0, lane);
    SYNC();
    if (lane == 0) Q.pq_cnt[slot] = n;
    if (lane < n) {
      float dist, pos[3], fr[9];
      contact_record(W.rc[lane], dist, pos, fr);
      float4 *o = reinterpret_cast<float4 *>(Q.pq_con + (slot * 8 + lane) * 16);
      o[0] = make_float4(dist, pos[0], pos[1], pos[2]);
      o[1] = make_float4(fr[0], fr[1], fr[2], fr[3]);
      o[2] = make_float4(fr[4], fr[5], fr[6], fr[7]);
      o[3] = make_float4(fr[8], 0.f, 0.f, 0.f);
    }
    SYNC();
  }
}

// Longest-first launch order: env costs vary by an order of magnitude (a robot lying on the floor solves 100 rows for 50
// sweeps, one that was just reset 45 rows for a few), and a batch is only ~2 rounds of resident waves, so the heavy envs must
// start first.  One workgroup: 64 cost buckets (heaviest = bucket 0), histogram, prefix, scatter.  The order inside a
// bucket is arbitrary — results do not depend on the launch order (outputs and RNG are keyed by env).
// `list`: the slot list of dmg1_step_active (only read), or null for all N envs (nslots = N).  The listed envs go by their costs,
// heaviest first, into the engine's own order; slots without an env (an entry outside [0, N)) go last, as -1, in a 65th bucket.
// nslots <= N entries are written.
extern "C" __global__ void __launch_bounds__(1024) g1_schedule_kernel(const int32_t *cost, const int32_t *list, int nslots, int N, int32_t *order) {
  __shared__ int hist[65], base[65], cmax;
  const int t = threadIdx.x;
  if (t < 65) hist[t] = 0;
  if (t == 0) cmax = 1;
  __syncthreads();
  int m = 1;
  for (int i = t; i < nslots; i += 1024) { const int e = list ? list[i] : i; if ((unsigned)e < (unsigned)N) m = max(m, cost[e]); }
  atomicMax(&cmax, m);
  __syncthreads();
  const float sc = 64.f / ((float)cmax + 1.f);
  for (int i = t; i < nslots; i += 1024) {
    const int e = list ? list[i] : i;
    atomicAdd(&hist[(unsigned)e < (unsigned)N ? 63 - min(63, max(0, (int)((float)cost[e] * sc))) : 64], 1);
  }
  __syncthreads();
  if (t == 0) { int a = 0; for (int b = 0; b < 65; b++) { base[b] = a; a += hist[b]; } }
  __syncthreads();
  for (int i = t; i < nslots; i += 1024) {
    const int e = list ? list[i] : i;
    const bool on = (unsigned)e < (unsigned)N;
    order[atomicAdd(&base[on ? 63 - min(63, max(0, (int)((float)cost[e] * sc))) : 64], 1)] = on ? e : -1;
  }
}

extern "C" __global__ void g1_gather_kernel(const float *state, int N, int off, int n, int stride, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * n) return;
  out[i] = state[(size_t)(i / n) * stride + off + i % n];
}
extern "C" __global__ void g1_scatter_int_kernel(float *state, int N, int off, int stride, const int32_t *in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  ((int32_t *)state)[(size_t)i * stride + off] = in[i];
}

}  // namespace g1

// ------------------------------------------------------------------------------------------ host side (C-ABI)
struct DmG1Engine : DmHost {
  DmG1Config cfg;
  int N = 0;
  g1::Dev T;                     // host copy of *dT: dmg1_load_clip packs the clip rows with it
  g1::Dev *dT = nullptr;
  double *dMesh = nullptr, *dClus = nullptr;
  int32_t *dOidx = nullptr;
  float *dState = nullptr, *dJT = nullptr, *dBT = nullptr, *dAR = nullptr, *dRowsE = nullptr, *dSepc = nullptr;
  int integrator = DM_INT_RK4;   // DM_INT_*: DmG1Config.integrator, or the model's under DM_CFG_INT_MODEL
  float *dQM = nullptr;          // Euler only: Launch::qm
  int32_t *dOrder = nullptr, *dCost = nullptr;
  float *dRows[DMG1_MAX_CLIPS] = {}, *dReset[DMG1_MAX_CLIPS] = {}, *dCom[DMG1_MAX_CLIPS] = {}, *dDebug = nullptr;
  int L[DMG1_MAX_CLIPS] = {}, flags[DMG1_MAX_CLIPS] = {};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  bool active_lpt = true;   // dmg1_step_active orders its slot list longest-first (from 512 envs up, as dmg1_step)
  int skip = 0;             // Launch::skip of every launch: g1::SKIP_SEP_CACHE under dmg1_set_null_cache
  // split pipeline (dmg1_step of batches >= 512 envs, or DmG1Config.pipeline = 2)
  bool split = false;
  char *dWs = nullptr;
  double *dPqGeo = nullptr;
  int32_t *dPqPair = nullptr, *dPqCnt = nullptr, *dTick = nullptr, *dQctr = nullptr;
  float *dPqCon = nullptr, *dSepc2 = nullptr;
};

// why the last dmg1_create failed: there is no handle to carry the text, so dmg1_last_error(NULL) returns it
static std::string g1_create_err = "null handle";

extern "C" void dmg1_default_config(DmG1Config *c) {
  memset(c, 0, sizeof *c);
  c->num_envs = 1; c->max_ep_length = 1000; c->vel_obs_scale = 0.1f; c->high_z = 2.0f; c->obs_bound = 100.0f;
  c->seed = 0; c->auto_reset = 1; c->device = 0;
  c->task = 0; c->amnesty_steps = 150; c->to_getup_len = 180;
  c->pipeline = 0;
  c->integrator = DM_CFG_INT_MODEL;   // the XML's (RK4, xml :7)
}
extern "C" size_t dmg1_model_sizeof(void) { return sizeof(DmModelG1); }

// Everything dmg1_create puts on the device.  On failure e->err says why and the caller deletes e, which frees what was made.
static int g1_init(DmG1Engine *e, const DmModelG1 &m) {
  const DmG1Config &cfg = e->cfg;
  if (g1_check_model(m, e->err) != DM_OK) return DM_EINVAL;
  if (cfg.integrator != DM_CFG_INT_MODEL && cfg.integrator != DM_CFG_INT_EULER && cfg.integrator != DM_CFG_INT_RK4)
    return dm_fail(e, DM_EINVAL, "DmG1Config.integrator must be DM_CFG_INT_MODEL, DM_CFG_INT_EULER or DM_CFG_INT_RK4");
  e->integrator = cfg.integrator == DM_CFG_INT_EULER ? DM_INT_EULER : cfg.integrator == DM_CFG_INT_RK4 ? DM_INT_RK4 : m.integrator;
  g1_build_tables(m, e->T);
  std::vector<double> verts, clus;
  std::vector<int32_t> oidx;
  if (g1_build_meshes(m, e->T, verts, oidx, clus) != 0) return dm_fail(e, DM_EINVAL, "a hull has more vertex clusters than 64 * g1::NCH");
  DM_DEVICE(e);
  HIPCHK(e, e->alloc(&e->dT, 1));
  HIPCHK(e, e->upload(e->dT, &e->T, 1));
  HIPCHK(e, e->alloc(&e->dMesh, verts.size()));
  HIPCHK(e, e->upload(e->dMesh, verts.data(), verts.size()));
  HIPCHK(e, e->alloc(&e->dOidx, oidx.size()));
  HIPCHK(e, e->upload(e->dOidx, oidx.data(), oidx.size()));
  HIPCHK(e, e->alloc(&e->dClus, clus.size()));
  HIPCHK(e, e->upload(e->dClus, clus.data(), clus.size()));
  const size_t N = (size_t)e->N;
  std::vector<float> init(N * g1::STATE, 0.f);
  for (size_t i = 0; i < N; i++)
    for (int k = 0; k < g1::NQ; k++) init[i * g1::STATE + g1::S_QPOS + k] = (float)m.qpos0[k];
  HIPCHK(e, e->alloc(&e->dState, init.size()));
  HIPCHK(e, e->upload(e->dState, init.data(), init.size()));
  HIPCHK(e, e->alloc(&e->dJT, N * 44 * g1::MAXROW));
  HIPCHK(e, e->alloc(&e->dBT, N * 44 * g1::MAXROW));
  HIPCHK(e, e->alloc(&e->dAR, N * g1::MAXROW * g1::MAXROW));
  HIPCHK(e, e->alloc(&e->dRowsE, N * 5 * g1::MAXROW));
  HIPCHK(e, e->alloc(&e->dSepc, N * (4 * g1::SEPC + 4)));
  HIPCHK(e, e->fill(e->dSepc, 0xFF, N * (4 * g1::SEPC + 4) * sizeof(float)));   // pair id -1 everywhere
  HIPCHK(e, e->alloc(&e->dOrder, N));
  HIPCHK(e, e->alloc(&e->dCost, N));
  HIPCHK(e, e->fill(e->dCost, 0, N * sizeof(int32_t)));
  if (e->integrator == DM_INT_EULER) HIPCHK(e, e->alloc(&e->dQM, N * g1::QM_STRIDE));
  e->split = cfg.pipeline == 2 || (cfg.pipeline == 0 && e->N >= 512);
#ifdef G1_PROFILE
  if (const char *pl = getenv("DMG1_PIPELINE")) e->split = atoi(pl) == 2;
#endif
  if (e->split) {   // ~135 KB per env: 0.55 GB at 4 096 envs
    const size_t NP = N * g1::PAIRCAP;
    HIPCHK(e, e->alloc(&e->dWs, N * g1::WS_BYTES));
    HIPCHK(e, e->alloc(&e->dPqGeo, NP * 36));
    HIPCHK(e, e->alloc(&e->dPqPair, NP));
    HIPCHK(e, e->alloc(&e->dPqCnt, NP));
    HIPCHK(e, e->alloc(&e->dPqCon, NP * 8 * 16));
    HIPCHK(e, e->alloc(&e->dTick, 2 * NP));
    HIPCHK(e, e->alloc(&e->dQctr, 8 * 4));
    HIPCHK(e, e->alloc(&e->dSepc2, N * 1024 * 4));
    HIPCHK(e, e->fill(e->dSepc2, 0xFF, N * 1024 * 4 * sizeof(float)));   // pair id -1 everywhere
  }
  HIPCHK(e, e->event(&e->ev0));
  HIPCHK(e, e->event(&e->ev1));
  return DM_OK;
}

extern "C" int dmg1_create(const void *model, size_t model_bytes, const DmG1Config *cfg, DmG1Handle *out) {
  if (!model || !cfg || !out || cfg->num_envs < 1) return DM_EINVAL;
  if (model_bytes != sizeof(DmModelG1)) { fprintf(stderr, "dmg1_create: model struct size %zu != %zu\n", model_bytes, sizeof(DmModelG1)); return DM_EINVAL; }
  if (!dm_have_device()) return DM_ENODEV;
  DmG1Engine *e = new DmG1Engine();
  e->cfg = *cfg;
  e->device = cfg->device;
  e->N = cfg->num_envs;
  const int rc = g1_init(e, *(const DmModelG1 *)model);
  if (rc != DM_OK) { g1_create_err = e->err; fprintf(stderr, "dmg1_create: %s\n", e->err.c_str()); delete e; return rc; }
  *out = e;
  return DM_OK;
}

extern "C" int dmg1_destroy(DmG1Handle e) { return dm_destroy_engine(e); }
extern "C" const char *dmg1_last_error(DmG1Handle e) { return e ? e->err.c_str() : g1_create_err.c_str(); }

extern "C" int dmg1_load_clip(DmG1Handle e, int clip_id, int L, const double *q, const double *v, const double *bx, const double *gx, int flags) {
  using namespace g1;
  if (!e || L < 1 || !q || !v || !bx || !gx || clip_id < 0 || clip_id >= DMG1_MAX_CLIPS) return DM_EINVAL;
  DM_DEVICE(e);
  std::vector<float> rows((size_t)L * CLIP_ROW, 0.f), reset((size_t)L * RESET_ROW, 0.f), com((size_t)L * COM_ROW, 0.f);
  g1_pack_clip(e->T, L, q, v, bx, gx, rows.data(), reset.data(), com.data());
  const int c = clip_id;
  e->L[c] = 0;   // an empty slot if the reload fails
  HIPCHK(e, e->reload({{&e->dRows[c], &rows}, {&e->dReset[c], &reset}, {&e->dCom[c], &com}}));
  e->L[c] = L; e->flags[c] = flags;
  return DM_OK;
}

// slots / nslots: the slot list of dmg1_step_active (MODE_STEP only); null = all N envs.  The pipeline (e->split) and every layout
// constant come from the engine's N; nslots sizes the grids only.
static int g1_launch(DmG1Engine *e, g1::Launch &P, void *stream, bool time_it, const int32_t *slots = nullptr, int nslots = 0) {
  P.T = e->dT; P.mesh_vert = e->dMesh; P.mesh_oidx = e->dOidx; P.mesh_clus = e->dClus; P.state = e->dState; P.jt = e->dJT; P.bt = e->dBT; P.ar = e->dAR; P.rows = e->dRowsE; P.sepc = e->dSepc;
  for (int c = 0; c < DMG1_MAX_CLIPS; c++) { P.clips[c].rows = e->dRows[c]; P.clips[c].reset = e->dReset[c]; P.clips[c].com = e->dCom[c]; P.clips[c].L = e->L[c]; P.clips[c].flags = e->flags[c]; }
  P.task = e->cfg.task; P.amnesty_steps = e->cfg.amnesty_steps; P.to_getup_len = e->cfg.to_getup_len;
  const int nl = slots ? nslots : e->N;
  P.N = e->N; P.nslots = nl; P.auto_reset = slots ? 0 : e->cfg.auto_reset; P.max_ep_length = e->cfg.max_ep_length;
  P.vel_obs_scale = e->cfg.vel_obs_scale; P.high_z = e->cfg.high_z; P.obs_bound = e->cfg.obs_bound; P.seed = e->cfg.seed;
  P.debug = e->dDebug;
  P.qm = e->dQM;
  const bool euler = P.mode == g1::MODE_STEP && e->integrator == DM_INT_EULER;   // the other modes run one evaluation and integrate nothing
  if (const char *why = dm_clips_missing(e->L, e->cfg.task != 0, true)) return dm_fail(e, DM_EINVAL, why);
  DM_DEVICE(e);
  bool lpt = true;
  P.skip = e->skip;
#ifdef G1_PROFILE   // phase switches of the diagnostic build only: the shipped library never reads the environment on a launch
  if (const char *sk = getenv("DMG1_SKIP")) P.skip = atoi(sk);   // g1::SKIP_* bits (dm_g1_device.h)
  lpt = !getenv("DMG1_NO_LPT");
#endif
  hipStream_t s = (hipStream_t)stream;
  if (time_it) HIPCHK(e, hipEventRecord(e->ev0, s));
  if (slots) P.order = slots;
  if (P.mode == g1::MODE_STEP && e->N >= 512 && lpt) {   // longest-first order from the previous step's costs
    if (!slots || e->active_lpt) {
      DM_LAUNCH(e, g1::g1_schedule_kernel, dim3(1), dim3(1024), 0, s, e->dCost, slots, nl, e->N, e->dOrder);
      P.order = e->dOrder;
    }
  }
  if (P.mode == g1::MODE_STEP) P.cost = e->dCost;
  if (P.mode == g1::MODE_STEP && e->split) {
    // split pipeline: 6 env launches around 5 pair launches (4 RK stages + the evaluation at the reset state of envs that ended);
    // under Euler 3 around 2.  The counters of the rounds that do not run stay at the zeros of the memset (dmg1_queue_counters).
    P.ws = e->dWs; P.pq_geo = e->dPqGeo; P.pq_pair = e->dPqPair; P.pq_cnt = e->dPqCnt; P.pq_con = e->dPqCon; P.tick = e->dTick;
    P.qctr = e->dQctr; P.sepc2 = e->dSepc2;
    HIPCHK(e, hipMemsetAsync(e->dQctr, 0, 8 * 4 * sizeof(int32_t), s));
    g1::PairLaunch Q;
    memset(&Q, 0, sizeof Q);
    Q.T = e->dT; Q.mesh_vert = e->dMesh; Q.mesh_oidx = e->dOidx; Q.mesh_clus = e->dClus; Q.pq_geo = e->dPqGeo; Q.pq_pair = e->dPqPair;
    Q.pq_cnt = e->dPqCnt; Q.pq_con = e->dPqCon; Q.tick = e->dTick; Q.sepc2 = e->dSepc2; Q.N = e->N;
    const int pair_waves = std::min(nl * 8, 256 * 4 * G1_PAIR_WAVES);   // persistent: every wave pulls tickets until the queue is empty
    const int rounds = euler ? 3 : 6;
    for (int r = 0; r < rounds; r++) {
      P.round = r;
      if (euler) DM_LAUNCH(e, g1::g1_env_euler_kernel, dim3(nl), dim3(64), 0, s, P);
      else DM_LAUNCH(e, g1::g1_env_kernel, dim3(nl), dim3(64), 0, s, P);
      if (r < rounds - 1) {
        Q.qctr = e->dQctr + 4 * r;
        DM_LAUNCH(e, g1::g1_pair_kernel, dim3(pair_waves), dim3(64), 0, s, Q);
      }
    }
  } else if (euler) {
    DM_LAUNCH(e, g1::g1_step_euler_kernel, dim3(nl), dim3(64), 0, s, P);
  } else {
    DM_LAUNCH(e, g1::g1_step_kernel, dim3(nl), dim3(64), 0, s, P);
  }
  if (time_it) { HIPCHK(e, hipEventRecord(e->ev1, s)); e->timed = true; }
  return DM_OK;
}

extern "C" int dmg1_reset(DmG1Handle e, const uint8_t *mask, const int32_t *idx_init, float *obs_out, void *stream) {
  if (!e) return DM_EINVAL;
  g1::Launch P;
  memset(&P, 0, sizeof P);
  P.mode = g1::MODE_RESET; P.mask = mask; P.idx_init = idx_init; P.obs = obs_out;
  return g1_launch(e, P, stream, false);
}
extern "C" int dmg1_step(DmG1Handle e, const float *actions, float *obs, float *rew, uint8_t *done, float *terms, int32_t *reason,
                         float *terminal_obs, void *stream) {
  if (!e || !actions) return DM_EINVAL;
  g1::Launch P;
  memset(&P, 0, sizeof P);
  P.mode = g1::MODE_STEP; P.actions = actions; P.obs = obs; P.rew = rew; P.done = done; P.terms = terms; P.reason = reason;
  P.terminal_obs = terminal_obs;
  return g1_launch(e, P, stream, true);
}
extern "C" int dmg1_step_active(DmG1Handle e, const float *actions, const int32_t *env_ids, int nslots, float *obs, float *rew,
                                uint8_t *done, float *terms, int32_t *reason, void *stream) {
  if (!e) return DM_EINVAL;
  if (!actions || !env_ids || !obs || !rew || !done || nslots < 1 || nslots > e->N) return dm_fail(e, DM_EINVAL, "dmg1_step_active: bad argument");
  g1::Launch P;
  memset(&P, 0, sizeof P);
  P.mode = g1::MODE_STEP; P.actions = actions; P.obs = obs; P.rew = rew; P.done = done; P.terms = terms; P.reason = reason;
  return g1_launch(e, P, stream, true, env_ids, nslots);   // no auto-reset; the pipeline of the whole batch, however few envs are left
}
extern "C" int dmg1_set_active_schedule(DmG1Handle e, int on) {
  if (!e) return DM_EINVAL;
  e->active_lpt = on != 0;
  return DM_OK;
}
extern "C" int dmg1_step_forced(DmG1Handle e, const float *qpos, const float *qvel, float *obs, float *rew, uint8_t *done,
                                float *terms, int32_t *reason, void *stream) {
  if (!e || !qpos || !qvel) return DM_EINVAL;
  g1::Launch P;
  memset(&P, 0, sizeof P);
  P.mode = g1::MODE_FORCED; P.in_qpos = qpos; P.in_qvel = qvel; P.obs = obs; P.rew = rew; P.done = done; P.terms = terms; P.reason = reason;
  return g1_launch(e, P, stream, false);
}
extern "C" int dmg1_set_state(DmG1Handle e, const float *qpos, const float *qvel, const float *warm, int run_forward, void *stream) {
  if (!e || !qpos || !qvel) return DM_EINVAL;
  g1::Launch P;
  memset(&P, 0, sizeof P);
  P.mode = g1::MODE_SETSTATE; P.in_qpos = qpos; P.in_qvel = qvel; P.in_warm = warm; P.run_forward = run_forward;
  return g1_launch(e, P, stream, false);
}
// out = null: nothing to do
static int g1_gather(DmG1Engine *e, int off, int n, float *out, void *stream) {
  if (!out) return DM_OK;
  const int tot = e->N * n;
  DM_DEVICE(e);
  DM_LAUNCH(e, g1::g1_gather_kernel, dim3((tot + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->dState, e->N, off, n, g1::STATE, out);
  return DM_OK;
}
static int g1_scatter(DmG1Engine *e, int off, const int32_t *in, void *stream) {
  if (!in) return DM_OK;
  DM_DEVICE(e);
  DM_LAUNCH(e, g1::g1_scatter_int_kernel, dim3((e->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->dState, e->N, off, g1::STATE, in);
  return DM_OK;
}
extern "C" int dmg1_get_state(DmG1Handle e, float *qpos, float *qvel, float *warm, void *stream) {
  if (!e) return DM_EINVAL;
  int rc = g1_gather(e, g1::S_QPOS, g1::NQ, qpos, stream);
  if (rc == DM_OK) rc = g1_gather(e, g1::S_QVEL, g1::NV, qvel, stream);
  if (rc == DM_OK) rc = g1_gather(e, g1::S_WARM, g1::NV, warm, stream);
  return rc;
}
extern "C" int dmg1_get_counters(DmG1Handle e, int32_t *idx, int32_t *eplen, float *eprew, void *stream) {
  if (!e) return DM_EINVAL;
  int rc = g1_gather(e, g1::S_IDX, 1, (float *)idx, stream);
  if (rc == DM_OK) rc = g1_gather(e, g1::S_EPLEN, 1, (float *)eplen, stream);
  if (rc == DM_OK) rc = g1_gather(e, g1::S_EPREW, 1, eprew, stream);
  return rc;
}
extern "C" int dmg1_set_counters(DmG1Handle e, const int32_t *idx, const int32_t *eplen, void *stream) {
  if (!e) return DM_EINVAL;
  const int rc = g1_scatter(e, g1::S_IDX, idx, stream);
  return rc != DM_OK ? rc : g1_scatter(e, g1::S_EPLEN, eplen, stream);
}
extern "C" int dmg1_queue_counters(DmG1Handle e, int32_t *host_out24) {
  if (!e || !host_out24) return DM_EINVAL;
  memset(host_out24, 0, 24 * sizeof(int32_t));
  if (!e->split) return DM_OK;
  DM_DEVICE(e);
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(host_out24, e->dQctr, 24 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DM_OK;
}
extern "C" int dmg1_set_seed(DmG1Handle e, uint64_t seed) {
  if (!e) return DM_EINVAL;
  e->cfg.seed = seed;
  return DM_OK;
}
extern "C" int dmg1_obs_dim(DmG1Handle e) { return e ? (e->cfg.task ? DMG1_NOBS_COMBINED : DMG1_NOBS) : DM_EINVAL; }
extern "C" int dmg1_get_motion(DmG1Handle e, int32_t *motion, void *stream) {
  if (!e || !motion) return DM_EINVAL;
  return g1_gather(e, g1::S_MOTION, 1, (float *)motion, stream);
}
extern "C" int dmg1_set_motion(DmG1Handle e, const int32_t *motion, void *stream) {
  if (!e || !motion) return DM_EINVAL;
  return g1_scatter(e, g1::S_MOTION, motion, stream);
}
extern "C" int dmg1_set_env_clips(DmG1Handle e, const int32_t *clip_ids, void *stream) { return dmg1_set_motion(e, clip_ids, stream); }
extern "C" int dmg1_get_env_clips(DmG1Handle e, int32_t *clip_ids, void *stream) { return dmg1_get_motion(e, clip_ids, stream); }
extern "C" int dmg1_set_debug(DmG1Handle e, float *debug) {
  if (!e) return DM_EINVAL;
  e->dDebug = debug;
  return DM_OK;
}
extern "C" int dmg1_set_null_cache(DmG1Handle e, int on) {
  if (!e) return DM_EINVAL;
  e->skip = on ? g1::SKIP_SEP_CACHE : 0;
  return DM_OK;
}
extern "C" int dmg1_sep_cache_entries(DmG1Handle e, int32_t *host_out2) {
  if (!e || !host_out2) return DM_EINVAL;
  host_out2[0] = host_out2[1] = 0;
  DM_DEVICE(e);
  HIPCHK(e, hipDeviceSynchronize());
  const size_t per_env = 4 * g1::SEPC + 4;
  std::vector<int32_t> h((size_t)e->N * per_env);
  HIPCHK(e, hipMemcpy(h.data(), e->dSepc, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int env = 0; env < e->N; env++)
    for (int k = 0; k < g1::SEPC; k++) host_out2[0] += h[env * per_env + 4 * k] >= 0;
  if (e->split && e->dSepc2) {
    h.resize((size_t)e->N * 1024 * 4);
    HIPCHK(e, hipMemcpy(h.data(), e->dSepc2, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < (size_t)e->N * 1024; k++) host_out2[1] += h[4 * k] >= 0;
  }
  return DM_OK;
}
static int g1_kernel_ms(DmG1Engine *e, float *ms) {
  DM_DEVICE(e);
  HIPCHK(e, hipEventSynchronize(e->ev1));
  HIPCHK(e, hipEventElapsedTime(ms, e->ev0, e->ev1));
  return DM_OK;
}
extern "C" float dmg1_last_kernel_ms(DmG1Handle e) {
  float ms = -1.f;
  return e && e->timed && g1_kernel_ms(e, &ms) == DM_OK ? ms : -1.f;
}
