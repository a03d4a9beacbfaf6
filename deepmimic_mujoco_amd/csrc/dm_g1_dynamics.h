// dm_g1_dynamics.h — position and velocity stage of one forward evaluation: pose chain, centre of mass, composite inertia and
// L^T D L factorisation, the solves with it, smooth dynamics, the position integrator, and the damped solve of the Euler integrator.
#pragma once
#include "dm_g1_device.h"
#include "dm_g1_math.h"
#include "dm_g1_topology.h"

namespace g1 {

// ------------------------------------------------------------------------------------------ position stage
// [EXT] mj_kinematics.  The pose chain (xpos, xquat) runs in fp64 and is kept as (fp32 value, fp32 remainder): the narrowphase
// is fp64 and takes its geom poses from it (stage_geo); everything else reads the rounded fp32 arrays.  `qlo`: the evaluation
// belongs to RK stage 2..4, whose qpos carries low words (integrate_pos).
__device__ __noinline__ void kinematics(const Dev &T, const int lane, const bool qlo) {
  if (lane == 0) {
    S.xpos[0][0] = S.xpos[0][1] = S.xpos[0][2] = 0;
    S.xquat[0][0] = 1; S.xquat[0][1] = S.xquat[0][2] = S.xquat[0][3] = 0;
    for (int i = 0; i < 3; i++) S.xpos_lo[0][i] = 0;
    for (int i = 0; i < 4; i++) S.xquat_lo[0][i] = 0;
    for (int i = 0; i < 9; i++) S.xmat[0][i] = (i % 4 == 0) ? 1.f : 0.f;
    S.xipos[0][0] = S.xipos[0][1] = S.xipos[0][2] = 0;
  }
  // the body's own joint rotation, all bodies at once (one fp64 sincos per lane, outside the level loop)
  double ql[4] = {1, 0, 0, 0}, rq[4] = {1, 0, 0, 0}, rp[3] = {0, 0, 0};
  if (lane >= 2 && lane < NB) {
    const int k = T.b_dof[lane];   // the body's single hinge; joint anchor = body origin
    const double ang = ((double)S.qpos[k + 1] + (qlo ? (double)S.u.rk.qlo[k + 1] : 0.0)) - T.qpos0_d[k + 1];
    double sn, cs;
    sincos(0.5 * ang, &sn, &cs);
    ql[0] = cs; ql[1] = T.d_axis_d[k][0] * sn; ql[2] = T.d_axis_d[k][1] * sn; ql[3] = T.d_axis_d[k][2] * sn;
  } else if (lane == 1) {   // free root: MuJoCo normalises the stored quaternion in place
    for (int i = 0; i < 4; i++) rq[i] = (double)S.qpos[3 + i] + (qlo ? (double)S.u.rk.qlo[3 + i] : 0.0);
    for (int i = 0; i < 3; i++) rp[i] = (double)S.qpos[i] + (qlo ? (double)S.u.rk.qlo[i] : 0.0);
    dquat_normalize(rq);
  }
  SYNC();
  for (int L = 1; L <= T.maxdepth; L++) {
    if (lane >= 1 && lane < NB && T.b_depth[lane] == L) {
      const int b = lane, p = T.b_parent[b];
      double pos[3], q[4];
      if (b == 1) {
        for (int i = 0; i < 4; i++) {   // x0q_lo: low words of the quaternion the RK stages start from (stage 1 only)
          float hi, l;
          split_hi_lo(rq[i], hi, l);
          q[i] = rq[i]; S.qpos[3 + i] = hi;
          if (!qlo) S.x0q_lo[i] = l;
        }
        for (int i = 0; i < 3; i++) pos[i] = rp[i];
      } else {
        double pq[4], pm[9];
        for (int i = 0; i < 4; i++) pq[i] = (double)S.xquat[p][i] + (double)S.xquat_lo[p][i];
        quat2mat(pm, pq);
        for (int i = 0; i < 3; i++)
          pos[i] = ((double)S.xpos[p][i] + (double)S.xpos_lo[p][i]) +
                   (pm[3 * i] * T.b_pos_d[b][0] + pm[3 * i + 1] * T.b_pos_d[b][1] + pm[3 * i + 2] * T.b_pos_d[b][2]);
        quat_mul(q, pq, T.b_quat_d[b]);
        const int k = T.b_dof[b];
        double qm[9];
        quat2mat(qm, q);
        for (int i = 0; i < 3; i++)
          S.xaxis[k][i] = (float)(qm[3 * i] * T.d_axis_d[k][0] + qm[3 * i + 1] * T.d_axis_d[k][1] + qm[3 * i + 2] * T.d_axis_d[k][2]);
        double qn[4];
        quat_mul(qn, q, ql);
        for (int i = 0; i < 4; i++) q[i] = qn[i];
      }
      dquat_normalize(q);
      double m[9];
      quat2mat(m, q);
      for (int i = 0; i < 3; i++) split_hi_lo(pos[i], S.xpos[b][i], S.xpos_lo[b][i]);
      for (int i = 0; i < 4; i++) split_hi_lo(q[i], S.xquat[b][i], S.xquat_lo[b][i]);
      for (int i = 0; i < 9; i++) S.xmat[b][i] = (float)m[i];
      for (int i = 0; i < 3; i++)
        S.xipos[b][i] = (float)(pos[i] + ((double)T.b_ipos[b][0] * m[3 * i] + (double)T.b_ipos[b][1] * m[3 * i + 1] + (double)T.b_ipos[b][2] * m[3 * i + 2]));
    }
    SYNC();
  }
  for (int g = lane; g < NG; g += 64) {
    const int b = T.g_body[g];
    float gp[3] = {T.g_pos[g][0], T.g_pos[g][1], T.g_pos[g][2]}, t[3];
    mat_vec(t, S.xmat[b], gp);
    for (int i = 0; i < 3; i++) S.gpos[g][i] = S.xpos[b][i] + t[i];
    const int ci = T.g_ci[g];
    if (ci >= 0)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        S.gmat[ci][3 * i + j] = S.xmat[b][3 * i] * T.g_mat[g][j] + S.xmat[b][3 * i + 1] * T.g_mat[g][3 + j] +
                               S.xmat[b][3 * i + 2] * T.g_mat[g][6 + j];
  }
  SYNC();
}

__device__ __noinline__ void com_pos(const Dev &T, const int lane) {   // [EXT] mj_comPos
  float m = (lane >= 1 && lane < NB) ? T.b_mass[lane] : 0.f, c[3];
  for (int i = 0; i < 3; i++) c[i] = wave_sum(m * ((lane < NB) ? S.xipos[lane][i] : 0.f)) * T.total_mass_inv;
  if (lane == 0) for (int i = 0; i < 3; i++) S.com[i] = c[i];
  if (lane < NB) {
    const int b = lane;
    float *ci = S.u.sm.cinert[b];
    if (b == 0) { for (int i = 0; i < 10; i++) ci[i] = 0; }
    else {
      const float *I = T.b_inertia[b], *R = S.xmat[b];
      float Ib[9] = {I[0], I[3], I[4], I[3], I[1], I[5], I[4], I[5], I[2]}, Tm[9], W[9];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Tm[3 * i + j] = R[3 * i] * Ib[j] + R[3 * i + 1] * Ib[3 + j] + R[3 * i + 2] * Ib[6 + j];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W[3 * i + j] = Tm[3 * i] * R[3 * j] + Tm[3 * i + 1] * R[3 * j + 1] + Tm[3 * i + 2] * R[3 * j + 2];
      float o[3] = {S.xipos[b][0] - c[0], S.xipos[b][1] - c[1], S.xipos[b][2] - c[2]}, mass = T.b_mass[b];
      float oo = dot3(o, o);
      ci[0] = W[0] + mass * (oo - o[0] * o[0]); ci[1] = W[4] + mass * (oo - o[1] * o[1]); ci[2] = W[8] + mass * (oo - o[2] * o[2]);
      ci[3] = W[1] - mass * o[0] * o[1]; ci[4] = W[2] - mass * o[0] * o[2]; ci[5] = W[5] - mass * o[1] * o[2];
      ci[6] = mass * o[0]; ci[7] = mass * o[1]; ci[8] = mass * o[2]; ci[9] = mass;
    }
  }
  if (lane < NV) {   // cdof: (angular, linear) about the whole-body COM
    const int k = lane;
    float *cd = S.cdof[k];
    if (k < 3) { for (int i = 0; i < 6; i++) cd[i] = 0; cd[3 + k] = 1; }
    else {
      float ax[3], off[3];
      const int b = T.d_body[k];
      if (k < 6) { ax[0] = S.xmat[1][k - 3]; ax[1] = S.xmat[1][3 + k - 3]; ax[2] = S.xmat[1][6 + k - 3]; }
      else { ax[0] = S.xaxis[k][0]; ax[1] = S.xaxis[k][1]; ax[2] = S.xaxis[k][2]; }
      for (int i = 0; i < 3; i++) off[i] = c[i] - S.xpos[b][i];
      cd[0] = ax[0]; cd[1] = ax[1]; cd[2] = ax[2];
      cross3(cd + 3, ax, off);
    }
  }
  SYNC();
}

// x <- L^-T x for one constraint row held in registers: the dof tree is compile-time (dm_g1_topology.h), so every index is
// static; the factor entries are wave-uniform LDS reads
template <int I, int J, int OFF>
struct RowAnc {
  static __device__ __forceinline__ void run(float (&x)[NV], const float xi, const float *L) {
    if constexpr (J >= 0) {
      x[J] = fmaf(-L[g1topo::MADR[I] + OFF], xi, x[J]);
      RowAnc<I, (J >= 0 ? g1topo::PARENT[J >= 0 ? J : 0] : -1), OFF + 1>::run(x, xi, L);
    }
  }
};
template <int I>
struct RowSolve {
  static __device__ __forceinline__ void run(float (&x)[NV], const float *L) {
    RowAnc<I, g1topo::PARENT[I], 1>::run(x, x[I], L);
    if constexpr (I > 0) RowSolve<I - 1>::run(x, L);
  }
};

// The entries of M (armature included) of the lane's dof, from the composite inertia in S.u.sm.crb: put(index in qM, value)
template <class Put>
__device__ __forceinline__ void m_entries(const Dev &T, const int lane, Put put) {
  if (lane < NV) {
    const int i = lane;
    float buf[6], cd[6];
    for (int q = 0; q < 6; q++) cd[q] = S.cdof[i][q];
    mul_inert_vec(buf, S.u.sm.crb[T.d_body[i]], cd);
    int adr = T.d_madr[i];
    float v = T.d_arm[i];
    for (int q = 0; q < 6; q++) v += cd[q] * buf[q];
    put(adr, v);
    const int n = T.d_nanc[i];
    const uint4 aw = *reinterpret_cast<const uint4 *>(T.d_anc[i]);   // the whole ancestor list in one load (a loop over T.d_anc[i][a]
    const uint32_t awv[4] = {aw.x, aw.y, aw.z, aw.w};                  // waits for one global load per ancestor)
#pragma unroll
    for (int a = 0; a < 14; a++) {
      if (a < n) {
        const int j = (awv[a >> 2] >> (8 * (a & 3))) & 255;
        float s = 0;
        for (int q = 0; q < 6; q++) s += S.cdof[j][q] * buf[q];
        put(adr + 1 + a, s);
      }
    }
  }
}

__device__ __forceinline__ void factor_ldl(const Dev &T, const int lane);

__device__ __noinline__ void crb_factor(const Dev &T, const int lane) {   // [EXT] mj_crb + mj_factorM
  if (lane < NB) {
    float acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t mk = T.b_desc[lane];
    if (lane == 0) mk = 0;
    while (mk) {
      const int d = __ffsll((long long)mk) - 1;
      mk &= mk - 1;
      for (int i = 0; i < 10; i++) acc[i] += S.u.sm.cinert[d][i];
    }
    for (int i = 0; i < 10; i++) S.u.sm.crb[lane][i] = acc[i];
  }
  SYNC();
  m_entries(T, lane, [&](const int i, const float v) { S.qLD[i] = v; });
  SYNC();
  factor_ldl(T, lane);
}

// Euler integrator only: the unfactored M of this evaluation into the env's row of Launch::qm, between crb_factor and fwd_smooth,
// while S.u.sm.crb still holds the composite inertia.  The collision stage overwrites that part of the LDS union, so the second
// factorisation of the step (euler_damped_qacc, after PGS) takes its M from here.
__device__ __noinline__ void park_m(const Launch &P, const Dev &T, const int env, const int lane) {
  float *qm = P.qm + (size_t)env * QM_STRIDE;
  m_entries(T, lane, [&](const int i, const float v) { qm[i] = v; });
}

// In-place elimination of the M entries in S.qLD, and the reciprocals of its diagonal
__device__ __forceinline__ void factor_ldl(const Dev &T, const int lane) {
  // L^T D L, rows of dof k: [k, parent(k), grand-parent, ...]; step k updates the rows of its ancestors.  The dof tree is
  // compile-time (dm_g1_topology.h): per step the only run-time table is the target entry of the lane's ancestor pair, and
  // those (43 steps x up to 105 pairs) are requested in one batch before the first step — a loop over T.d_anc / T.d_madr was
  // three dependent global loads per step.
  uint32_t tgt[NV];
#pragma unroll
  for (int k = 1; k < NV; k++) tgt[k] = T.f_tgt[k][lane];
  const int ta0 = T.tri_a[lane], tb0 = T.tri_b[lane], ta1 = T.tri_a[lane + 64], tb1 = T.tri_b[lane + 64];
  StaticFor<0, NV - 1>::run([&](auto kc) {
    constexpr int k = NV - 1 - decltype(kc)::value;     // NV-1 .. 1
    constexpr int n = g1topo::NANC[k], kk = g1topo::MADR[k], np = n * (n + 1) / 2;
    const float dk = S.qLD[kk];
    if (lane < np) S.qLD[tgt[k] & 0xffff] -= S.qLD[kk + 1 + tb0] * (S.qLD[kk + 1 + ta0] / dk);
    if constexpr (np > 64) {
      if (lane + 64 < np) S.qLD[tgt[k] >> 16] -= S.qLD[kk + 1 + tb1] * (S.qLD[kk + 1 + ta1] / dk);
    }
    SYNC();
    if (lane < n) S.qLD[kk + 1 + lane] = S.qLD[kk + 1 + lane] / dk;
    SYNC();
    return true;
  });
  if (lane < NV) { const float d = S.qLD[T.d_madr[lane]]; S.dinv[lane] = 1.f / d; S.dsq[lane] = 1.f / sqrtf(d); }
  SYNC();
}

// x <- M^-1 x for an LDS vector, M = L^T D L on the compile-time dof tree: lane j keeps x_j in a register.  L^-T: dofs in
// descending order, x_i broadcast (v_readlane, static lane) to its ancestors — the ancestors of a dof are a chain, so the factor
// entry lane j needs is qLD[MADR[i] + NANC[i] - nanc_j] and "is an ancestor" is a compile-time lane mask.  L^-1: dofs in
// ascending order, the final x_j broadcast to its descendants (column-oriented, no reduction).  ~450 instructions with
// two-instruction dependent steps; the tree walk through T.d_nanc / T.d_anc it replaces (a table load, LDS read-modify-writes
// and a wave reduction per dof) took ~100 k cycles per call, eight calls per env-step.  (A static solve with the whole vector in
// 43 registers of every lane, as the constraint rows use, was slower still: +1 ms per launch.)
constexpr uint64_t g1_anc_mask(int i) {
  uint64_t m = 0;
  for (int j = g1topo::PARENT[i]; j >= 0; j = g1topo::PARENT[j]) m |= 1ull << j;
  return m;
}
constexpr uint64_t g1_desc_mask(int j) {
  uint64_t m = 0;
  for (int i = 0; i < g1topo::NV; i++) if ((g1_anc_mask(i) >> j) & 1) m |= 1ull << i;
  return m;
}
__device__ __noinline__ void solve_m(const Dev &T, float *xl, const int lane) {
  const int lk = lane < NV ? lane : 0;
  const int nl = T.d_nanc[lk], ml = T.d_madr[lk] + nl;
  float x = xl[lk];
  StaticFor<0, NV - 1>::run([&](auto ic) {
    constexpr int i = NV - 1 - decltype(ic)::value;            // NV-1 .. 1
    constexpr uint64_t mask = g1_anc_mask(i);
    constexpr int base = g1topo::MADR[i] + g1topo::NANC[i];
    const float xi = rl(x, i);
    if ((mask >> lane) & 1) x = fmaf(-S.qLD[base - nl], xi, x);
    return true;
  });
  x *= S.dinv[lk];
  StaticFor<0, NV - 1>::run([&](auto jc) {
    constexpr int j = decltype(jc)::value;                     // 0 .. NV-2
    constexpr uint64_t mask = g1_desc_mask(j);
    if constexpr (mask != 0) {
      const float xj = rl(x, j);
      if ((mask >> lane) & 1) x = fmaf(-S.qLD[ml - g1topo::NANC[j]], xj, x);
    }
    return true;
  });
  SYNC();
  if (lane < NV) xl[lane] = x;
  SYNC();
}

// ------------------------------------------------------------------------------------------ velocity stage
__device__ __noinline__ void fwd_smooth(const Dev &T, const int lane) {   // mj_comVel, mj_passive, mj_rne, mj_fwdActuation
  if (lane == 0) for (int i = 0; i < 6; i++) { S.cvel[0][i] = 0; S.u.sm.cacc[0][i] = (i == 5) ? -T.gravity[2] : 0.f; }
  SYNC();
  for (int L = 1; L <= T.maxdepth; L++) {
    if (lane >= 1 && lane < NB && T.b_depth[lane] == L) {
      const int b = lane, p = T.b_parent[b];
      float cv[6], ca[6];
      for (int i = 0; i < 6; i++) { cv[i] = S.cvel[p][i]; ca[i] = S.u.sm.cacc[p][i]; }
      if (b == 1) {
        for (int k = 0; k < 3; k++) {
          for (int i = 0; i < 6; i++) S.u.sm.cdofdot[k][i] = 0;
          for (int i = 0; i < 6; i++) cv[i] += S.cdof[k][i] * S.qvel[k];
        }
        for (int k = 3; k < 6; k++) {
          float dd[6], cd[6];
          for (int i = 0; i < 6; i++) cd[i] = S.cdof[k][i];
          cross_motion(dd, cv, cd);
          for (int i = 0; i < 6; i++) { S.u.sm.cdofdot[k][i] = dd[i]; ca[i] += dd[i] * S.qvel[k]; }
        }
        for (int k = 3; k < 6; k++)
          for (int i = 0; i < 6; i++) cv[i] += S.cdof[k][i] * S.qvel[k];
      } else {
        const int k = T.b_dof[b];
        float dd[6], cd[6];
        for (int i = 0; i < 6; i++) cd[i] = S.cdof[k][i];
        cross_motion(dd, cv, cd);
        const float qv = S.qvel[k];
        for (int i = 0; i < 6; i++) { S.u.sm.cdofdot[k][i] = dd[i]; ca[i] += dd[i] * qv; cv[i] += cd[i] * qv; }
      }
      float t[6], t1[6], f[6];
      mul_inert_vec(f, S.u.sm.cinert[b], ca);
      mul_inert_vec(t, S.u.sm.cinert[b], cv);
      cross_force(t1, cv, t);
      for (int i = 0; i < 6; i++) { S.cvel[b][i] = cv[i]; S.u.sm.cacc[b][i] = ca[i]; S.u.sm.cfrc[b][i] = f[i] + t1[i]; }
    }
    SYNC();
  }
  // subtree sums of cfrc into crb[b][0..5] (crb is dead after the factorisation)
  if (lane >= 1 && lane < NB) {
    float acc[6] = {0, 0, 0, 0, 0, 0};
    uint64_t mk = T.b_desc[lane];
    while (mk) {
      const int d = __ffsll((long long)mk) - 1;
      mk &= mk - 1;
      for (int i = 0; i < 6; i++) acc[i] += S.u.sm.cfrc[d][i];
    }
    for (int i = 0; i < 6; i++) S.u.sm.crb[lane][i] = acc[i];
  }
  SYNC();
  if (lane < NV) {
    const int k = lane;
    float bias = 0;
    for (int i = 0; i < 6; i++) bias += S.cdof[k][i] * S.u.sm.crb[T.d_body[k]][i];
    const float passive = -T.d_damp[k] * S.qvel[k];
    float act = 0;
    const int a = T.d_act[k];
    if (a >= 0) act = fminf(fmaxf(S.ctrl[a], T.d_clo[k]), T.d_chi[k]);   // gear 1
    const float fs = passive - bias + act;
    S.bias[k] = bias; S.fsm[k] = fs; S.qas[k] = fs;
  }
  SYNC();
  solve_m(T, S.qas, lane);
  SYNC();
}

// [EXT] mj_integratePos from the step's start state x0q (+ the low words of its normalised root quaternion), in fp64.  `lo`: keep
// the low words of the result for the next evaluation's pose chain (RK stages 2..4); the step's final state is the rounded value.
__device__ void integrate_pos(const Dev &T, const float *vel, const double a, const bool lo, const int lane) {
  const double h = a * T.timestep_d;
  if (lane == 0) {
    for (int i = 0; i < 3; i++) {
      float hi, l;
      split_hi_lo((double)S.x0q[i] + h * (double)vel[i], hi, l);
      S.qpos[i] = hi;
      if (lo) S.u.rk.qlo[i] = l;
    }
    double w[3] = {(double)vel[3], (double)vel[4], (double)vel[5]};
    double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (n < MINVAL) { w[0] = 1; w[1] = w[2] = 0; n = 0; } else { w[0] /= n; w[1] /= n; w[2] /= n; }
    const double ang = h * n;
    double sn, cs;
    sincos(0.5 * ang, &sn, &cs);
    double qr[4] = {cs, w[0] * sn, w[1] * sn, w[2] * sn}, qo[4], qn[4];
    for (int i = 0; i < 4; i++) qo[i] = (double)S.x0q[3 + i] + (double)S.x0q_lo[i];
    dquat_normalize(qo);
    quat_mul(qn, qo, qr);
    dquat_normalize(qn);
    for (int i = 0; i < 4; i++) {
      float hi, l;
      split_hi_lo(qn[i], hi, l);
      S.qpos[3 + i] = hi;
      if (lo) S.u.rk.qlo[3 + i] = l;
    }
  }
  if (lane >= 6 && lane < NV) {
    float hi, l;
    split_hi_lo((double)S.x0q[lane + 1] + h * (double)vel[lane], hi, l);
    S.qpos[lane + 1] = hi;
    if (lo) S.u.rk.qlo[lane + 1] = l;
  }
}

// [EXT] mj_Euler's implicit joint damping, after the evaluation: S.tmp <- qacc' with (M + h B) qacc' = qfrc_smooth + qfrc_constraint,
// B = diag(damping), computed as qacc' = qacc - (M + h B)^-1 h B qacc (the correction is small against qacc: fp32 keeps more of it
// than a solve of the summed forces would).  M: the entries park_m kept; the factor in S.qLD, S.dinv, S.dsq is that of M + h B
// afterwards — nothing reads them before the next evaluation's crb_factor.  S.qacc is left as the evaluation wrote it.
__device__ __noinline__ void euler_damped_qacc(const Dev &T, const float *qm, const int lane) {
  for (int i = lane; i < NM; i += 64) S.qLD[i] = qm[i];
  float hb = 0;
  if (lane < NV) { hb = T.timestep * T.d_damp[lane]; S.tmp[lane] = hb * S.qacc[lane]; }
  SYNC();
  if (lane < NV) S.qLD[T.d_madr[lane]] += hb;
  SYNC();
  factor_ldl(T, lane);
  solve_m(T, S.tmp, lane);
  if (lane < NV) S.tmp[lane] = S.qacc[lane] - S.tmp[lane];
  SYNC();
}

}  // namespace g1
