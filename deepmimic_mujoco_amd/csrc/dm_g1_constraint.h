// dm_g1_constraint.h — constraint stage: rows and Jacobian, A = J M^-1 J^T through the factor, PGS.
#pragma once
#include "dm_g1_device.h"
#include "dm_g1_math.h"
#include "dm_g1_dynamics.h"

namespace g1 {

// ------------------------------------------------------------------------------------------ constraints
__device__ __forceinline__ float impedance(const float *solimp, float pos, float margin) {   // [EXT] getimpedance
  const float dmin = solimp[0], dmax = solimp[1], width = solimp[2], mid = solimp[3], power = solimp[4];
  if (dmin == dmax || width <= MINVALF) return 0.5f * (dmin + dmax);
  const float x = fabsf(pos - margin) / width;
  if (x >= 1) return dmax;
  if (x <= 0) return dmin;
  float y;
  if (power == 1) y = x;
  else if (x <= mid) y = powf(x, power) / powf(mid, power - 1);
  else y = 1 - powf(1 - x, power) / powf(1 - mid, power - 1);
  return dmin + y * (dmax - dmin);
}

// rows -> J^T (global, dof-major), R, aref; returns nefc.  Order: friction loss (dof order), limits (joint order), contacts.
__device__ __noinline__ int make_constraint(const Dev &T, float *JT, float *RW, const int ncon, const int lane) {
  float *e_R = RW, *e_b = RW + MAXROW, *e_f = RW + 2 * MAXROW, *e_lim = RW + 3 * MAXROW;
  int32_t *e_meta = (int32_t *)(RW + 4 * MAXROW);
  // friction-loss rows: dofs 6..42 -> rows 0..36
  int nefc = 0;
  for (int k = 6; k < NV; k++) {   // (all hinges of this model carry friction loss; the table says which)
    if (T.d_floss[k] > 0) nefc++;
  }
  const int nfric = nefc;
  if (lane < NV - 6) {
    const int k = 6 + lane;
    // row index = number of friction dofs before k
    int r = 0;
    for (int q = 6; q < k; q++) r += T.d_floss[q] > 0;
    if (T.d_floss[k] > 0) {
      e_meta[r] = ROW_FRICTION | (k << 2);
      e_lim[r] = T.d_floss[k];
      const float imp = impedance(T.solimp, 0.f, 0.f);
      e_R[r] = fmaxf(MINVALF, (1 - imp) * T.d_invw[k] / imp);
      e_b[r] = -T.B * S.qvel[k];   // aref (K = 0 for friction rows)
    }
  }
  // joint limits
  bool lo = false, hi = false;
  float dlo = 0, dhi = 0;
  if (lane < NV - 6) {
    const int k = 6 + lane;
    const float q = S.qpos[k + 1];
    dlo = q - T.d_lo[k]; dhi = T.d_hi[k] - q;
    lo = dlo < 0; hi = dhi < 0;
  }
  {
    const unsigned long long mlo = __ballot(lo), mhi = __ballot(hi);
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int before = __popcll(mlo & lt) + __popcll(mhi & lt);
    if (lo || hi) {
      const int k = 6 + lane;
      int r = nefc + before;
      for (int side = 0; side < 2; side++) {
        if (!(side ? hi : lo)) continue;
        if (r < MAXROW) {
          const float dist = side ? dhi : dlo;
          e_meta[r] = ROW_LIMIT | (k << 2) | (side << 12);
          e_lim[r] = 0;
          const float imp = impedance(T.solimp, dist, 0.f);
          e_R[r] = fmaxf(MINVALF, (1 - imp) * T.d_invw[k] / imp);
          const float jv = side ? -1.f : 1.f;
          e_b[r] = -T.B * (jv * S.qvel[k]) - T.K * imp * dist;
        }
        r++;
      }
    }
    nefc += __popcll(mlo) + __popcll(mhi);
  }
  const int nlimit = nefc - nfric;
  // contacts: 4 pyramid rows each
  const int row0 = nefc;
  int kept = ncon;
  if (row0 + 4 * ncon > MAXROW) kept = (MAXROW - row0) / 4;
  nefc = row0 + 4 * kept;
  SYNC();
  // zero J^T for all rows, then fill
  for (int k = 0; k < NV; k++)
    for (int r = lane; r < nefc; r += 64) JT[k * MAXROW + r] = 0.f;
  SYNC();
  for (int r = lane; r < row0; r += 64) {
    const int meta = e_meta[r], k = (meta >> 2) & 0x3FF, type = meta & 3;
    JT[k * MAXROW + r] = (type == ROW_FRICTION) ? 1.f : (((meta >> 12) & 1) ? -1.f : 1.f);
  }
  for (int c = 0; c < kept; c++) {
    const int b1 = T.g_body[S.u.co.c_g1[c]], b2 = T.g_body[S.u.co.c_g2[c]];
    const float mu = S.u.co.c_mu[c];
    const int r0 = row0 + 4 * c;
    if (lane < NV) {
      const int k = lane;
      const bool in1 = (T.b_chain[b1] >> k) & 1, in2 = (T.b_chain[b2] >> k) & 1;
      float j[3] = {0, 0, 0};
      if (in1 != in2) {
        float off[3] = {S.u.co.c_pos[c][0] - S.com[0], S.u.co.c_pos[c][1] - S.com[1], S.u.co.c_pos[c][2] - S.com[2]}, t[3];
        cross3(t, S.cdof[k], off);
        for (int i = 0; i < 3; i++) j[i] = (in2 ? 1.f : -1.f) * (S.cdof[k][3 + i] + t[i]);
      }
      const float *fr = S.u.co.c_frame[c];
      const float j0 = fr[0] * j[0] + fr[1] * j[1] + fr[2] * j[2], j1 = fr[3] * j[0] + fr[4] * j[1] + fr[5] * j[2],
                  j2 = fr[6] * j[0] + fr[7] * j[1] + fr[8] * j[2];
      JT[k * MAXROW + r0] = j0 + mu * j1; JT[k * MAXROW + r0 + 1] = j0 - mu * j1;
      JT[k * MAXROW + r0 + 2] = j0 + mu * j2; JT[k * MAXROW + r0 + 3] = j0 - mu * j2;
    }
    if (lane == 0) {
      const float tran = T.b_invw[b1] + T.b_invw[b2], diag = tran + mu * mu * tran;
      const float imp = impedance(T.solimp, S.u.co.c_dist[c], 0.f);
      const float R0 = fmaxf(MINVALF, (1 - imp) * diag / imp), Rpy = 2.f * mu * mu * R0;
      for (int e = 0; e < 4; e++) {
        e_meta[r0 + e] = ROW_CONTACT | (c << 2);
        e_lim[r0 + e] = 0;
        e_R[r0 + e] = Rpy;
        e_f[r0 + e] = imp;   // parked: aref needs the row velocity, computed below
      }
    }
  }
  SYNC();
  // contact rows: vel = J qvel, aref = -B vel - K imp dist
  for (int r = row0 + lane; r < nefc; r += 64) {
    float vel = 0;
    for (int k = 0; k < NV; k++) vel += JT[k * MAXROW + r] * S.qvel[k];
    const int c = (e_meta[r] >> 2);
    e_b[r] = -T.B * vel - T.K * e_f[r] * S.u.co.c_dist[c];
  }
  if (lane == 0) { S.info[1] = nefc; S.info[2] = nlimit; if (kept < ncon) S.info[4] = 1; }
  SYNC();
  return nefc;
}


// A = J M^-1 J^T + R into the per-env scratch.  Up to 128 rows: lane r (and r + 64) keeps its row of B = D^-1/2 L^-T J^T in
// 43 registers (solved with static indices), and A[i][:] is 43 broadcasts of row i (v_readlane: scalar operands) times the
// lanes' own rows — no memory traffic except J in and A out.  More rows: the general path through the B^T scratch.
// (body shared by the out-of-line copy the monolithic kernel calls and the split env kernel, which inlines it: as a callee it
// saves and restores 112 VGPRs per call through scratch — 28 KB per env and evaluation, most of g1_env_kernel's HBM writes)
__device__ __forceinline__ void project_constraint_body(const Dev &T, const float *JT, float *BT, float *AR, const float *RW,
                                                const int nefc, const int lane) {
  const float *e_R = RW;
  if (nefc <= MAXROW) {
    // rows in chunks of 64 (up to four): the lanes' rows of B in 43 registers each; A[i][j] for i in the same chunk by
    // broadcasts of row i, for i in an EARLIER chunk from the rows that chunk stored in the B^T scratch (wave-uniform loads),
    // written both ways
    const int nchunk = (nefc + 63) >> 6;
    for (int cj = 0; cj < nchunk; cj++) {
      const int j = lane + 64 * cj;
      const bool on = j < nefc;
      float x[NV];
#pragma unroll
      for (int k = 0; k < NV; k++) x[k] = on ? JT[k * MAXROW + j] : 0.f;
      RowSolve<NV - 1>::run(x, S.qLD);
#pragma unroll
      for (int k = 0; k < NV; k++) x[k] *= S.dsq[k];
      if (nchunk > 1) {
#pragma unroll
        for (int k = 0; k < NV; k++) if (on) BT[k * MAXROW + j] = x[k];
        SYNC();
      }
      // A is stored SCALED for the PGS sweep: entry (i, j) x -1 / A_jj, the factor of the lane that owns column j (the sweep
      // carries g_j = -r_j / A_jj); the diagonal itself goes to the spare row 43 of the B^T scratch
      const float rj = on ? e_R[j] : 0.f;
      float ajj = rj;
#pragma unroll
      for (int k = 0; k < NV; k++) ajj = fmaf(x[k], x[k], ajj);
      const float nj = on ? -1.f / ajj : 0.f;
      if (on) BT[NV * MAXROW + j] = ajj;
      if (nchunk > 1) SYNC();
      // rows of the same chunk: the 64 x 64 block B B^T on the matrix pipe — four 32 x 32 sub-blocks of v_mfma_f32_32x32x2f32
      // over 22 k pairs.  The instruction wants lane (r, h) to supply B[row r][k0 + h]: one v_permlane32_swap of (x[k0], x[k0 + 1])
      // yields the operand of rows 0..31 (lower half keeps x[k0], upper half receives the lower half's x[k0 + 1]) AND that of rows
      // 32..63 (the other result).  88 MFMAs + 22 swaps instead of 64 x (43 v_readlane + 43 FMA).
      {
        typedef float f16v __attribute__((ext_vector_type(16)));
        f16v acc00, acc01, acc10, acc11;
#pragma unroll
        for (int v = 0; v < 16; v++) acc00[v] = acc01[v] = acc10[v] = acc11[v] = 0.f;
        StaticFor<0, (NV + 1) / 2>::run([&](auto kc) {
          constexpr int k0 = decltype(kc)::value * 2;
          const float xa = x[k0], xb = (k0 + 1 < NV) ? x[k0 + 1 < NV ? k0 + 1 : 0] : 0.f;
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(xa), __float_as_uint(xb), false, false);
          const float op0 = __uint_as_float(sw[0]), op1 = __uint_as_float(sw[1]);
          acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(op0, op0, acc00, 0, 0, 0);
          acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(op0, op1, acc01, 0, 0, 0);
          acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(op1, op0, acc10, 0, 0, 0);
          acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(op1, op1, acc11, 0, 0, 0);
          return true;
        });
        // result fragment: lane (c, h) holds D[row = 8 (v / 4) + 4 h + v % 4][col = c] of its sub-block; column j's scale
        // -1 / A_jj lives in lane j: both halves fetched with one swap
        const auto nsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(nj), __float_as_uint(nj), false, false);
        const float n0 = __uint_as_float(nsw[0]), n1 = __uint_as_float(nsw[1]);   // of columns c and 32 + c
        const int c = lane & 31, h = lane >> 5, base = 64 * cj;
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const int r = 8 * (v / 4) + 4 * h + (v % 4);
#pragma unroll
          for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int jb = 0; jb < 2; jb++) {
              const int i = base + 32 * ib + r, jj = base + 32 * jb + c;
              const float val = ib == 0 ? (jb == 0 ? acc00[v] : acc01[v]) : (jb == 0 ? acc10[v] : acc11[v]);
              if (i < nefc && jj < nefc) AR[i * MAXROW + jj] = (i == jj) ? -1.f : val * (jb == 0 ? n0 : n1);
            }
        }
      }
      // cross blocks: an earlier chunk's rows (operand fragments loaded straight from the B^T scratch in the layout the
      // instruction wants) against this chunk's, on the matrix pipe as well; pass 0 gives the block A[ci][cj], pass 1 its
      // transpose A[cj][ci] with the operands exchanged, so both are stored with coalesced rows
      for (int ci = 0; ci < cj; ci++) {
        typedef float f16v __attribute__((ext_vector_type(16)));
        const int c = lane & 31, h = lane >> 5;
        const auto nsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(nj), __float_as_uint(nj), false, false);
        const float ncj[2] = {__uint_as_float(nsw[0]), __uint_as_float(nsw[1])};          // columns of this chunk
        const float nci[2] = {-1.f / BT[NV * MAXROW + 64 * ci + c], -1.f / BT[NV * MAXROW + 64 * ci + 32 + c]};   // of chunk ci (full)
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
          f16v d00, d01, d10, d11;
#pragma unroll
          for (int v = 0; v < 16; v++) d00[v] = d01[v] = d10[v] = d11[v] = 0.f;
          StaticFor<0, (NV + 1) / 2>::run([&](auto kc) {
            constexpr int k0 = decltype(kc)::value * 2;
            const float xa = x[k0], xb = (k0 + 1 < NV) ? x[k0 + 1 < NV ? k0 + 1 : 0] : 0.f;
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(xa), __float_as_uint(xb), false, false);
            const float oj0 = __uint_as_float(sw[0]), oj1 = __uint_as_float(sw[1]);
            const bool kv = k0 + h < NV;
            const float oi0 = kv ? BT[(k0 + h) * MAXROW + 64 * ci + c] : 0.f, oi1 = kv ? BT[(k0 + h) * MAXROW + 64 * ci + 32 + c] : 0.f;
            if (pass == 0) {
              d00 = __builtin_amdgcn_mfma_f32_32x32x2f32(oi0, oj0, d00, 0, 0, 0);
              d01 = __builtin_amdgcn_mfma_f32_32x32x2f32(oi0, oj1, d01, 0, 0, 0);
              d10 = __builtin_amdgcn_mfma_f32_32x32x2f32(oi1, oj0, d10, 0, 0, 0);
              d11 = __builtin_amdgcn_mfma_f32_32x32x2f32(oi1, oj1, d11, 0, 0, 0);
            } else {
              d00 = __builtin_amdgcn_mfma_f32_32x32x2f32(oj0, oi0, d00, 0, 0, 0);
              d01 = __builtin_amdgcn_mfma_f32_32x32x2f32(oj0, oi1, d01, 0, 0, 0);
              d10 = __builtin_amdgcn_mfma_f32_32x32x2f32(oj1, oi0, d10, 0, 0, 0);
              d11 = __builtin_amdgcn_mfma_f32_32x32x2f32(oj1, oi1, d11, 0, 0, 0);
            }
            return true;
          });
          const int rbase = 64 * (pass == 0 ? ci : cj), cbase = 64 * (pass == 0 ? cj : ci);
#pragma unroll
          for (int v = 0; v < 16; v++) {
            const int r = 8 * (v / 4) + 4 * h + (v % 4);
#pragma unroll
            for (int a2 = 0; a2 < 2; a2++)
#pragma unroll
              for (int b2 = 0; b2 < 2; b2++) {
                const int i = rbase + 32 * a2 + r, jj = cbase + 32 * b2 + c;
                const float val = a2 == 0 ? (b2 == 0 ? d00[v] : d01[v]) : (b2 == 0 ? d10[v] : d11[v]);
                if (i < nefc && jj < nefc) AR[i * MAXROW + jj] = val * (pass == 0 ? ncj[b2] : nci[b2]);
              }
          }
        }
      }
    }
    SYNC();
    return;
  }
}

// [EXT] mj_fwdConstraint + mj_solPGS: dual PGS, rows unilateral (limits, pyramid edges) or boxed (friction loss)
__device__ __forceinline__ void fwd_constraint_body(const Dev &T, const float *JT, const float *BT, const float *AR, float *RW, const int nefc, const int lane,
                                             const int max_iter) {
  float *e_R = RW, *e_b = RW + MAXROW, *e_f = RW + 2 * MAXROW, *e_lim = RW + 3 * MAXROW;
  const int32_t *e_meta = (const int32_t *)(RW + 4 * MAXROW);
  if (nefc == 0) {
    if (lane < NV) { S.qacc[lane] = S.qas[lane]; S.warm[lane] = S.qas[lane]; S.qfc[lane] = 0; }
    if (lane == 0) S.info[3] = 0;
    SYNC();
    return;
  }
  // b = J qacc_smooth - aref; warm-start forces from J qacc_warmstart - aref
  for (int r = lane; r < nefc; r += 64) {
    float s = 0, w = 0;
    for (int k = 0; k < NV; k++) { const float j = JT[k * MAXROW + r]; s += j * S.qas[k]; w += j * S.warm[k]; }
    const float aref = e_b[r], jar = w - aref, D = 1.f / e_R[r];
    float f;
    if ((e_meta[r] & 3) == ROW_FRICTION) {
      const float fl = e_lim[r], rf = e_R[r] * fl;
      f = jar <= -rf ? fl : (jar >= rf ? -fl : -D * jar);
    } else f = jar < 0 ? -D * jar : 0.f;
    e_b[r] = s - aref;
    e_f[r] = f;
  }
  SYNC();
  const int nr = (nefc + 63) >> 6;   // rows per lane (<= 4)
  float res[4] = {0, 0, 0, 0}, fr[4] = {0, 0, 0, 0}, diag[4] = {1, 1, 1, 1};
  float cost = 0;
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const int r = lane + 64 * m;
    if (m < nr && r < nefc) {
      float s = 0;
      for (int c0 = 0; c0 < nefc; c0 += 8) {             // eight column loads in flight (a plain loop waits for each)
        float a[8], fc[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const bool ok = c0 + q < nefc;
          a[q] = ok ? AR[(c0 + q) * MAXROW + r] : 0.f;
          fc[q] = ok ? e_f[c0 + q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; q++) s = fmaf(a[q], fc[q], s);
      }
      diag[m] = BT[NV * MAXROW + r];
      s *= -diag[m];                                     // A is stored x -1 / A_rr (project_constraint)
      fr[m] = e_f[r];
      cost += fr[m] * (0.5f * s + e_b[r]);
      res[m] = e_b[r] + s;
    }
  }
  cost = wave_sum(cost);
  if (cost > 0) {
#pragma unroll
    for (int m = 0; m < 4; m++) { const int r = lane + 64 * m; if (m < nr && r < nefc) { fr[m] = 0; res[m] = e_b[r]; } }
  }
  // the rows' type / bound live in registers of the owning lane; A rows are fetched sixteen sweep-steps ahead (the
  // per-env A scratch is L2-resident: one exposed round trip per block of rows instead of one per row)
  float lm[4] = {-1, -1, -1, -1}, dinv[4] = {1, 1, 1, 1};   // friction-loss bound (< 0: unilateral row), 1 / A_ii
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const int r = lane + 64 * m;
    if (m < nr && r < nefc) { lm[m] = ((e_meta[r] & 3) == ROW_FRICTION) ? e_lim[r] : -1.f; dinv[m] = 1.f / diag[m]; }
  }
  PROF(11);
  constexpr int PF = 16;
  int iter = 0;
  if (nefc <= 64) {
    // up to 64 rows (nine evaluations in ten): lane j keeps its row of A in 64 registers, the sweep is unrolled over the rows
    // with static lanes and static register indices — no memory and no dynamic lane select in the sweep's dependent chain
    float arow[64];
#pragma unroll
    for (int i = 0; i < 64; i++) arow[i] = (i < nefc && lane < nefc) ? AR[i * MAXROW + lane] : 0.f;
    // Lane j's force changes only at step j of a sweep, so a sweep carries the residual alone, scaled: g = -r / A_jj with the
    // lane's row of A pre-multiplied by -1 / A_jj.  The change its row WOULD take is then med3(g, lo - f, hi - f) (unilateral
    // rows: lo = 0, hi = inf; friction-loss rows: -+ the bound), the two bounds constant within the sweep.  A step is
    // v_med3, v_readlane, fma (+ the owner recording the g it saw): one broadcast instead of five, a three-instruction
    // dependent chain.  Forces and the cost decrease (mj_solPGS "improvement") are committed once per sweep.
    float f0 = fr[0];
    const float aii0 = diag[0], fl0 = lm[0], nainv0 = -dinv[0];
    const float lo0 = fl0 >= 0.f ? -fl0 : 0.f, hi0 = fl0 >= 0.f ? fl0 : __builtin_inff();
    float g0 = res[0] * nainv0;
    while (iter < max_iter) {
      const float nlo = lo0 - f0, nhi = hi0 - f0;
      float seen = g0;
      int lane_s = lane;
      asm volatile("" : "+v"(lane_s));   // keeps the per-row lane compares inside the sweep (else 64 SGPR pairs of masks spill)
      StaticFor<0, 64>::run([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if (i >= nefc) return false;
        const float dl_ = rl(__builtin_amdgcn_fmed3f(g0, nlo, nhi), i);
        seen = (lane_s == i) ? g0 : seen;
        asm volatile("" : "+v"(seen));   // select NOW: left alone the compiler keeps all 64 intermediate g alive and spills A
        g0 = fmaf(arow[i], dl_, g0);
        return true;
      });
      const float dl0 = __builtin_amdgcn_fmed3f(seen, nlo, nhi);
      const float improvement = -wave_sum(lane < nefc ? dl0 * aii0 * (0.5f * dl0 - seen) : 0.f);   // dl (dl A_ii / 2 + r), r = -g A_ii
      f0 = (dl0 == nlo) ? lo0 : ((dl0 == nhi) ? hi0 : f0 + dl0);                                 // exactly on the bound when clamped
      iter++;
      if (improvement * T.pgs_scale < T.tolerance) break;
    }
    fr[0] = f0;
  } else if (nefc <= 128) {
    // 65..128 rows (bodies on the floor — the envs that set the launch time): rows j and j + 64 per lane; the first 64 sweep
    // steps run as above on two register rows of A (columns 0..63), the steps for rows 64.. take their A rows from the
    // scratch, prefetched a block ahead
    float ar0[64], ar1[64];
#pragma unroll
    for (int i = 0; i < 64; i++) { ar0[i] = AR[i * MAXROW + lane]; ar1[i] = (lane + 64 < nefc) ? AR[i * MAXROW + lane + 64] : 0.f; }
    float f0 = fr[0], f1 = fr[1];
    const float aii0 = diag[0], fl0 = lm[0], aii1 = diag[1], fl1 = lm[1], nainv0 = -dinv[0], nainv1 = -dinv[1];
    const float lo0 = fl0 >= 0.f ? -fl0 : 0.f, hi0 = fl0 >= 0.f ? fl0 : __builtin_inff();
    const float lo1 = fl1 >= 0.f ? -fl1 : 0.f, hi1 = fl1 >= 0.f ? fl1 : __builtin_inff();
    float g0 = res[0] * nainv0, g1 = res[1] * nainv1;
    const bool has1 = lane + 64 < nefc;
    while (iter < max_iter) {
      const float nlo0 = lo0 - f0, nhi0 = hi0 - f0, nlo1 = lo1 - f1, nhi1 = hi1 - f1;
      float seen0 = g0, seen1 = g1;
      int lane_s = lane;
      asm volatile("" : "+v"(lane_s));
      StaticFor<0, 64>::run([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float dl_ = rl(__builtin_amdgcn_fmed3f(g0, nlo0, nhi0), i);
        seen0 = (lane_s == i) ? g0 : seen0;
        asm volatile("" : "+v"(seen0));
        g0 = fmaf(ar0[i], dl_, g0);
        g1 = fmaf(ar1[i], dl_, g1);
        return true;
      });
      for (int i0 = 64; i0 < nefc; i0 += PF) {
        float a0[PF], a1[PF];
#pragma unroll
        for (int q = 0; q < PF; q++) {
          const int i = i0 + q;
          a0[q] = (i < nefc) ? AR[i * MAXROW + lane] : 0.f;
          a1[q] = (i < nefc && has1) ? AR[i * MAXROW + lane + 64] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < PF; q++) {
          const int src = i0 + q - 64;
          if (i0 + q < nefc) {
            const float dl_ = rl(__builtin_amdgcn_fmed3f(g1, nlo1, nhi1), src);
            seen1 = (lane_s == src) ? g1 : seen1;
            asm volatile("" : "+v"(seen1));
            g0 = fmaf(a0[q], dl_, g0);
            g1 = fmaf(a1[q], dl_, g1);
          }
        }
      }
      const float dl0 = __builtin_amdgcn_fmed3f(seen0, nlo0, nhi0), dl1 = has1 ? __builtin_amdgcn_fmed3f(seen1, nlo1, nhi1) : 0.f;
      const float improvement = -wave_sum(dl0 * aii0 * (0.5f * dl0 - seen0) + (has1 ? dl1 * aii1 * (0.5f * dl1 - seen1) : 0.f));
      f0 = (dl0 == nlo0) ? lo0 : ((dl0 == nhi0) ? hi0 : f0 + dl0);
      if (has1) f1 = (dl1 == nlo1) ? lo1 : ((dl1 == nhi1) ? hi1 : f1 + dl1);
      iter++;
      if (improvement * T.pgs_scale < T.tolerance) break;
    }
    fr[0] = f0; fr[1] = f1;
  } else {
    // 129..256 rows (bodies lying on the floor with many mesh / floor contacts — the DPCombinedEnv getup phases): four rows per
    // lane, the same scaled-residual step; the four A columns of a row are requested a block of PF rows ahead (the block's
    // owner register set is uniform: PF divides 64)
    float g[4], f[4], lo[4], hi[4], nainv[4], aii[4];
    bool has[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      has[m] = m < nr && lane + 64 * m < nefc;
      f[m] = fr[m]; aii[m] = diag[m]; nainv[m] = -dinv[m];
      lo[m] = lm[m] >= 0.f ? -lm[m] : 0.f;
      hi[m] = lm[m] >= 0.f ? lm[m] : __builtin_inff();
      g[m] = res[m] * nainv[m];
    }
    while (iter < max_iter) {
      float nlo[4], nhi[4], seen[4];
#pragma unroll
      for (int m = 0; m < 4; m++) { nlo[m] = lo[m] - f[m]; nhi[m] = hi[m] - f[m]; seen[m] = g[m]; }
      int lane_s = lane;
      asm volatile("" : "+v"(lane_s));
      for (int i0 = 0; i0 < nefc; i0 += PF) {
        float a[4][PF];
#pragma unroll
        for (int q = 0; q < PF; q++) {
          const int i = i0 + q;
#pragma unroll
          for (int m = 0; m < 4; m++) a[m][q] = (i < nefc && has[m]) ? AR[i * MAXROW + lane + 64 * m] : 0.f;
        }
#define PGS_BLOCK(M)                                                                        \
        _Pragma("unroll") for (int q = 0; q < PF; q++) {                                    \
          const int src = (i0 + q) & 63;                                                    \
          if (i0 + q < nefc) {                                                              \
            const float dl_ = rl(__builtin_amdgcn_fmed3f(g[M], nlo[M], nhi[M]), src);    \
            seen[M] = (lane_s == src) ? g[M] : seen[M];                                     \
            asm volatile("" : "+v"(seen[M]));                                               \
            _Pragma("unroll") for (int m = 0; m < 4; m++) g[m] = fmaf(a[m][q], dl_, g[m]); \
          }                                                                                 \
        }
        switch (i0 >> 6) {
          case 0: PGS_BLOCK(0) break;
          case 1: PGS_BLOCK(1) break;
          case 2: PGS_BLOCK(2) break;
          default: PGS_BLOCK(3) break;
        }
#undef PGS_BLOCK
      }
      float imp = 0.f;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const float dl = has[m] ? __builtin_amdgcn_fmed3f(seen[m], nlo[m], nhi[m]) : 0.f;
        imp += dl * aii[m] * (0.5f * dl - seen[m]);
        if (has[m]) f[m] = (dl == nlo[m]) ? lo[m] : ((dl == nhi[m]) ? hi[m] : f[m] + dl);
      }
      const float improvement = -wave_sum(imp);
      iter++;
      if (improvement * T.pgs_scale < T.tolerance) break;
    }
#pragma unroll
    for (int m = 0; m < 4; m++) fr[m] = f[m];
  }
  PROF(12);
#pragma unroll
  for (int m = 0; m < 4; m++) { const int r = lane + 64 * m; if (m < nr && r < nefc) e_f[r] = fr[m]; }
  SYNC();
  // qfrc_constraint = J^T f: lane k owns dof k and walks its row of J^T (eight loads in flight; 43 wave reductions of row
  // products were 1 700 instructions per evaluation)
  if (lane < NV) {
    const float *jk = JT + lane * MAXROW;
    float s = 0;
    for (int r0 = 0; r0 < nefc; r0 += 8) {
      float a[8], fc[8];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const bool ok = r0 + q < nefc;
        a[q] = ok ? jk[r0 + q] : 0.f;
        fc[q] = ok ? e_f[r0 + q] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; q++) s = fmaf(a[q], fc[q], s);
    }
    S.qfc[lane] = s; S.tmp[lane] = s;
  }
  SYNC();
  solve_m(T, S.tmp, lane);
  SYNC();
  if (lane < NV) { const float a = S.tmp[lane] + S.qas[lane]; S.qacc[lane] = a; S.warm[lane] = a; }
  if (lane == 0) S.info[3] = iter;
  SYNC();
}

}  // namespace g1
