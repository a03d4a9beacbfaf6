// Stand-alone host program of tests/test_lane_records_cpu.py: every field of the lane-major records (csrc/dm_tables.h) has the
// bits of the DmDev entry it replaces.  The tables are synthetic: every 32-bit word of DmDev holds its own index pattern, so
// two different entries never compare equal; only the indices the builder follows (b_dofadr, b_dofnum, g_body) are valid ids.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../deepmimic_mujoco_amd/csrc/dm_tables.h"

// the chunk offsets the kernels address (REC4(record, chunk) in dm_kernels.hip)
static_assert(offsetof(DmBodyRec, dofadr) == 0 && offsetof(DmBodyRec, chainb) == 8 && offsetof(DmBodyRec, pos) == 16 &&
              offsetof(DmBodyRec, mass) == 28 && offsetof(DmBodyRec, axis) == 32 && offsetof(DmBodyRec, ipos) == 68 &&
              offsetof(DmBodyRec, inertia) == 80, "body record layout");
static_assert(offsetof(DmDofRec, body) == 0 && offsetof(DmDofRec, arm) == 12 && offsetof(DmDofRec, madr) == 16 &&
              offsetof(DmDofRec, damp) == 24 && offsetof(DmDofRec, clo) == 32 && offsetof(DmDofRec, ancm) == 40, "dof record layout");
static_assert(offsetof(DmGeomRec, pos) == 0 && offsetof(DmGeomRec, body) == 12 && offsetof(DmGeomRec, mat) == 16, "geom record layout");
static_assert(offsetof(DmContactRowRec, condim) == 0 && offsetof(DmContactRowRec, mu) == 4 && offsetof(DmContactRowRec, margin) == 8 &&
              offsetof(DmContactRowRec, invw) == 12 && offsetof(DmContactRowRec, chain) == 16 && offsetof(DmContactRowRec, body) == 24, "contact-row record layout");
static_assert(offsetof(DmLimitRowRec, lo) == 0 && offsetof(DmLimitRowRec, invw) == 8, "limit-row record layout");
static_assert(offsetof(DmDev, rec) % 16 == 0 && sizeof(DmDev) % 16 == 0, "records start on a 16-byte boundary");

static long checks = 0, bad = 0;

static void same(const void *rec, const void *tab, size_t n, const char *what, int idx) {
  checks++;
  if (memcmp(rec, tab, n) != 0) {
    if (bad++ < 20) fprintf(stderr, "MISMATCH %s at %d\n", what, idx);
  }
}
#define SAME(recfield, tabentry, what, idx)                                        \
  do {                                                                             \
    static_assert(sizeof(recfield) == sizeof(tabentry), "field sizes differ: " what); \
    same(&(recfield), &(tabentry), sizeof(recfield), what, idx);                   \
  } while (0)

int main() {
  static DmDev T;
  const size_t nw = offsetof(DmDev, rec) / 4;
  uint32_t *w = reinterpret_cast<uint32_t *>(&T);
  for (size_t i = 0; i < nw; i++) w[i] = 0x3C000000u + (uint32_t)i * 0x101u;     // distinct, finite as fp32, never zero
  // the ids the builder follows: a made-up but valid tree (1 to 3 hinges per body, geoms spread over the bodies)
  for (int b = 0; b < 16; b++) {
    T.b_dofnum[b] = 1 + b % 3;
    T.b_dofadr[b] = (b * 5) % (DM_NV - 2);
  }
  for (int g = 0; g < 16; g++) T.g_body[g] = (g * 5 + 3) % DM_NBODY;
  dm_build_lane_records(T);
  const DmLaneRec &R = T.rec;

  const float zero3[3] = {0.f, 0.f, 0.f};
  for (int l = 0; l < DMK_REC_LANES; l++) {
    const int b = l < DM_NBODY ? l : 0, k = l < DM_NV ? l : 0, g = l < DM_NGEOM ? l : 0;   // lanes past the role count: entry 0
    const DmBodyRec &rb = R.body[l];
    SAME(rb.dofadr, T.b_dofadr[b], "b_dofadr", l);
    SAME(rb.dofnum, T.b_dofnum[b], "b_dofnum", l);
    SAME(rb.chainb, T.b_chainb[b], "b_chainb", l);
    SAME(rb.subtree, T.b_subtree[b], "b_subtree", l);
    SAME(rb.pos, T.b_pos[b], "b_pos", l);
    SAME(rb.mass, T.b_mass[b], "b_mass", l);
    SAME(rb.ipos, T.b_ipos[b], "b_ipos", l);
    SAME(rb.inertia, T.b_inertia[b], "b_inertia", l);
    for (int j = 0; j < 3; j++) {
      if (j < T.b_dofnum[b]) SAME(rb.axis[j], T.d_axis[T.b_dofadr[b] + j], "d_axis[b_dofadr + j]", l);
      else SAME(rb.axis[j], zero3, "axis past b_dofnum", l);
    }
    const DmDofRec &rd = R.dof[l];
    SAME(rd.body, T.d_body[k], "d_body", l);
    SAME(rd.nanc, T.d_nanc[k], "d_nanc", l);
    SAME(rd.pbody, T.d_pbody[k], "d_pbody", l);
    SAME(rd.madr, T.d_madr[k], "d_madr", l);
    SAME(rd.ancm, T.d_ancm[k], "d_ancm", l);
    SAME(rd.arm, T.d_arm[k], "d_arm", l);
    SAME(rd.damp, T.d_damp[k], "d_damp", l);
    SAME(rd.act, T.d_act[k], "d_act", l);
    SAME(rd.gear, T.d_gear[k], "d_gear", l);
    SAME(rd.clo, T.d_clo[k], "d_clo", l);
    SAME(rd.chi, T.d_chi[k], "d_chi", l);
    const DmGeomRec &rg = R.geom[l];
    SAME(rg.body, T.g_body[g], "g_body", l);
    SAME(rg.pos, T.g_pos[g], "g_pos", l);
    SAME(rg.mat, T.g_mat[g], "g_mat", l);
  }
  for (int g = 0; g < DM_NGEOM; g++) {
    const DmContactRowRec &rc = R.crow[g];
    const int b = T.g_body[g];
    SAME(rc.body, T.g_body[g], "crow g_body", g);
    SAME(rc.condim, T.g_condim[g], "crow g_condim", g);
    SAME(rc.mu, T.g_mu[g], "crow g_mu", g);
    SAME(rc.margin, T.g_margin[g], "crow g_margin", g);
    SAME(rc.invw, T.b_invw[b], "crow b_invw[g_body]", g);
    SAME(rc.chain, T.b_chain[b], "crow b_chain[g_body]", g);
  }
  for (int k = 0; k < DM_NV; k++) {
    const DmLimitRowRec &rl = R.lrow[k];
    SAME(rl.lo, T.d_lo[k], "lrow d_lo", k);
    SAME(rl.hi, T.d_hi[k], "lrow d_hi", k);
    SAME(rl.invw, T.d_invw[k], "lrow d_invw", k);
  }
  // the tables in front of the records are what they were
  for (size_t i = 0; i < nw; i++) {
    const uint32_t *p = &w[i];
    const bool id = (p >= (uint32_t *)T.b_dofadr && p < (uint32_t *)(T.b_dofadr + 16)) || (p >= (uint32_t *)T.b_dofnum && p < (uint32_t *)(T.b_dofnum + 16)) ||
                    (p >= (uint32_t *)T.g_body && p < (uint32_t *)(T.g_body + 16));
    if (!id && w[i] != 0x3C000000u + (uint32_t)i * 0x101u) { bad++; fprintf(stderr, "table word %zu was overwritten\n", i); break; }
  }
  printf("lane records: %ld checks, %ld mismatches\n", checks, bad);
  return bad ? 1 : 0;
}
