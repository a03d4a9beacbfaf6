// dm_tables.h — the read-only model tables of the step kernels (DmDev) and their lane-major records.
// Plain C++ with no HIP dependency: the host builds both, the kernels only read them, and a stand-alone
// host program can check the records against the tables (tests/test_lane_records_cpu.py).
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/dm_model.h"

#define DMK_MAXANC 12          // deepest dof has 12 ancestors (root 6 + hip 3 + knee 1 + ankle x,y)
#define DMK_REC_LANES 64       // one record per lane and role

// One collision candidate: everything the prefilter and the narrowphase need except the poses.
struct DmPairDev {
  int16_t g1, g2;
  int8_t t1, t2, pad0, pad1;
  float margin, rbsum;   // max of the two margins; sum of the bounding radii (plane: radius of geom 2)
  float z1[3], z2[3];    // geom sizes
};

// Lane-major records: what a lane reads from the tables in one phase, copied next to each other in 16-byte
// chunks and indexed by the lane itself, so that a phase's constants arrive in a few 16-byte loads at
// base + lane * stride + constant, none of them behind an index that has to be loaded first.  Every field is a plain
// copy of the DmDev entry it replaces (same bits); lanes beyond a role's count repeat entry 0, as lb / lk / lg do.
struct alignas(16) DmBodyRec {     // lane = body
  int32_t dofadr, dofnum; uint32_t chainb, subtree;   // b_dofadr, b_dofnum, b_chainb, b_subtree (read again by the velocity stage)
  float pos[3], mass;                        // b_pos, b_mass
  float axis[3][3];                          // d_axis[b_dofadr + j] of the body's up to three hinges (zero for j >= b_dofnum)
  float ipos[3];                             // b_ipos
  float inertia[6]; uint32_t pad[2];         // b_inertia
};
struct alignas(16) DmDofRec {      // lane = dof
  int32_t body, nanc, pbody; float arm;      // d_body, d_nanc, d_pbody, d_arm: kinematics .. columns of M
  int32_t madr, act; float damp, gear;       // d_madr, d_act, d_damp, d_gear: after the factorisation
  float clo, chi; uint64_t ancm;             // d_clo, d_chi, d_ancm
};
struct alignas(16) DmGeomRec {     // lane = geom
  float pos[3]; int32_t body;                // g_pos, g_body
  float mat[9]; uint32_t pad[3];             // g_mat
};
struct alignas(16) DmContactRowRec {   // index = geom id: what a contact row needs of one of its two geoms
  int32_t condim; float mu, margin, invw;    // g_condim, g_mu, g_margin, b_invw[g_body]
  uint64_t chain; int32_t body; uint32_t pad;   // b_chain[g_body], g_body
};
struct alignas(16) DmLimitRowRec {     // index = dof: what a joint-limit row needs
  float lo, hi, invw; uint32_t pad;          // d_lo, d_hi, d_invw
};
static_assert(sizeof(DmBodyRec) == 112 && sizeof(DmDofRec) == 48 && sizeof(DmGeomRec) == 64 && sizeof(DmContactRowRec) == 32 &&
              sizeof(DmLimitRowRec) == 16, "the kernels address the records by 16-byte chunk");
struct alignas(16) DmLaneRec {
  DmBodyRec body[DMK_REC_LANES];
  DmDofRec dof[DMK_REC_LANES];
  DmGeomRec geom[DMK_REC_LANES];
  DmContactRowRec crow[DM_NGEOM];
  DmLimitRowRec lrow[DM_NV];
};

// Global-memory (read-only) model tables, fp32.  Built on the host from DmModel.
struct DmDev {
  // scalars
  float timestep, tolerance, pgs_scale, gravity[3];
  float K, B;               // reference-acceleration stiffness / damping (refsafe applied)
  float solimp[5];
  float total_mass_inv;
  float qpos0[36];
  int32_t iterations, npair;
  int32_t torso_body, rfoot_geom, lfoot_geom, floor_geom;
  int32_t ee_geom[4];
  // bodies
  int32_t b_parent[16], b_depth[16], b_dofadr[16], b_dofnum[16];
  float b_pos[16][3], b_ipos[16][3], b_inertia[16][6], b_mass[16], b_invw[16];
  uint32_t b_subtree[16];       // bit c: body c is in the subtree of b (incl. b)
  uint64_t b_chain[16];         // bit k: dof k moves body b
  uint32_t b_chainb[16];        // ancestor bodies root..self, one byte each (0 = none)
  // dofs
  int32_t d_body[DM_NV], d_nanc[DM_NV], d_act[DM_NV], d_limited[DM_NV];
  float d_axis[DM_NV][3];       // joint axis in the body frame (hinges)
  float d_arm[DM_NV], d_damp[DM_NV], d_invw[DM_NV], d_lo[DM_NV], d_hi[DM_NV];
  float d_gear[DM_NV], d_clo[DM_NV], d_chi[DM_NV];
  uint8_t d_anc[DM_NV][DMK_MAXANC];
  uint8_t d_ancabs[DM_NV][DMK_MAXANC + 4]; // ancestor dof at absolute depth d (0 if none)
  uint64_t d_desc[DM_NV];       // bit k: dof k is a strict descendant
  int32_t d_pbody[DM_NV];       // parent body of the dof's body
  uint64_t nanc_pack[3];        // d_nanc of every dof, 4 bits each
  uint64_t d_ancm[DM_NV];       // bit j: dof j is a strict ancestor
  int32_t d_madr[DM_NV];        // start of row i in the sparse factor
  // geoms
  int32_t g_body[16], g_type[16], g_condim[16];
  float g_pos[16][3], g_mat[16][9], g_size[16][3], g_rbound[16], g_margin[16], g_mu[16];
  // candidate pairs (canonical order)
  int16_t p_g1[DM_MAXPAIR], p_g2[DM_MAXPAIR];
  DmPairDev pairs[DM_MAXPAIR];
  uint8_t tri_a[80], tri_b[80]; // lower-triangle pair decode for the factorisation
  // lane-major records of the fields above (dm_build_lane_records), 16-byte aligned
  DmLaneRec rec;
};

// Fills T.rec from the other fields of T alone.  Host only.
static inline void dm_build_lane_records(DmDev &T) {
  DmLaneRec &R = T.rec;
  memset(&R, 0, sizeof(R));
  for (int l = 0; l < DMK_REC_LANES; l++) {
    const int b = l < DM_NBODY ? l : 0, k = l < DM_NV ? l : 0, g = l < DM_NGEOM ? l : 0;
    DmBodyRec &rb = R.body[l];
    for (int i = 0; i < 3; i++) { rb.pos[i] = T.b_pos[b][i]; rb.ipos[i] = T.b_ipos[b][i]; }
    for (int i = 0; i < 6; i++) rb.inertia[i] = T.b_inertia[b][i];
    rb.mass = T.b_mass[b];
    rb.dofadr = T.b_dofadr[b]; rb.dofnum = T.b_dofnum[b];
    rb.chainb = T.b_chainb[b]; rb.subtree = T.b_subtree[b];
    for (int j = 0; j < 3; j++) {
      const int d = T.b_dofadr[b] + j;
      if (j < T.b_dofnum[b] && d >= 0 && d < DM_NV)
        for (int i = 0; i < 3; i++) rb.axis[j][i] = T.d_axis[d][i];
    }
    DmDofRec &rd = R.dof[l];
    rd.body = T.d_body[k]; rd.nanc = T.d_nanc[k]; rd.pbody = T.d_pbody[k]; rd.madr = T.d_madr[k];
    rd.ancm = T.d_ancm[k]; rd.arm = T.d_arm[k]; rd.damp = T.d_damp[k];
    rd.act = T.d_act[k]; rd.gear = T.d_gear[k]; rd.clo = T.d_clo[k]; rd.chi = T.d_chi[k];
    DmGeomRec &rg = R.geom[l];
    for (int i = 0; i < 3; i++) rg.pos[i] = T.g_pos[g][i];
    for (int i = 0; i < 9; i++) rg.mat[i] = T.g_mat[g][i];
    rg.body = T.g_body[g];
  }
  for (int g = 0; g < DM_NGEOM; g++) {
    DmContactRowRec &rc = R.crow[g];
    const int b = T.g_body[g];
    rc.body = b; rc.condim = T.g_condim[g]; rc.mu = T.g_mu[g]; rc.margin = T.g_margin[g];
    if (b >= 0 && b < DM_NBODY) { rc.chain = T.b_chain[b]; rc.invw = T.b_invw[b]; }
  }
  for (int k = 0; k < DM_NV; k++) {
    DmLimitRowRec &rl = R.lrow[k];
    rl.lo = T.d_lo[k]; rl.hi = T.d_hi[k]; rl.invw = T.d_invw[k];
  }
}
