// dm_tables_host.h — what the humanoid engine computes on the host from a DmModel and a clip: the model check, the fp32 device
// tables (DmDev) and the clip and reset rows.  Pure host arithmetic into memory the caller passes: no HIP runtime call, no kernel,
// so a stand-alone program runs it on a CPU (tests/host/host_tables.hip).  dm_device.h is here for the layouts only.
#pragma once

#include "dm_device.h"
#include "dm_host.h"
#include "dm_topology.h"

// DM_OK, or DM_EINVAL and why.  Every index build_tables and the kernels take from the model is in range afterwards.
static int check_model(const DmModel &m, std::string &err) {
  if (m.nq != DM_NQ || m.nv != DM_NV || m.nu != DM_NU || m.nbody != DM_NBODY || m.ngeom != DM_NGEOM)
    DM_REJECT("model dimensions do not match the compiled-in humanoid3d dimensions");
  if (m.integrator != DM_INT_RK4 && m.integrator != DM_INT_EULER) DM_REJECT("integrator must be RK4 or Euler");
  if (m.npair < 0 || m.npair > DM_MAXPAIR) DM_REJECT("npair out of range");
  DM_PRECEDES(body_parent, 1, DM_NBODY, 0);
  DM_PRECEDES(dof_parent, 0, DM_NV, -1);
  DM_RANGE(dof_body, DM_NV, 0, DM_NBODY);
  DM_RANGE(dof_jnt, DM_NV, 0, DM_NJNT);
  DM_RANGE(act_dof, DM_NU, 0, DM_NV);
  DM_RANGE(geom_body, DM_NGEOM, 0, DM_NBODY);
  DM_RANGE(pair_geom1, m.npair, 0, DM_NGEOM);
  DM_RANGE(pair_geom2, m.npair, 0, DM_NGEOM);
  DM_RANGE(ee_geom, DM_NEE, 0, DM_NGEOM);
  DM_RANGE(torso_body, 1, 0, DM_NBODY);
  DM_RANGE(rfoot_geom, 1, 0, DM_NGEOM);
  DM_RANGE(lfoot_geom, 1, 0, DM_NGEOM);
  DM_RANGE(floor_geom, 1, 0, DM_NGEOM);
  for (int b = 1; b < DM_NBODY; b++) {
    if (m.body_quat[b][0] != 1.0) DM_REJECT("kernels assume identity body quaternions");
    if (m.body_dofnum[b] != 1 && m.body_dofnum[b] != 3 && m.body_dofnum[b] != 6)
      DM_REJECT("kernels assume 1- or 3-hinge bodies under a free root");
    if (m.body_dofadr[b] < 0 || m.body_dofadr[b] + m.body_dofnum[b] > DM_NV) DM_REJECT("body_dofadr out of range");
    if (m.body_depth[b] < 1 || m.body_depth[b] > 4) DM_REJECT("tree depth > 4");
  }
  for (int j = 0; j < DM_NJNT; j++)
    for (int i = 0; i < 3; i++)
      if (m.jnt_pos[j][i] != 0.0) DM_REJECT("kernels assume joint anchors at the body origin");
  if (m.jnt_type[0] != DM_JNT_FREE || m.jnt_body[0] != 1) DM_REJECT("joint 0 must be the free root");
  for (int k = 0; k < DM_NV; k++)
    if (m.dof_parent[k] != topo::PARENT[k] || m.dof_Madr[k] != topo::MADR[k])
      DM_REJECT("dof tree differs from the compiled-in topology (regenerate csrc/dm_topology.h)");
  for (int b = 0; b < DM_NBODY; b++)
    if (m.body_parent[b] != topo::BPARENT[b])
      DM_REJECT("body tree differs from the compiled-in topology (regenerate csrc/dm_topology.h)");
  return DM_OK;
}

static void build_tables(const DmModel &m, DmDev &T) {
  memset(&T, 0, sizeof(T));
  T.timestep = (float)m.timestep;
  T.tolerance = (float)m.tolerance;
  T.pgs_scale = (float)(1.0 / (m.meaninertia * (DM_NV > 1 ? DM_NV : 1)));
  for (int i = 0; i < 3; i++) T.gravity[i] = (float)m.gravity[i];
  dm_ref_kb(m.solref, m.solimp, m.timestep, T.K, T.B);
  for (int i = 0; i < 5; i++) T.solimp[i] = (float)m.solimp[i];
  double mt = 0;
  for (int b = 0; b < DM_NBODY; b++) mt += m.body_mass[b];
  T.total_mass_inv = (float)(1.0 / mt);
  for (int i = 0; i < DM_NQ; i++) T.qpos0[i] = (float)m.qpos0[i];
  T.iterations = m.iterations;
  T.npair = m.npair;
  T.torso_body = m.torso_body; T.rfoot_geom = m.rfoot_geom; T.lfoot_geom = m.lfoot_geom; T.floor_geom = m.floor_geom;
  for (int i = 0; i < 4; i++) T.ee_geom[i] = m.ee_geom[i];
  for (int b = 0; b < DM_NBODY; b++) {
    T.b_parent[b] = m.body_parent[b]; T.b_depth[b] = m.body_depth[b];
    T.b_dofadr[b] = m.body_dofadr[b] < 0 ? 0 : m.body_dofadr[b]; T.b_dofnum[b] = m.body_dofnum[b];
    for (int i = 0; i < 3; i++) { T.b_pos[b][i] = (float)m.body_pos[b][i]; T.b_ipos[b][i] = (float)m.body_ipos[b][i]; }
    for (int i = 0; i < 6; i++) T.b_inertia[b][i] = (float)m.body_inertia[b][i];
    T.b_mass[b] = (float)m.body_mass[b];
    T.b_invw[b] = (float)m.body_invweight0[b][0];
    uint32_t sub = 0;
    for (int c = 1; c < DM_NBODY; c++) {
      int a = c;
      while (a > 0 && a != b) a = m.body_parent[a];
      if (a == b && b > 0) sub |= 1u << c;
    }
    T.b_subtree[b] = sub;
    uint64_t chain = 0;
    for (int a = b; a > 0; a = m.body_parent[a])
      for (int k = 0; k < m.body_dofnum[a]; k++) chain |= 1ull << (m.body_dofadr[a] + k);
    T.b_chain[b] = chain;
    uint32_t cb = 0;
    int ids[8], nc = 0;
    for (int a = b; a > 0; a = m.body_parent[a]) ids[nc++] = a;
    for (int c = 0; c < nc && c < 4; c++) cb |= (uint32_t)ids[nc - 1 - c] << (8 * c);   // root first
    T.b_chainb[b] = cb;
  }
  for (int k = 0; k < DM_NV; k++) {
    int j = m.dof_jnt[k];
    T.d_body[k] = m.dof_body[k];
    T.d_act[k] = -1;
    T.d_limited[k] = (m.jnt_type[j] == DM_JNT_HINGE) ? m.jnt_limited[j] : 0;
    for (int i = 0; i < 3; i++) T.d_axis[k][i] = (float)m.jnt_axis[j][i];
    T.d_arm[k] = (float)m.dof_armature[k]; T.d_damp[k] = (float)m.dof_damping[k];
    T.d_invw[k] = (float)m.dof_invweight0[k];
    T.d_lo[k] = (float)m.jnt_range[j][0]; T.d_hi[k] = (float)m.jnt_range[j][1];
    int n = 0;
    for (int a = m.dof_parent[k]; a >= 0 && n < DMK_MAXANC; a = m.dof_parent[a]) T.d_anc[k][n++] = (uint8_t)a;
    T.d_nanc[k] = n;
    for (int d = 0; d < n; d++) T.d_ancabs[k][d] = T.d_anc[k][n - 1 - d];   // absolute depth d
    T.d_pbody[k] = m.body_parent[m.dof_body[k]];
  }
  for (int k = 0; k < DM_NV; k++) {
    for (int a = 0; a < T.d_nanc[k]; a++) T.d_desc[T.d_anc[k][a]] |= 1ull << k;
    T.nanc_pack[k >> 4] |= (uint64_t)T.d_nanc[k] << (4 * (k & 15));
    for (int a = 0; a < T.d_nanc[k]; a++) T.d_ancm[k] |= 1ull << T.d_anc[k][a];
    T.d_madr[k] = m.dof_Madr[k];
  }
  for (int a = 0; a < DM_NU; a++) {
    int k = m.act_dof[a];
    T.d_act[k] = a; T.d_gear[k] = (float)m.act_gear[a];
    T.d_clo[k] = (float)m.act_ctrlrange[a][0]; T.d_chi[k] = (float)m.act_ctrlrange[a][1];
  }
  for (int g = 0; g < DM_NGEOM; g++) {
    T.g_body[g] = m.geom_body[g]; T.g_type[g] = m.geom_type[g]; T.g_condim[g] = m.geom_condim[g];
    for (int i = 0; i < 3; i++) { T.g_pos[g][i] = (float)m.geom_pos[g][i]; T.g_size[g][i] = (float)m.geom_size[g][i]; }
    double M[9];
    dm_quat_to_mat(m.geom_quat[g], M);
    for (int i = 0; i < 9; i++) T.g_mat[g][i] = (float)M[i];
    T.g_rbound[g] = (float)m.geom_rbound[g]; T.g_margin[g] = (float)m.geom_margin[g];
    T.g_mu[g] = (float)m.geom_friction[g][0];
  }
  for (int p = 0; p < DM_MAXPAIR; p++) { T.p_g1[p] = (int16_t)m.pair_geom1[p]; T.p_g2[p] = (int16_t)m.pair_geom2[p]; }
  for (int p = 0; p < m.npair; p++) {
    int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    DmPairDev &pr = T.pairs[p];
    pr.g1 = (int16_t)g1; pr.g2 = (int16_t)g2;
    pr.t1 = (int8_t)m.geom_type[g1]; pr.t2 = (int8_t)m.geom_type[g2];
    pr.margin = (float)fmax(m.geom_margin[g1], m.geom_margin[g2]);
    pr.rbsum = (float)((m.geom_type[g1] == DM_GEOM_PLANE ? 0.0 : m.geom_rbound[g1]) + m.geom_rbound[g2]);
    for (int i = 0; i < 3; i++) { pr.z1[i] = (float)m.geom_size[g1][i]; pr.z2[i] = (float)m.geom_size[g2][i]; }
  }
  int p = 0;
  for (int b = 0; b < DMK_MAXANC; b++)
    for (int a = 0; a <= b; a++) { T.tri_a[p] = (uint8_t)a; T.tri_b[p] = (uint8_t)b; p++; }
  dm_build_lane_records(T);   // T.rec: the per-lane copies the step kernels load a phase ahead (dm_tables.h)
}

// The clip rows (L x DMK_CLIP_ROW) and reset rows (L x DMK_RESET_ROW) of dm_load_clip, zero-initialised by the caller.
static void pack_clip(const DmModel &m, int L, const double *qpos, const double *qvel, const double *body_xpos, const double *geom_xpos,
                      float *rows, float *reset) {
  for (int f = 0; f < L; f++) {
    float *r = rows + (size_t)f * DMK_CLIP_ROW;
    const double *q = qpos + (size_t)f * DM_NQ, *v = qvel + (size_t)f * DM_NV;
    for (int i = 0; i < 28; i++) { r[i] = (float)q[7 + i]; r[28 + i] = (float)v[6 + i]; }
    for (int i = 0; i < 4; i++) r[56 + i] = (float)q[3 + i];
    for (int ee = 0; ee < 4; ee++)
      for (int i = 0; i < 3; i++) r[60 + 3 * ee + i] = (float)geom_xpos[((size_t)f * DM_NGEOM + m.ee_geom[ee]) * 3 + i];
    double com[3];
    dm_mass_centre(m.body_mass, DM_NBODY, body_xpos + (size_t)f * DM_NBODY * 3, com);
    for (int i = 0; i < 3; i++) { r[72 + i] = (float)com[i]; r[75 + i] = (float)q[i]; }
    r[78] = (float)v[0]; r[79] = (float)v[1];   // root linear velocity xy (DPCombinedEnv task reward)
    float *rr = reset + (size_t)f * DMK_RESET_ROW;
    for (int i = 0; i < DM_NQ; i++) rr[i] = (float)q[i];
    for (int i = 0; i < DM_NV; i++) rr[35 + i] = (float)v[i];
  }
}
