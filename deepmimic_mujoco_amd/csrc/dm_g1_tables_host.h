// dm_g1_tables_host.h — what the G1 engine computes on the host from a DmModelG1 and a clip: the model check, the device tables
// (g1::Dev), the hulls reordered into vertex clusters, and the clip, reset and COM rows.  Pure host arithmetic into memory the caller
// passes: no HIP runtime call, no kernel, so a stand-alone program runs it on a CPU (tests/host/host_tables.hip).  dm_g1_device.h is
// here for the layouts only.
#pragma once

#include "dm_g1_device.h"
#include "dm_g1_topology.h"
#include "dm_host.h"

#include <string.h>

// DM_OK, or DM_EINVAL and why.  Every index g1_build_tables, g1_build_meshes and the kernels take from the model is in range afterwards.
static int g1_check_model(const DmModelG1 &m, std::string &err) {
  using namespace g1;
  if (m.nq != NQ || m.nv != NV || m.nu != NU || m.nbody != NB || m.ngeom != NG || m.njnt != NJ || m.nM != NM)
    DM_REJECT("model dimensions are not the Unitree G1's");
  if (m.integrator != DM_INT_RK4 && m.integrator != DM_INT_EULER) DM_REJECT("integrator must be RK4 or Euler");
  if (m.npair < 0 || m.npair > 1024) DM_REJECT("npair out of range");
  DM_PRECEDES(body_parent, 1, NB, 0);
  DM_PRECEDES(dof_parent, 0, NV, -1);
  DM_RANGE(dof_body, NV, 0, NB);
  DM_RANGE(dof_jnt, NV, 0, NJ);
  DM_RANGE(act_dof, NU, 0, NV);
  DM_RANGE(geom_body, NG, 0, NB);
  DM_RANGE(pair_geom1, m.npair, 0, NG);
  DM_RANGE(pair_geom2, m.npair, 0, NG);
  DM_RANGE(geom_mesh, NG, -1, DM_NMESH);
  DM_RANGE(mesh_vertnum, DM_NMESH, 0, DM_NMESHVERT + 1);
  for (int me = 0; me < DM_NMESH; me++)
    if (m.mesh_vertadr[me] < 0 || m.mesh_vertadr[me] > DM_NMESHVERT - m.mesh_vertnum[me]) DM_REJECT("mesh_vertadr out of range");
  DM_RANGE(ee_geom, 4, 0, NG);
  DM_RANGE(extra_geom, 8, 0, NG);
  DM_RANGE(torso_body, 1, 0, NB);
  DM_RANGE(rfoot_geom, 1, 0, NG);
  DM_RANGE(lfoot_geom, 1, 0, NG);
  DM_RANGE(floor_geom, 1, 0, NG);
  DM_RANGE(rew_qposadr, NREW, 0, NQ);
  DM_RANGE(rew_dofadr, NREW, 0, NV);
  DM_RANGE(rew_jnt, NREW, 0, NJ);
  if (m.jnt_type[0] != DM_JNT_FREE || m.jnt_body[0] != 1) DM_REJECT("joint 0 must be the free root");
  if (m.body_dofadr[1] != 0 || m.body_dofnum[1] != 6) DM_REJECT("body_dofadr out of range: body 1 carries the free root's six dofs");
  for (int b = 2; b < NB; b++)
    if (m.body_jntnum[b] != 1 || m.body_dofnum[b] != 1 || m.body_dofadr[b] != b + 4 || m.body_jntadr[b] != b - 1 || m.body_depth[b] > 15)
      DM_REJECT("kernel assumes one hinge per body in body order");
  for (int j = 0; j < NJ; j++)
    for (int i = 0; i < 3; i++)
      if (m.jnt_pos[j][i] != 0.0) DM_REJECT("kernel assumes joint anchors at the body origin");
  for (int k = 0; k < NV; k++) {
    int n = 0;
    for (int j = m.dof_parent[k]; j >= 0; j = m.dof_parent[j]) n++;
    if (n > 14) DM_REJECT("dof chain deeper than 14 ancestors");
    if (m.dof_parent[k] != g1topo::PARENT[k] || m.dof_Madr[k] != g1topo::MADR[k])
      DM_REJECT("dof tree differs from the compiled-in topology (regenerate csrc/dm_g1_topology.h)");
    if (k >= 6 && !(m.dof_frictionloss[k] > 0)) DM_REJECT("kernel assumes friction loss on every hinge");
  }
  for (int a = 0; a < NU; a++)
    if (m.act_gear[a] != 1.0) DM_REJECT("kernel assumes motor gear 1");
  {
    int seen[DM_NGEOM] = {0}, nci = 0;
    for (int p = 0; p < m.npair; p++) { seen[m.pair_geom1[p]] = 1; seen[m.pair_geom2[p]] = 1; }
    for (int g = 0; g < NG; g++) {
      nci += seen[g];
      if (seen[g] && m.geom_type[g] == DM_GEOM_MESH && m.geom_mesh[g] < 0) DM_REJECT("geom_mesh out of range: a colliding mesh geom without a mesh");
    }
    if (nci > NCG) DM_REJECT("more colliding geoms than the kernel's LDS layout holds");
  }
  for (int g = 0; g < NG; g++)
    if (m.geom_margin[g] != 0.0) DM_REJECT("kernel assumes zero geom margins (xml has none)");
  return DM_OK;
}

static void g1_build_tables(const DmModelG1 &m, g1::Dev &T) {
  using namespace g1;
  memset(&T, 0, sizeof T);
  T.timestep = (float)m.timestep; T.tolerance = (float)m.tolerance;
  T.pgs_scale = (float)(1.0 / (m.meaninertia * (double)NV));
  dm_ref_kb(m.solref, m.solimp, m.timestep, T.K, T.B);
  for (int i = 0; i < 5; i++) T.solimp[i] = (float)m.solimp[i];
  for (int i = 0; i < 3; i++) T.gravity[i] = (float)m.gravity[i];
  double mt = 0;
  for (int b = 1; b < NB; b++) mt += m.body_mass[b];
  T.total_mass_inv = (float)(1.0 / mt);
  T.low_z = (float)m.low_z; T.action_scale = (float)m.action_scale;
  T.iterations = m.iterations; T.npair = m.npair;
  T.torso_body = m.torso_body; T.floor_geom = m.floor_geom; T.rfoot_geom = m.rfoot_geom; T.lfoot_geom = m.lfoot_geom;
  for (int i = 0; i < 4; i++) T.ee_geom[i] = m.ee_geom[i];
  for (int i = 0; i < 8; i++) T.extra_geom[i] = m.extra_geom[i];
  for (int i = 0; i < NREW; i++) { T.rew_q[i] = m.rew_qposadr[i]; T.rew_v[i] = m.rew_dofadr[i]; T.rew_j[i] = m.rew_jnt[i]; }
  for (int i = 0; i < NQ; i++) { T.qpos0[i] = (float)m.qpos0[i]; T.qpos0_d[i] = m.qpos0[i]; }
  T.timestep_d = m.timestep;
  int maxd = 0;
  for (int b = 0; b < NB; b++) {
    T.b_parent[b] = m.body_parent[b]; T.b_depth[b] = m.body_depth[b]; T.b_dof[b] = m.body_dofadr[b];
    if (m.body_depth[b] > maxd) maxd = m.body_depth[b];
    for (int i = 0; i < 3; i++) { T.b_pos[b][i] = (float)m.body_pos[b][i]; T.b_ipos[b][i] = (float)m.body_ipos[b][i]; }
    for (int i = 0; i < 4; i++) { T.b_quat[b][i] = (float)m.body_quat[b][i]; T.b_quat_d[b][i] = m.body_quat[b][i]; }
    for (int i = 0; i < 3; i++) T.b_pos_d[b][i] = m.body_pos[b][i];
    for (int i = 0; i < 6; i++) T.b_inertia[b][i] = (float)m.body_inertia[b][i];
    T.b_mass[b] = (float)m.body_mass[b]; T.b_invw[b] = (float)m.body_invweight0[b][0];
  }
  T.maxdepth = maxd;
  for (int b = 1; b < NB; b++)
    for (int a = b; a > 0; a = m.body_parent[a]) T.b_desc[a] |= 1ull << b;
  for (int k = 0; k < NV; k++) {
    T.d_body[k] = m.dof_body[k]; T.d_madr[k] = m.dof_Madr[k]; T.d_act[k] = -1;
    int n = 0;
    for (int j = m.dof_parent[k]; j >= 0; j = m.dof_parent[j]) T.d_anc[k][n++] = (uint8_t)j;
    T.d_nanc[k] = n;
    const int j = m.dof_jnt[k];
    for (int i = 0; i < 3; i++) { T.d_axis[k][i] = (float)m.jnt_axis[j][i]; T.d_axis_d[k][i] = m.jnt_axis[j][i]; }
    T.d_arm[k] = (float)m.dof_armature[k]; T.d_damp[k] = (float)m.dof_damping[k]; T.d_invw[k] = (float)m.dof_invweight0[k];
    T.d_floss[k] = (float)m.dof_frictionloss[k];
    T.d_lo[k] = (float)m.jnt_range[j][0]; T.d_hi[k] = (float)m.jnt_range[j][1];
    if (!m.jnt_limited[j]) { T.d_lo[k] = -1e30f; T.d_hi[k] = 1e30f; }
  }
  for (int b = 1; b < NB; b++) {   // dofs that move body b: dofs of b and of its ancestors
    for (int a = b; a > 0; a = m.body_parent[a])
      for (int k = m.body_dofadr[a]; k < m.body_dofadr[a] + m.body_dofnum[a]; k++) T.b_chain[b] |= 1ull << k;
  }
  for (int a = 0; a < NU; a++) {
    const int k = m.act_dof[a];
    T.d_act[k] = a; T.d_clo[k] = (float)m.act_ctrlrange[a][0]; T.d_chi[k] = (float)m.act_ctrlrange[a][1];
  }
  for (int g = 0; g < NG; g++) {
    T.g_body[g] = m.geom_body[g]; T.g_type[g] = m.geom_type[g]; T.g_mesh[g] = m.geom_mesh[g];
    for (int i = 0; i < 3; i++) {
      T.g_pos[g][i] = (float)m.geom_pos[g][i]; T.g_size[g][i] = (float)m.geom_size[g][i];
      T.g_pos_d[g][i] = m.geom_pos[g][i]; T.g_size_d[g][i] = m.geom_size[g][i];
    }
    dm_quat_to_mat(m.geom_quat[g], T.g_mat_d[g]);
    for (int i = 0; i < 9; i++) T.g_mat[g][i] = (float)T.g_mat_d[g][i];
    T.g_rbound[g] = (float)m.geom_rbound[g]; T.g_mu[g] = (float)m.geom_friction[g][0];
    const double *zs = m.geom_size[g];
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (m.geom_type[g] == DM_GEOM_SPHERE) { for (int i = 0; i < 3; i++) { lo[i] = -zs[0]; hi[i] = zs[0]; } }
    else if (m.geom_type[g] == DM_GEOM_CYLINDER) { lo[0] = lo[1] = -zs[0]; hi[0] = hi[1] = zs[0]; lo[2] = -zs[1]; hi[2] = zs[1]; }
    else if (m.geom_type[g] == DM_GEOM_BOX) { for (int i = 0; i < 3; i++) { lo[i] = -zs[i]; hi[i] = zs[i]; } }
    else if (m.geom_type[g] == DM_GEOM_MESH && m.geom_mesh[g] >= 0) {
      const int me = m.geom_mesh[g];
      for (int i = 0; i < 3; i++) { lo[i] = 1e30; hi[i] = -1e30; }
      for (int v = m.mesh_vertadr[me]; v < m.mesh_vertadr[me] + m.mesh_vertnum[me]; v++)
        for (int i = 0; i < 3; i++) { lo[i] = fmin(lo[i], m.mesh_vert[v][i]); hi[i] = fmax(hi[i], m.mesh_vert[v][i]); }
    }
    for (int i = 0; i < 3; i++) { T.g_bc[g][i] = (float)(0.5 * (lo[i] + hi[i])); T.g_bh[g][i] = (float)(0.5 * (hi[i] - lo[i]) * 1.00001 + 1e-6); }
  }
  for (int g = 0; g < 96; g++) T.g_ci[g] = -1;
  int nci = 0;
  for (int p = 0; p < m.npair; p++) {
    T.p_g1[p] = (int16_t)m.pair_geom1[p]; T.p_g2[p] = (int16_t)m.pair_geom2[p];
    for (int q = 0; q < 2; q++) { const int g = q ? m.pair_geom2[p] : m.pair_geom1[p]; if (T.g_ci[g] < 0 && nci < NCG) T.g_ci[g] = nci++; }
  }
  for (int i = 0; i < DM_NMESH; i++)
    for (int k = 0; k < 3; k++) T.m_center[i][k] = m.mesh_center[i][k];   // vertex / cluster ranges: g1_build_meshes
  int p = 0;
  for (int b = 0; b < 15 && p < 128; b++)   // pairs (a <= c), c-major: index p -> (a, c)
    for (int a = 0; a <= b && p < 128; a++) { T.tri_a[p] = (uint8_t)a; T.tri_b[p] = (uint8_t)b; p++; }
  for (int k = 0; k < NV; k++) {
    const int n = T.d_nanc[k], np = n * (n + 1) / 2;
    for (int l = 0; l < 64; l++) {
      uint32_t w = 0;
      for (int hf = 0; hf < 2; hf++) {
        const int q = l + 64 * hf;
        uint32_t t = 0;
        if (q < np) { const int a = T.tri_a[q], c = T.tri_b[q]; t = (uint32_t)(T.d_madr[T.d_anc[k][a]] + (c - a)); }
        w |= t << (16 * hf);
      }
      T.f_tgt[k][l] = w;
    }
  }
}

// Reorder every hull into compact clusters: a k-d partition along the longest extent, split so that the left side is a whole
// number of 64-vertex leaves (every leaf but one per hull is full); a leaf occupies 64 vertex slots (unused slots carry the
// invalid original index 0x7fffffff) and has two bounds: an enclosing sphere (centre shrunk from the mean of the vertices by
// Badoiu-Clarkson steps) and a box about the same centre.
static void g1_kd_split(const DmModelG1 &m, int a0, std::vector<int> &idx, int lo, int hi, std::vector<std::pair<int, int>> &leaves) {
  if (hi - lo <= 64) { leaves.push_back({lo, hi}); return; }
  double mn[3] = {1e30, 1e30, 1e30}, mx[3] = {-1e30, -1e30, -1e30};
  for (int k = lo; k < hi; k++)
    for (int i = 0; i < 3; i++) { mn[i] = fmin(mn[i], m.mesh_vert[a0 + idx[k]][i]); mx[i] = fmax(mx[i], m.mesh_vert[a0 + idx[k]][i]); }
  int ax = 0;
  for (int i = 1; i < 3; i++) if (mx[i] - mn[i] > mx[ax] - mn[ax]) ax = i;
  const int half = (hi - lo) / 2, mid = lo + ((half + 63) / 64) * 64 < hi ? lo + ((half + 63) / 64) * 64 : (lo + hi) / 2;   // left side: full leaves
  std::nth_element(idx.begin() + lo, idx.begin() + mid, idx.begin() + hi, [&](int p, int q) {
    const double vp = m.mesh_vert[a0 + p][ax], vq = m.mesh_vert[a0 + q][ax];
    return vp < vq || (vp == vq && p < q);
  });
  g1_kd_split(m, a0, idx, lo, mid, leaves);
  g1_kd_split(m, a0, idx, mid, hi, leaves);
}
// 0, or -1 if a hull has more than 64 * g1::NCH clusters
static int g1_build_meshes(const DmModelG1 &m, g1::Dev &T, std::vector<double> &verts, std::vector<int32_t> &oidx,
                            std::vector<double> &clus) {
  int vadr = 0, cadr = 0;
  for (int me = 0; me < DM_NMESH; me++) {
    const int n = m.mesh_vertnum[me], a0 = m.mesh_vertadr[me];
    T.m_vadr[me] = vadr; T.m_cadr[me] = cadr; T.m_vnum[me] = 0; T.m_cnum[me] = 0;
    if (n == 0) continue;
    std::vector<int> idx(n);
    for (int k = 0; k < n; k++) idx[k] = k;
    std::vector<std::pair<int, int>> leaves;
    g1_kd_split(m, a0, idx, 0, n, leaves);
    for (auto &lf : leaves) {
      double cc[3] = {0, 0, 0}, rad = 0;
      const int cnt = lf.second - lf.first;
      for (int k = lf.first; k < lf.second; k++) for (int i = 0; i < 3; i++) cc[i] += m.mesh_vert[a0 + idx[k]][i];
      for (int i = 0; i < 3; i++) cc[i] /= cnt;
      auto radius_at = [&](const double *c3) {
        double r = 0;
        for (int k = lf.first; k < lf.second; k++) {
          double d2 = 0;
          for (int i = 0; i < 3; i++) { const double df = m.mesh_vert[a0 + idx[k]][i] - c3[i]; d2 += df * df; }
          r = fmax(r, sqrt(d2));
        }
        return r;
      };
      rad = radius_at(cc);
      {   // a tighter enclosing sphere (Badoiu-Clarkson steps towards the farthest vertex): fewer clusters survive the bound test
        double c2[3] = {cc[0], cc[1], cc[2]};
        for (int it = 1; it <= 200; it++) {
          int far = lf.first; double best = -1;
          for (int k = lf.first; k < lf.second; k++) {
            double d2 = 0;
            for (int i = 0; i < 3; i++) { const double df = m.mesh_vert[a0 + idx[k]][i] - c2[i]; d2 += df * df; }
            if (d2 > best) { best = d2; far = k; }
          }
          for (int i = 0; i < 3; i++) c2[i] += (m.mesh_vert[a0 + idx[far]][i] - c2[i]) / (it + 1);
          const double r2 = radius_at(c2);
          if (r2 < rad) { rad = r2; for (int i = 0; i < 3; i++) cc[i] = c2[i]; }
        }
      }
      for (int k = lf.first; k < lf.second; k++) {
        for (int i = 0; i < 3; i++) verts.push_back(m.mesh_vert[a0 + idx[k]][i]);
        oidx.push_back(idx[k]);
      }
      for (int k = cnt; k < 64; k++) { verts.push_back(0); verts.push_back(0); verts.push_back(0); oidx.push_back(0x7fffffff); }
      clus.push_back(cc[0]); clus.push_back(cc[1]); clus.push_back(cc[2]); clus.push_back(rad * (1 + 1e-9) + 1e-12);
      double hx[3] = {0, 0, 0};
      for (int k = lf.first; k < lf.second; k++)
        for (int i = 0; i < 3; i++) hx[i] = fmax(hx[i], fabs(m.mesh_vert[a0 + idx[k]][i] - cc[i]));
      for (int i = 0; i < 3; i++) clus.push_back(hx[i] * (1 + 1e-9) + 1e-12);
      clus.push_back(0.0);
    }
    const int nclus = (int)leaves.size();
    if (nclus > 64 * g1::NCH) return -1;
    T.m_vnum[me] = nclus * 64; T.m_cnum[me] = nclus;
    vadr += nclus * 64; cadr += nclus;
  }
  return 0;
}

// The clip rows (L x CLIP_ROW), reset rows (L x RESET_ROW) and COM rows (L x COM_ROW) of dmg1_load_clip, zero-initialised by the
// caller.  T: the host copy of the tables the engine was created with (its fp32 masses weigh the COM).
static void g1_pack_clip(const g1::Dev &T, int L, const double *q, const double *v, const double *bx, const double *gx, float *rows,
                         float *reset, float *com) {
  using namespace g1;
  for (int f = 0; f < L; f++) {
    float *r = rows + (size_t)f * CLIP_ROW;
    for (int i = 0; i < NREW; i++) { r[CR_QPOS + i] = (float)q[(size_t)f * NQ + T.rew_q[i]]; r[CR_QVEL + i] = (float)v[(size_t)f * NV + T.rew_v[i]]; }
    for (int i = 0; i < 4; i++) r[CR_ROOTQ + i] = (float)q[(size_t)f * NQ + 3 + i];
    r[CR_ROOTV] = (float)v[(size_t)f * NV]; r[CR_ROOTV + 1] = (float)v[(size_t)f * NV + 1];
    for (int e4 = 0; e4 < 4; e4++)
      for (int i = 0; i < 3; i++) r[CR_EE + 3 * e4 + i] = (float)gx[((size_t)f * NG + T.ee_geom[e4]) * 3 + i];
    for (int i = 0; i < NQ; i++) reset[(size_t)f * RESET_ROW + RR_QPOS + i] = (float)q[(size_t)f * NQ + i];
    for (int i = 0; i < NV; i++) reset[(size_t)f * RESET_ROW + RR_QVEL + i] = (float)v[(size_t)f * NV + i];
    double c[3];
    dm_mass_centre(T.b_mass, NB, bx + (size_t)f * NB * 3, c);
    for (int i = 0; i < 3; i++) com[(size_t)f * COM_ROW + i] = (float)c[i];
  }
}
