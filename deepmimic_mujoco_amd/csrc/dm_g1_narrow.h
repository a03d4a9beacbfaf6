// dm_g1_narrow.h — collision stage: broadphase filters and the fp64, wave-uniform narrowphase of one staged geom pair (analytic
// routines, MPR with the clustered hull support mapping).  Both pipelines stage a pair and call narrow_pair.
#pragma once
#include "dm_g1_device.h"
#include "dm_g1_math.h"

namespace g1 {

// ------------------------------------------------------------------------------------------ narrowphase (fp64, wave-uniform)
// one contact of the pair being processed, and the view of one of its two geoms — both live in LDS (Lds::rc, Lds::geo):
// the narrowphase is wave-uniform scalar code, and per-lane copies of these would sit in scratch memory
struct Con { double dist, pos[3], n[3]; };
struct Geo {
  int type, nvert, nclus;
  const double *pos, *mat, *size, *center;   // into Lds::geo
  const double *vert, *clus;                 // global: clustered hull vertices, cluster bounds
  const int32_t *oidx;
};

// ---- support mapping of a hull (see mesh_support_pair below)
// Support ties (oracle/dm_convex.h "ties"): MPR queries a hull along its portal normal, in which two hull vertices tie EXACTLY by
// construction at every edge-edge / face-vertex contact; "first strict maximum" is then decided by the last bit of two dot
// products and ends in a different contact normal.  Rule (both sides): values within SUP_TIE of the maximum are tied, the
// lowest ORIGINAL vertex index wins.  A lane keeps its best value and the lowest-index vertex within SUP_TIE of it.
constexpr double SUP_TIE = 1e-12;
struct MeshPick { double best, cv, x, y, z; int bo, bk; };   // best value | candidate: value, vertex, original index, slot
// every lane scans vertex `lane` of up to four clusters of hull A and four of hull B (-1: none): sixteen independent loads in
// one round trip, no cross-lane step; the pick keeps the vertex itself, so no fetch follows the reduction
struct Scan4 { double x[4], y[4], z[4]; int o[4]; };
__device__ __forceinline__ void scan4_load(const Geo &g, const int (&c)[4], Scan4 &v, const int lane) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int k = 64 * (c[q] < 0 ? 0 : c[q]) + lane;
    const bool ok = c[q] >= 0;
    v.x[q] = ok ? g.vert[3 * k] : 0.0; v.y[q] = ok ? g.vert[3 * k + 1] : 0.0; v.z[q] = ok ? g.vert[3 * k + 2] : 0.0;
    v.o[q] = ok ? g.oidx[k] : 0x7fffffff;
  }
}
__device__ __forceinline__ void scan4_pick(const double *dl, const int (&c)[4], const Scan4 &v, MeshPick &p, const int lane) {
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (v.o[q] != 0x7fffffff) {
      const double sv = v.x[q] * dl[0] + v.y[q] * dl[1] + v.z[q] * dl[2];
      const bool up = sv > p.best;
      // new candidate: a new best whose window the old candidate left (or that has the lower index), or a lower index inside the window
      if (up ? (!(p.cv >= sv - SUP_TIE) || v.o[q] < p.bo) : (sv >= p.best - SUP_TIE && v.o[q] < p.bo)) {
        p.cv = sv; p.bo = v.o[q]; p.bk = 64 * c[q] + lane;
        p.x = v.x[q]; p.y = v.y[q]; p.z = v.z[q];
      }
      if (up) p.best = sv;
    }
}
// the lanes' picks -> the wave's pick: the maximum value, and among equal values the lowest original index (one lane in all
// but degenerate cases: a ballot and v_readlanes; ties walk the tied lanes)
__device__ __forceinline__ void wave_pick(MeshPick &p) {
  const double vmax = wmax_f64(p.best);
  unsigned long long eq = __ballot(p.cv >= vmax - SUP_TIE);   // never empty: the lane that holds the maximum has best - SUP_TIE <= cv <= best
  int l = __ffsll((long long)eq) - 1;
  int bo = __builtin_amdgcn_readlane(p.bo, l);
  eq &= eq - 1;
  while (eq) {
    const int l2 = __ffsll((long long)eq) - 1;
    eq &= eq - 1;
    const int o2 = __builtin_amdgcn_readlane(p.bo, l2);
    if (o2 < bo) { bo = o2; l = l2; }
  }
  p.best = vmax; p.bo = bo; p.bk = __builtin_amdgcn_readlane(p.bk, l);
  p.x = readlane_f64(p.x, l); p.y = readlane_f64(p.y, l); p.z = readlane_f64(p.z, l);
}
// the next (up to) four candidate clusters of a hull: bit sets of clusters lane + 64 m, consumed in ascending order
__device__ __forceinline__ bool next4(unsigned long long (&todo)[NCH], int (&c)[4]) {
  bool any = false;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    c[q] = -1;
#pragma unroll
    for (int m = 0; m < NCH; m++)
      if (c[q] < 0 && todo[m]) { c[q] = __ffsll((long long)todo[m]) - 1 + 64 * m; todo[m] &= todo[m] - 1; any = true; }
  }
  return any;
}
// cluster spheres of one hull for clusters lane + 64 m (loads only), then bounds ub[m] and the cluster with the largest centre . d
struct ClusLoad { double c[NCH][7]; };   // centre 3 | sphere radius | half extents of the box about the centre 3
__device__ __forceinline__ void cluster_load(const Geo &g, const bool on, ClusLoad &L, const int lane) {
#pragma unroll
  for (int m = 0; m < NCH; m++) {
    const int c = lane + 64 * m;
    const bool ok = on && c < g.nclus;
    const double *cl = g.clus + 8 * (ok ? c : 0);
#pragma unroll
    for (int i = 0; i < 7; i++) L.c[m][i] = ok ? cl[i] : 0.0;
  }
}
__device__ __forceinline__ void cluster_bounds(const Geo &g, const double *dl, const bool on, const ClusLoad &L, double (&ub)[NCH], int &top,
                                               const int lane) {
  if (!on) { for (int m = 0; m < NCH; m++) ub[m] = -1e300; top = 0; return; }   // (wave-uniform) not a mesh: nothing to reduce
  const double dn = sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
  double best = -1e300;
  top = 0x7fffffff;
#pragma unroll
  for (int m = 0; m < NCH; m++) {
    const int c = lane + 64 * m;
    ub[m] = -1e300;
    if (on && c < g.nclus) {
      const double dc = L.c[m][0] * dl[0] + L.c[m][1] * dl[1] + L.c[m][2] * dl[2];
      // the tighter of two bounds: the enclosing sphere, and the box about the same centre (flat patches of the hull surface)
      ub[m] = dc + fmin(L.c[m][3] * dn, L.c[m][4] * fabs(dl[0]) + L.c[m][5] * fabs(dl[1]) + L.c[m][6] * fabs(dl[2]));
      if (dc > best) { best = dc; top = c; }
    }
  }
  const double vmax = wmax_f64(best);
  unsigned long long eq = __ballot(best == vmax);
  int l = __ffsll((long long)eq) - 1, t = __builtin_amdgcn_readlane(top, l);
  eq &= eq - 1;
  while (eq) {
    l = __ffsll((long long)eq) - 1;
    eq &= eq - 1;
    const int t2 = __builtin_amdgcn_readlane(top, l);
    if (t2 < t) t = t2;
  }
  top = t;
}
// Support vertices of up to two hulls at once, in local directions dlA / dlB.  The vertices are stored in compact clusters
// (k-d leaves, padded to 64 slots) with a bounding sphere and box each.  Three dependent memory round trips for BOTH hulls together
// (the narrowphase is one wave's latency chain: round trips are what it costs; every load of a round is requested before the
// first reduction of that round): (1) every cluster's centre . d and bound centre . d + min(radius |d|, box term); (2) the cluster with
// the largest centre . d is scanned: a true support value to prune with; (3) the clusters whose bound still reaches it are
// scanned, four per trip, every lane keeping its own best and the vertex it belongs to, one wave reduction at the
// end.  Exact; equal support values resolve to the lowest ORIGINAL vertex index, like a serial first-maximum scan.
__device__ __forceinline__ void mesh_support_pair(const Geo &A, const double *dlA, const bool meshA, MeshPick &pa, const Geo &B,
                                                  const double *dlB, const bool meshB, MeshPick &pb, const int lane) {
  double ubA[NCH], ubB[NCH];
  int topA, topB;
  { ClusLoad LA, LB;
    cluster_load(A, meshA, LA, lane);
    cluster_load(B, meshB, LB, lane);
    cluster_bounds(A, dlA, meshA, LA, ubA, topA, lane);
    cluster_bounds(B, dlB, meshB, LB, ubB, topB, lane); }
  pa = {-1e300, -1e300, 0.0, 0.0, 0.0, 0x7fffffff, 0};
  pb = pa;
  { const int ca[4] = {meshA ? topA : -1, -1, -1, -1}, cb[4] = {meshB ? topB : -1, -1, -1, -1};
    Scan4 va, vb;
    scan4_load(A, ca, va, lane);
    scan4_load(B, cb, vb, lane);
    scan4_pick(dlA, ca, va, pa, lane);
    scan4_pick(dlB, cb, vb, pb, lane); }
  const double ba = meshA ? wmax_f64(pa.best) : 0.0, bb = meshB ? wmax_f64(pb.best) : 0.0;
  unsigned long long todoA[NCH], todoB[NCH];
#pragma unroll
  for (int m = 0; m < NCH; m++) {
    todoA[m] = meshA ? __ballot(ubA[m] >= ba - SUP_TIE && (lane + 64 * m) != topA) : 0ull;
    todoB[m] = meshB ? __ballot(ubB[m] >= bb - SUP_TIE && (lane + 64 * m) != topB) : 0ull;
  }
  // (both hulls' candidates in ONE loop — eight clusters per trip — measured slower: 34 more live doubles spill)
  for (;;) {
    int ca[4];
    if (!next4(todoA, ca)) break;
    Scan4 va;
    scan4_load(A, ca, va, lane);
    scan4_pick(dlA, ca, va, pa, lane);
  }
  for (;;) {
    int cb[4];
    if (!next4(todoB, cb)) break;
    Scan4 vb;
    scan4_load(B, cb, vb, lane);
    scan4_pick(dlB, cb, vb, pb, lane);
  }
  if (meshA) wave_pick(pa);
  if (meshB) wave_pick(pb);
}
// slot of the support vertex in the clustered array, and the vertex itself
__device__ __forceinline__ int mesh_support_index(const Geo &g, const double *dl, double *v, const int lane) {
  MeshPick i, j;
  mesh_support_pair(g, dl, true, i, g, dl, false, j, lane);
  v[0] = i.x; v[1] = i.y; v[2] = i.z;
  return i.bk;
}

// [EXT] mjccd_support for the analytic shapes (local direction dl -> local point p)
__device__ __forceinline__ void support_local(const Geo &g, const double *dl, double *p) {
  p[0] = p[1] = p[2] = 0;
  if (g.type == DM_GEOM_SPHERE) {
    const double n = dnorm(dl);
    if (n > 0) for (int i = 0; i < 3; i++) p[i] = dl[i] * g.size[0] / n;
  } else if (g.type == DM_GEOM_CYLINDER) {
    const double n = sqrt(dl[0] * dl[0] + dl[1] * dl[1]);
    if (n > MINVAL) { p[0] = dl[0] * g.size[0] / n; p[1] = dl[1] * g.size[0] / n; }
    p[2] = dl[2] * g.size[1] >= -0.5 * SUP_TIE ? g.size[1] : -g.size[1];
  } else if (g.type == DM_GEOM_BOX) {
    for (int i = 0; i < 3; i++) p[i] = dl[i] * g.size[i] >= -0.5 * SUP_TIE ? g.size[i] : -g.size[i];
  }
}

// ---- libccd MPR (ccdMPRPenetration), restated; tolerance / iteration cap = MuJoCo's mpr_tolerance / mpr_iterations
#define CCD_EPS 2.220446049250313e-16
#define MPR_TOL 1e-6
#define MPR_ITER 50
struct Sup { double v[3], v1[3], v2[3]; };
__device__ __forceinline__ bool ccd_zero(double x) { return fabs(x) < CCD_EPS; }
__device__ __forceinline__ bool ccd_eq(double a, double b) {
  double ab = fabs(a - b);
  if (ab < CCD_EPS) return true;
  a = fabs(a); b = fabs(b);
  return b > a ? ab < CCD_EPS * b : ab < CCD_EPS * a;
}
// support point of A - B in direction dir: both supports together, so the two hull scans share their memory round trips
__device__ __forceinline__ void mpr_support(const Geo &a, const Geo &b, const double *dir, Sup &s, const int lane) {
  double nd[3] = {-dir[0], -dir[1], -dir[2]}, dla[3], dlb[3], pa[3], pb[3];
  drot_t(dla, a.mat, dir);
  drot_t(dlb, b.mat, nd);
  const bool ma = a.type == DM_GEOM_MESH, mb = b.type == DM_GEOM_MESH;

  support_local(a, dla, pa);
  support_local(b, dlb, pb);
  if (ma || mb) {
    MeshPick ka, kb;
#ifdef G1_PROFILE
    const long long t0_ = clock64();
#endif
    mesh_support_pair(a, dla, ma, ka, b, dlb, mb, kb, lane);
#ifdef G1_PROFILE
    if (lane == 0) { S.prof[13] += (unsigned)(clock64() - t0_); S.prof[12] += 1; }
#endif
    if (ma) { pa[0] = ka.x; pa[1] = ka.y; pa[2] = ka.z; }
    if (mb) { pb[0] = kb.x; pb[1] = kb.y; pb[2] = kb.z; }
  }
  drot(s.v1, a.mat, pa);
  drot(s.v2, b.mat, pb);
  for (int i = 0; i < 3; i++) { s.v1[i] += a.pos[i]; s.v2[i] += b.pos[i]; s.v[i] = s.v1[i] - s.v2[i]; }
}
__device__ __forceinline__ void portal_dir(const Sup *ps, double *dir) {
  double a[3], b[3];
  dsub(a, ps[2].v, ps[1].v);
  dsub(b, ps[3].v, ps[1].v);
  dcross(dir, a, b);
  dnormalize(dir);
}
__device__ __forceinline__ bool reach_tol(const Sup *ps, const Sup &v4, const double *dir) {
  const double dv4 = ddot(v4.v, dir);
  double m = fmin(fmin(dv4 - ddot(ps[1].v, dir), dv4 - ddot(ps[2].v, dir)), dv4 - ddot(ps[3].v, dir));
  return ccd_eq(m, MPR_TOL) || m < MPR_TOL;
}
__device__ __forceinline__ void expand_portal(Sup *ps, const Sup &v4) {
  double c[3];
  dcross(c, v4.v, ps[0].v);
  if (ddot(ps[1].v, c) > 0) { if (ddot(ps[2].v, c) > 0) ps[1] = v4; else ps[3] = v4; }
  else { if (ddot(ps[3].v, c) > 0) ps[2] = v4; else ps[1] = v4; }
}
__device__ __forceinline__ double tri_closest_origin(const double *a, const double *b, const double *c, double *w) {
  double ab[3], ac[3], ap[3] = {-a[0], -a[1], -a[2]};
  dsub(ab, b, a); dsub(ac, c, a);
  const double d1 = ddot(ab, ap), d2 = ddot(ac, ap);
  if (d1 <= 0 && d2 <= 0) { for (int i = 0; i < 3; i++) w[i] = a[i]; return ddot(w, w); }
  double bp[3] = {-b[0], -b[1], -b[2]};
  const double d3 = ddot(ab, bp), d4 = ddot(ac, bp);
  if (d3 >= 0 && d4 <= d3) { for (int i = 0; i < 3; i++) w[i] = b[i]; return ddot(w, w); }
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0 && d1 >= 0 && d3 <= 0) {
    const double v = d1 / (d1 - d3);
    for (int i = 0; i < 3; i++) w[i] = a[i] + v * ab[i];
    return ddot(w, w);
  }
  double cp[3] = {-c[0], -c[1], -c[2]};
  const double d5 = ddot(ab, cp), d6 = ddot(ac, cp);
  if (d6 >= 0 && d5 <= d6) { for (int i = 0; i < 3; i++) w[i] = c[i]; return ddot(w, w); }
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0 && d2 >= 0 && d6 <= 0) {
    const double v = d2 / (d2 - d6);
    for (int i = 0; i < 3; i++) w[i] = a[i] + v * ac[i];
    return ddot(w, w);
  }
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
    const double v = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    for (int i = 0; i < 3; i++) w[i] = b[i] + v * (c[i] - b[i]);
    return ddot(w, w);
  }
  const double den = 1.0 / (va + vb + vc), v = vb * den, u = vc * den;
  for (int i = 0; i < 3; i++) w[i] = a[i] + ab[i] * v + ac[i] * u;
  return ddot(w, w);
}
// 0 = penetration (depth, dir a -> b, pos), -1 = none
// The routine is a state machine around ONE support evaluation site (discoverPortal's vertices 1, 2, 3.., refinePortal,
// findPenetr): the support mapping of two hulls is the bulk of the code, and one inlined copy costs neither the code size
// of five nor a function call (whose callee-saved registers would go through scratch memory a hundred times per env-step).
// The arithmetic and its order are those of the straight-line libccd routine.
// `hint` (or null): a direction that separated the pair at an earlier evaluation — tested first with one support evaluation;
// returns -2 if it still separates them (disjoint shapes: MPR would find no contact either, so the shortcut is result-neutral).
// On a `no intersection` verdict reached through a strictly negative support projection, `sep` receives that direction.
__device__ __forceinline__ int mpr_penetration(const Geo &a, const Geo &b, double *depth, double *dir, double *pos, const double *hint,
                                               double *sep, bool &sep_valid, Sup *ps, const int lane) {
  enum { V1, V2, DISCOVER, REFINE, PENETR, HINT };
  constexpr double SEP_EPS = 1e-9;
  sep_valid = false;
  // ps: the portal (v0..v3: v, v1, v2), wave-uniform state in LDS (every lane writes the same values; 72 VGPRs if kept per lane)
  Sup sv;
  double d[3], va[3], vb[3], dot;
  for (int i = 0; i < 3; i++) { ps[0].v1[i] = a.center[i]; ps[0].v2[i] = b.center[i]; ps[0].v[i] = a.center[i] - b.center[i]; }
  if (ccd_zero(ps[0].v[0]) && ccd_zero(ps[0].v[1]) && ccd_zero(ps[0].v[2])) ps[0].v[0] += CCD_EPS * 10;
  for (int i = 0; i < 3; i++) d[i] = -ps[0].v[i];
  dnormalize(d);
  int state = V1, guard = 0, it = 0;
  if (hint) { state = HINT; for (int i = 0; i < 3; i++) d[i] = hint[i]; }
#define MPR_MISS(DOT) do { if ((DOT) < -SEP_EPS) { sep[0] = d[0]; sep[1] = d[1]; sep[2] = d[2]; sep_valid = true; } return -1; } while (0)
  for (;;) {
    mpr_support(a, b, d, sv, lane);
    if (state == HINT) {
      if (ddot(sv.v, d) < -SEP_EPS) return -2;
      for (int i = 0; i < 3; i++) d[i] = -ps[0].v[i];   // the hint went stale: the routine proper
      dnormalize(d);
      state = V1;
    } else if (state == V1) {
      ps[1] = sv;
      dot = ddot(ps[1].v, d);
      if (ccd_zero(dot) || dot < 0) MPR_MISS(dot);
      dcross(d, ps[0].v, ps[1].v);
      if (ccd_zero(ddot(d, d))) {
        for (int i = 0; i < 3; i++) pos[i] = 0.5 * (ps[1].v1[i] + ps[1].v2[i]);
        if (ccd_zero(ps[1].v[0]) && ccd_zero(ps[1].v[1]) && ccd_zero(ps[1].v[2])) { *depth = 0; dir[0] = dir[1] = dir[2] = 0; return 0; }
        for (int i = 0; i < 3; i++) dir[i] = ps[1].v[i];
        *depth = dnormalize(dir);
        return 0;
      }
      dnormalize(d);
      state = V2;
    } else if (state == V2) {
      ps[2] = sv;
      dot = ddot(ps[2].v, d);
      if (ccd_zero(dot) || dot < 0) MPR_MISS(dot);
      dsub(va, ps[1].v, ps[0].v); dsub(vb, ps[2].v, ps[0].v);
      dcross(d, va, vb);
      dnormalize(d);
      if (ddot(d, ps[0].v) > 0) { Sup t = ps[1]; ps[1] = ps[2]; ps[2] = t; for (int i = 0; i < 3; i++) d[i] = -d[i]; }
      state = DISCOVER;
      guard = 0;
    } else if (state == DISCOVER) {
      if (guard > 1000) return -1;
      guard++;
      ps[3] = sv;
      dot = ddot(ps[3].v, d);
      if (ccd_zero(dot) || dot < 0) MPR_MISS(dot);
      bool cont = false;
      dcross(va, ps[1].v, ps[3].v);
      dot = ddot(va, ps[0].v);
      if (dot < 0 && !ccd_zero(dot)) { ps[2] = ps[3]; cont = true; }
      if (!cont) {
        dcross(va, ps[3].v, ps[2].v);
        dot = ddot(va, ps[0].v);
        if (dot < 0 && !ccd_zero(dot)) { ps[1] = ps[3]; cont = true; }
      }
      if (cont) {
        dsub(va, ps[1].v, ps[0].v); dsub(vb, ps[2].v, ps[0].v);
        dcross(d, va, vb);
        dnormalize(d);
      } else {   // portal found: refinePortal's first test, or straight on to findPenetr (same portal direction)
        portal_dir(ps, d);
        dot = ddot(d, ps[1].v);
        state = (ccd_zero(dot) || dot > 0) ? PENETR : REFINE;
        guard = 0;
      }
    } else if (state == REFINE) {
      dot = ddot(sv.v, d);
      if (!(ccd_zero(dot) || dot > 0)) MPR_MISS(dot);
      if (reach_tol(ps, sv, d)) return -1;
      expand_portal(ps, sv);
      if (++guard >= 10000) return -1;
      portal_dir(ps, d);
      dot = ddot(d, ps[1].v);
      if (ccd_zero(dot) || dot > 0) state = PENETR;
    } else {   // findPenetr
      if (reach_tol(ps, sv, d) || it > MPR_ITER) {
        *depth = sqrt(tri_closest_origin(ps[1].v, ps[2].v, ps[3].v, dir));
        if (ccd_zero(*depth)) dir[0] = dir[1] = dir[2] = 0; else dnormalize(dir);
        double bb[4], t[3], sum;
        portal_dir(ps, d);
        dcross(t, ps[1].v, ps[2].v); bb[0] = ddot(t, ps[3].v);
        dcross(t, ps[3].v, ps[2].v); bb[1] = ddot(t, ps[0].v);
        dcross(t, ps[0].v, ps[1].v); bb[2] = ddot(t, ps[3].v);
        dcross(t, ps[2].v, ps[1].v); bb[3] = ddot(t, ps[0].v);
        sum = bb[0] + bb[1] + bb[2] + bb[3];
        if (ccd_zero(sum) || sum < 0) {
          bb[0] = 0;
          dcross(t, ps[2].v, ps[3].v); bb[1] = ddot(t, d);
          dcross(t, ps[3].v, ps[1].v); bb[2] = ddot(t, d);
          dcross(t, ps[1].v, ps[2].v); bb[3] = ddot(t, d);
          sum = bb[1] + bb[2] + bb[3];
        }
        const double inv = 1.0 / sum;
        double p1[3] = {0, 0, 0}, p2[3] = {0, 0, 0};
        for (int k = 0; k < 4; k++)
          for (int i = 0; i < 3; i++) { p1[i] += bb[k] * ps[k].v1[i]; p2[i] += bb[k] * ps[k].v2[i]; }
        for (int i = 0; i < 3; i++) pos[i] = 0.5 * inv * (p1[i] + p2[i]);
        return 0;
      }
      expand_portal(ps, sv);
      it++;
      portal_dir(ps, d);
    }
  }
#undef MPR_MISS
}

// [EXT] mjc_Convex at margin 0; spheres get their analytic normal afterwards (mjc_fixNormal)
// Separating-direction cache (per env, in global memory): pairs that passed the box filter but do not touch — adjacent links,
// typically — keep the direction that proved it, stored in geom 1's frame; the next evaluation re-tests it with ONE support
// evaluation instead of running the portal search (4..5 on average).  Entries: pair id, direction xyz; slot SEPC = next victim.
constexpr int SEPC = 16;
// `direct`: cache points at the ONE entry of this (env, pair) — the pair kernel's waves own a pair each, a shared 16-entry set would race.
__device__ __forceinline__ int np_convex(Con *c, const Geo &a, const Geo &b, float *cache, const bool direct, const int pair, Sup *ps,
                                         const int lane) {
  double depth, dir[3], pos[3], hint[3], sep[3];
  bool sep_valid;
  int slot = -1;
  if (cache) {
    const unsigned long long hit = direct ? (__float_as_int(cache[0]) == pair ? 1ull : 0ull)
                                          : __ballot(lane < SEPC && __float_as_int(cache[4 * (lane < SEPC ? lane : 0)]) == pair);
    if (hit) {
      slot = __ffsll((long long)hit) - 1;
      const double hl[3] = {cache[4 * slot + 1], cache[4 * slot + 2], cache[4 * slot + 3]};
      drot(hint, a.mat, hl);
      dnormalize(hint);
    }
  }
  const int res = mpr_penetration(a, b, &depth, dir, pos, slot >= 0 ? hint : nullptr, sep, sep_valid, ps, lane);
  if (cache && res == -1 && sep_valid) {   // remember what separated them (geom 1's frame)
    if (slot < 0) {
      if (direct) slot = 0;
      else { slot = __float_as_int(cache[4 * SEPC]) & (SEPC - 1); if (lane == 0) cache[4 * SEPC] = __int_as_float(slot + 1); }
    }
    double sl[3];
    drot_t(sl, a.mat, sep);
    if (lane == 0) { cache[4 * slot] = __int_as_float(pair); cache[4 * slot + 1] = (float)sl[0]; cache[4 * slot + 2] = (float)sl[1]; cache[4 * slot + 3] = (float)sl[2]; }
  } else if (cache && res == 0 && slot >= 0) {
    if (lane == 0) cache[4 * slot] = __int_as_float(-1);   // they touch now: drop the entry
  }
  if (res != 0) return 0;
  if (dir[0] == 0 && dir[1] == 0 && dir[2] == 0) return 0;
  c->dist = -depth;
  for (int i = 0; i < 3; i++) { c->pos[i] = pos[i]; c->n[i] = dir[i]; }
  double n1[3], n2[3];
  bool h1 = false, h2 = false;
  if (a.type == DM_GEOM_SPHERE) { dsub(n1, pos, a.pos); h1 = dnormalize(n1) > MINVAL; }
  if (b.type == DM_GEOM_SPHERE) { dsub(n2, b.pos, pos); h2 = dnormalize(n2) > MINVAL; }
  if (h1 && h2) { for (int i = 0; i < 3; i++) c->n[i] = n1[i] + n2[i]; dnormalize(c->n); }
  else if (h1) for (int i = 0; i < 3; i++) c->n[i] = n1[i];
  else if (h2) for (int i = 0; i < 3; i++) c->n[i] = n2[i];
  return 1;
}

__device__ __forceinline__ int np_plane_sphere(Con *c, const Geo &p, const double *spos, double r) {
  double n[3] = {p.mat[2], p.mat[5], p.mat[8]}, df[3];
  dsub(df, spos, p.pos);
  const double dist = ddot(df, n) - r;
  if (dist > 0) return 0;
  c->dist = dist;
  for (int i = 0; i < 3; i++) { c->n[i] = n[i]; c->pos[i] = spos[i] - n[i] * (r + 0.5 * dist); }
  return 1;
}
__device__ __forceinline__ int np_plane_box(Con *c, const Geo &p, const Geo &b) {
  double n[3] = {p.mat[2], p.mat[5], p.mat[8]}, df[3];
  dsub(df, b.pos, p.pos);
  const double dist = ddot(df, n);
  int cnt = 0;
  for (int i = 0; i < 8; i++) {
    double v[3] = {b.size[0] * ((i & 1) ? 1 : -1), b.size[1] * ((i & 2) ? 1 : -1), b.size[2] * ((i & 4) ? 1 : -1)}, corner[3];
    drot(corner, b.mat, v);
    const double ld = ddot(n, corner);
    if (dist + ld > 0 || ld > 0) continue;
    c[cnt].dist = dist + ld;
    for (int k = 0; k < 3; k++) { c[cnt].n[k] = n[k]; c[cnt].pos[k] = corner[k] + b.pos[k] - n[k] * 0.5 * c[cnt].dist; }
    if (++cnt >= 4) return 4;
  }
  return cnt;
}
__device__ __forceinline__ int np_plane_cylinder(Con *c, const Geo &p, const Geo &cy) {   // [EXT] mjc_PlaneCylinder
  double normal[3] = {p.mat[2], p.mat[5], p.mat[8]}, axis[3] = {cy.mat[2], cy.mat[5], cy.mat[8]};
  double prjaxis = ddot(normal, axis);
  if (prjaxis > 0) { for (int i = 0; i < 3; i++) axis[i] = -axis[i]; prjaxis = -prjaxis; }
  double dif[3], vec[3];
  dsub(dif, cy.pos, p.pos);
  const double dist0 = ddot(dif, normal);
  for (int i = 0; i < 3; i++) vec[i] = axis[i] * prjaxis - normal[i];
  const double len2 = ddot(vec, vec);
  if (len2 >= MINVAL * MINVAL) { const double s = cy.size[0] / sqrt(len2); for (int i = 0; i < 3; i++) vec[i] *= s; }
  else for (int i = 0; i < 3; i++) vec[i] = cy.mat[3 * i] * cy.size[0];
  const double prjvec = ddot(vec, normal);
  for (int i = 0; i < 3; i++) axis[i] *= cy.size[1];
  prjaxis *= cy.size[1];
  int n = 0;
  if (dist0 + prjaxis + prjvec > 0) return 0;
  { const double dd = dist0 + prjaxis + prjvec; c[n].dist = dd;
    for (int i = 0; i < 3; i++) { c[n].pos[i] = cy.pos[i] + vec[i] + axis[i] - normal[i] * dd * 0.5; c[n].n[i] = normal[i]; } n++; }
  if (dist0 - prjaxis + prjvec <= 0) {
    const double dd = dist0 - prjaxis + prjvec; c[n].dist = dd;
    for (int i = 0; i < 3; i++) { c[n].pos[i] = cy.pos[i] + vec[i] - axis[i] - normal[i] * dd * 0.5; c[n].n[i] = normal[i]; } n++;
  }
  const double prjvec1 = -0.5 * prjvec;
  if (dist0 + prjaxis + prjvec1 <= 0) {
    double vec1[3];
    dcross(vec1, vec, axis);
    dnormalize(vec1);
    for (int i = 0; i < 3; i++) vec1[i] *= cy.size[0] * sqrt(3.0) * 0.5;
    const double dd = dist0 + prjaxis + prjvec1;
    for (int sg = 1; sg >= -1; sg -= 2) {
      c[n].dist = dd;
      for (int i = 0; i < 3; i++) { c[n].pos[i] = cy.pos[i] + sg * vec1[i] + axis[i] - 0.5 * vec[i] - normal[i] * dd * 0.5; c[n].n[i] = normal[i]; }
      n++;
    }
  }
  return n;
}
// [EXT] mjc_PlaneConvex for a mesh: support vertex towards the plane + three directions tilted by 0.3 (low-confidence
// restatement of the multi-contact rule, identical to the oracle's)
__device__ __forceinline__ int np_plane_mesh_body(Con *c, const Geo &p, const Geo &g, const int lane) {
  double normal[3] = {p.mat[2], p.mat[5], p.mat[8]}, t1[3] = {p.mat[0], p.mat[3], p.mat[6]}, t2[3] = {p.mat[1], p.mat[4], p.mat[7]};
  int used[4], n = 0;
  for (int k = 0; k < 4; k++) {
    double dw[3], dl[3];
    if (k == 0) for (int i = 0; i < 3; i++) dw[i] = -normal[i];
    else {
      const double ang = 2.0 * 3.14159265358979323846 * (k - 1) / 3.0, ca = 0.3 * cos(ang), sa = 0.3 * sin(ang);
      for (int i = 0; i < 3; i++) dw[i] = -normal[i] + ca * t1[i] + sa * t2[i];
    }
    drot_t(dl, g.mat, dw);
    double vl[3];
    const int vi = mesh_support_index(g, dl, vl, lane);
    bool dup = false;
    for (int j = 0; j < n; j++) dup |= used[j] == vi;
    if (dup) continue;
    double v[3], dif[3];
    drot(v, g.mat, vl);
    for (int i = 0; i < 3; i++) v[i] += g.pos[i];
    dsub(dif, v, p.pos);
    const double dist = ddot(dif, normal);
    if (dist > 0) { if (k == 0) return 0; continue; }
    used[n] = vi;
    c[n].dist = dist;
    for (int i = 0; i < 3; i++) { c[n].pos[i] = v[i] - 0.5 * dist * normal[i]; c[n].n[i] = normal[i]; }
    n++;
  }
  return n;
}
__device__ __forceinline__ int np_sphere_sphere(Con *c, const double *p1, double r1, const double *p2, double r2) {
  double df[3];
  dsub(df, p2, p1);
  const double cd = dnorm(df), dist = cd - r1 - r2;
  if (dist > 0) return 0;
  c->dist = dist;
  if (cd < MINVAL) { c->n[0] = 1; c->n[1] = c->n[2] = 0; }
  else for (int i = 0; i < 3; i++) c->n[i] = df[i] / cd;
  for (int i = 0; i < 3; i++) c->pos[i] = p1[i] + c->n[i] * (r1 + 0.5 * dist);
  return 1;
}
__device__ __forceinline__ int np_sphere_box(Con *c, const Geo &s, const Geo &b) {
  double t[3], ctr[3], cl[3], nl[3];
  const double r = s.size[0];
  dsub(t, s.pos, b.pos);
  drot_t(ctr, b.mat, t);
  for (int i = 0; i < 3; i++) { cl[i] = dclamp(ctr[i], -b.size[i], b.size[i]); nl[i] = cl[i] - ctr[i]; }
  const double dd = dnorm(nl);
  double dist, pl[3];
  if (dd - r > 0) return 0;
  if (dd <= MINVAL) {
    double closest = 2 * (b.size[0] + b.size[1] + b.size[2]);
    int k = 0;
    for (int i = 0; i < 6; i++) {
      const double test = b.size[i / 2] - ((i % 2) ? -1.0 : 1.0) * ctr[i / 2];
      if (test < closest) { closest = test; k = i; }
    }
    nl[0] = nl[1] = nl[2] = 0;
    nl[k / 2] = (k % 2) ? 1.0 : -1.0;
    dist = -closest - r;
  } else {
    for (int i = 0; i < 3; i++) nl[i] /= dd;
    dist = dd - r;
  }
  for (int i = 0; i < 3; i++) pl[i] = ctr[i] + nl[i] * (r + 0.5 * dist);
  c->dist = dist;
  drot(c->n, b.mat, nl);
  drot(t, b.mat, pl);
  for (int i = 0; i < 3; i++) c->pos[i] = t[i] + b.pos[i];
  return 1;
}
// box-box (SAT + face clipping), same construction as the humanoid3d path (own construction, not MuJoCo's code)
__device__ __forceinline__ int np_box_box_body(Con *c, const Geo &A, const Geo &Bx, double (*poly)[3], double (*tmp)[3]) {
  const double *p1 = A.pos, *R1 = A.mat, *s1 = A.size, *p2 = Bx.pos, *R2 = Bx.mat, *s2 = Bx.size;
  double R[9], AR[9], t[3], tw[3];
  dsub(tw, p2, p1);
  drot_t(t, R1, tw);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      R[3 * i + j] = R1[i] * R2[j] + R1[3 + i] * R2[3 + j] + R1[6 + i] * R2[6 + j];
      AR[3 * i + j] = fabs(R[3 * i + j]) + 1e-9;
    }
  double best = -1e30, bn[3] = {0, 0, 0};
  int code = -1;
  for (int i = 0; i < 3; i++) {
    const double s = fabs(t[i]) - (s1[i] + s2[0] * AR[3 * i] + s2[1] * AR[3 * i + 1] + s2[2] * AR[3 * i + 2]);
    if (s > 0) return 0;
    if (s > best) { best = s; code = i; }
  }
  for (int j = 0; j < 3; j++) {
    const double tj = t[0] * R[j] + t[1] * R[3 + j] + t[2] * R[6 + j];
    const double s = fabs(tj) - (s2[j] + s1[0] * AR[j] + s1[1] * AR[3 + j] + s1[2] * AR[6 + j]);
    if (s > 0) return 0;
    if (s > best) { best = s; code = 3 + j; }
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double ei[3] = {0, 0, 0}, ej[3] = {R[j], R[3 + j], R[6 + j]}, ax[3];
      ei[i] = 1;
      dcross(ax, ei, ej);
      const double l = dnorm(ax);
      if (l < 1e-6) continue;
      for (int k = 0; k < 3; k++) ax[k] /= l;
      double ra = 0, rb = 0;
      for (int k = 0; k < 3; k++) ra += s1[k] * fabs(ax[k]);
      for (int k = 0; k < 3; k++) { double ek[3] = {R[k], R[3 + k], R[6 + k]}; rb += s2[k] * fabs(ddot(ax, ek)); }
      const double s = fabs(ddot(t, ax)) - (ra + rb);
      if (s > 0) return 0;
      if (s > best + 0.05 * fabs(best) + 1e-6) { best = s; code = 6 + 3 * i + j; bn[0] = ax[0]; bn[1] = ax[1]; bn[2] = ax[2]; }
    }
  if (code < 0) return 0;
  if (code >= 6) {
    const int i = (code - 6) / 3, j = (code - 6) % 3;
    double n1[3] = {bn[0], bn[1], bn[2]};
    if (ddot(n1, t) < 0) for (int k = 0; k < 3; k++) n1[k] = -n1[k];
    double pa[3], pb[3];
    for (int k = 0; k < 3; k++) pa[k] = (k == i) ? 0 : ((n1[k] > 0) ? s1[k] : -s1[k]);
    for (int k = 0; k < 3; k++) pb[k] = t[k];
    for (int k = 0; k < 3; k++) {
      if (k == j) continue;
      double ek[3] = {R[k], R[3 + k], R[6 + k]};
      const double sg = (ddot(n1, ek) > 0) ? -s2[k] : s2[k];
      for (int q = 0; q < 3; q++) pb[q] += sg * ek[q];
    }
    double ua[3] = {0, 0, 0}, ub[3] = {R[j], R[3 + j], R[6 + j]}, w[3];
    ua[i] = 1;
    dsub(w, pb, pa);
    const double uaub = ddot(ua, ub), q1 = ddot(ua, w), q2 = -ddot(ub, w), dd = 1 - uaub * uaub;
    double alpha = 0, beta = 0;
    if (dd > 1e-12) { alpha = (q1 + uaub * q2) / dd; beta = (uaub * q1 + q2) / dd; }
    alpha = dclamp(alpha, -s1[i], s1[i]);
    beta = dclamp(beta, -s2[j], s2[j]);
    double mid[3], mw[3];
    for (int k = 0; k < 3; k++) mid[k] = 0.5 * ((pa[k] + ua[k] * alpha) + (pb[k] + ub[k] * beta));
    drot(mw, R1, mid);
    drot(c->n, R1, n1);
    for (int k = 0; k < 3; k++) c->pos[k] = mw[k] + p1[k];
    c->dist = best;
    return 1;
  }
  const double *Ra, *Rb, *sa, *sb, *pa, *pb;
  int ax, flip;
  if (code < 3) { Ra = R1; Rb = R2; sa = s1; sb = s2; pa = p1; pb = p2; ax = code; flip = 0; }
  else { Ra = R2; Rb = R1; sa = s2; sb = s1; pa = p2; pb = p1; ax = code - 3; flip = 1; }
  double nrm[3] = {Ra[ax], Ra[3 + ax], Ra[6 + ax]}, dab[3];
  dsub(dab, pb, pa);
  if (ddot(nrm, dab) < 0) for (int k = 0; k < 3; k++) nrm[k] = -nrm[k];
  int ib = 0;
  double bestd = -1, nb[3];
  drot_t(nb, Rb, nrm);
  for (int k = 0; k < 3; k++) if (fabs(nb[k]) > bestd) { bestd = fabs(nb[k]); ib = k; }
  const double sgn = (nb[ib] > 0) ? -1.0 : 1.0;
  const int u = (ib + 1) % 3, v = (ib + 2) % 3;
  int np = 4;
  for (int q = 0; q < 4; q++) {
    const double su = (q == 0 || q == 3) ? -sb[u] : sb[u], sv = (q < 2) ? -sb[v] : sb[v];
    double loc[3], w[3], rel[3];
    loc[ib] = sgn * sb[ib]; loc[u] = su; loc[v] = sv;
    drot(w, Rb, loc);
    for (int k = 0; k < 3; k++) rel[k] = w[k] + pb[k] - pa[k];
    drot_t(poly[q], Ra, rel);
  }
  const int axes[2] = {(ax + 1) % 3, (ax + 2) % 3};
  for (int e = 0; e < 2; e++)
    for (int sd = -1; sd <= 1; sd += 2) {
      const int a = axes[e];
      int nn = 0;
      for (int q = 0; q < np; q++) {
        const double *P = poly[q], *Q = poly[(q + 1) % np];
        const double dp = sd * P[a] - sa[a], dq = sd * Q[a] - sa[a];
        if (dp <= 0) { for (int k = 0; k < 3; k++) tmp[nn][k] = P[k]; nn++; }
        if ((dp < 0 && dq > 0) || (dp > 0 && dq < 0)) {
          const double f = dp / (dp - dq);
          for (int k = 0; k < 3; k++) tmp[nn][k] = P[k] + f * (Q[k] - P[k]);
          nn++;
        }
        if (nn >= 15) break;
      }
      np = nn;
      for (int q = 0; q < np; q++) for (int k = 0; k < 3; k++) poly[q][k] = tmp[q][k];
      if (np == 0) return 0;
    }
  double nl[3];
  drot_t(nl, Ra, nrm);
  int cnt = 0;
  for (int q = 0; q < np && cnt < 8; q++) {
    const double depth = ddot(nl, poly[q]) - sa[ax];
    if (depth > 0) continue;
    double pl[3], pw[3];
    for (int k = 0; k < 3; k++) pl[k] = poly[q][k] - nl[k] * 0.5 * depth;
    drot(pw, Ra, pl);
    for (int k = 0; k < 3; k++) { c[cnt].pos[k] = pw[k] + pa[k]; c[cnt].n[k] = flip ? -nrm[k] : nrm[k]; }
    c[cnt].dist = depth;
    cnt++;
  }
  while (cnt > 4) {
    int w = 0;
    for (int q = 1; q < cnt; q++) if (c[q].dist >= c[w].dist) w = q;
    for (int q = w; q < cnt - 1; q++) c[q] = c[q + 1];
    cnt--;
  }
  return cnt;
}

// Staging of the pair being processed (fp64, wave-uniform): the two geoms (pos 3 | mat 9 | size 3 | centre 3 each), its contacts,
// the box-box polygons and the MPR portal.  The monolithic kernel keeps it in LDS slack of the contact stage (S.u.co), the pair
// kernel of the split pipeline in a small LDS block of its own.
struct NpStage {
  double (*geo)[18];
  int32_t (*geoi)[6];     // type, nvert, nclus, vertex start, cluster start, pad
  Con *rc;
  double (*poly0)[3], (*poly1)[3];
  Sup *ps;
};
// entry l (0..17) of geom g's staged record: its pose in fp64 from the fp64 pose of its body (kinematics) and the fp64 tables
__device__ __forceinline__ double geo_entry(const Dev &T, const int g, const int l) {
  const int type = T.g_type[g], me = T.g_mesh[g], b = T.g_body[g];
  double bq[4], R[9], v;
  for (int i = 0; i < 4; i++) bq[i] = (double)S.xquat[b][i] + (double)S.xquat_lo[b][i];
  quat2mat(R, bq);
  if (l >= 12 && l < 15) v = T.g_size_d[g][l - 12];
  else if (l >= 3 && l < 12) {
    const int i = (l - 3) / 3, j = (l - 3) % 3;
    v = R[3 * i] * T.g_mat_d[g][j] + R[3 * i + 1] * T.g_mat_d[g][3 + j] + R[3 * i + 2] * T.g_mat_d[g][6 + j];
  } else {
    const int i = l < 3 ? l : l - 15;
    v = ((double)S.xpos[b][i] + (double)S.xpos_lo[b][i]) +
        (R[3 * i] * T.g_pos_d[g][0] + R[3 * i + 1] * T.g_pos_d[g][1] + R[3 * i + 2] * T.g_pos_d[g][2]);
    if (l >= 15 && type == DM_GEOM_MESH) {
      double gm[3];
      for (int j = 0; j < 3; j++) gm[j] = R[3 * i] * T.g_mat_d[g][j] + R[3 * i + 1] * T.g_mat_d[g][3 + j] + R[3 * i + 2] * T.g_mat_d[g][6 + j];
      v += gm[0] * T.m_center[me][0] + gm[1] * T.m_center[me][1] + gm[2] * T.m_center[me][2];
    }
  }
  return v;
}
__device__ __forceinline__ void stage_geoi(const Dev &T, const NpStage &W, int g, int slot) {
  const int type = T.g_type[g], me = T.g_mesh[g];
  const bool mesh = type == DM_GEOM_MESH;
  W.geoi[slot][0] = type; W.geoi[slot][1] = mesh ? T.m_vnum[me] : 0; W.geoi[slot][2] = mesh ? T.m_cnum[me] : 0;
  W.geoi[slot][3] = mesh ? T.m_vadr[me] : 0; W.geoi[slot][4] = mesh ? T.m_cadr[me] : 0;
}
// stage geom g of the current pair in slot `slot` (lanes 0..17 write one double each)
__device__ __forceinline__ void stage_geo(const Dev &T, const NpStage &W, int g, int slot, const int lane) {
  if (lane < 18) W.geo[slot][lane] = geo_entry(T, g, lane);
  if (lane == 0) stage_geoi(T, W, g, slot);
}
struct MeshPtrs { const double *vert; const int32_t *oidx; const double *clus; };
__device__ __forceinline__ void view_geo(const MeshPtrs &M, const NpStage &W, int slot, Geo &o) {
  o.type = W.geoi[slot][0]; o.nvert = W.geoi[slot][1]; o.nclus = W.geoi[slot][2];
  o.pos = &W.geo[slot][0]; o.mat = &W.geo[slot][3]; o.size = &W.geo[slot][12]; o.center = &W.geo[slot][15];
  o.vert = M.vert + 3 * (size_t)W.geoi[slot][3];
  o.oidx = M.oidx + W.geoi[slot][3];
  o.clus = M.clus + 8 * (size_t)W.geoi[slot][4];
}
// pair classes (cost): 0 analytic, 1 plane - mesh (support queries), 2 MPR
__device__ __forceinline__ int pair_class(const int t1, const int t2) {
  if (t1 == DM_GEOM_PLANE && t2 == DM_GEOM_MESH) return 1;
  if (t1 == DM_GEOM_PLANE || (t1 == DM_GEOM_SPHERE && (t2 == DM_GEOM_SPHERE || t2 == DM_GEOM_BOX)) || (t1 == DM_GEOM_BOX && t2 == DM_GEOM_BOX)) return 0;
  return 2;
}

__device__ __forceinline__ void make_frame(float *f) {   // [EXT] mju_makeFrame
  float n = sqrtf(dot3(f, f));
  if (n < MINVALF) { f[0] = 1; f[1] = f[2] = 0; } else { f[0] /= n; f[1] /= n; f[2] /= n; }
  if (sqrtf(dot3(f + 3, f + 3)) < 0.5f) {
    f[3] = f[4] = f[5] = 0;
    if (f[1] < 0.5f && f[1] > -0.5f) f[4] = 1; else f[5] = 1;
  }
  const float t = dot3(f, f + 3);
  for (int i = 0; i < 3; i++) f[3 + i] -= t * f[i];
  n = sqrtf(dot3(f + 3, f + 3));
  if (n < MINVALF) { f[3] = 1; f[4] = f[5] = 0; } else { f[3] /= n; f[4] /= n; f[5] /= n; }
  cross3(f + 6, f, f + 3);
}

// Separating-axis test of two oriented boxes (15 axes), conservative by `slack`: true only if the boxes are at least that far
// apart.  The filter is result-neutral: disjoint bounding boxes cannot hold intersecting geoms.
__device__ __forceinline__ bool obb_separated(const float *c1, const float *R1, const float *h1, const float *c2, const float *R2, const float *h2,
                              const float slack) {
  float R[9], AR[9], t[3], tw[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
  for (int i = 0; i < 3; i++) t[i] = R1[i] * tw[0] + R1[3 + i] * tw[1] + R1[6 + i] * tw[2];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      R[3 * i + j] = R1[i] * R2[j] + R1[3 + i] * R2[3 + j] + R1[6 + i] * R2[6 + j];
      AR[3 * i + j] = fabsf(R[3 * i + j]) + 1e-6f;
    }
  for (int i = 0; i < 3; i++)
    if (fabsf(t[i]) > h1[i] + h2[0] * AR[3 * i] + h2[1] * AR[3 * i + 1] + h2[2] * AR[3 * i + 2] + slack) return true;
  for (int j = 0; j < 3; j++)
    if (fabsf(t[0] * R[j] + t[1] * R[3 + j] + t[2] * R[6 + j]) > h2[j] + h1[0] * AR[j] + h1[1] * AR[3 + j] + h1[2] * AR[6 + j] + slack)
      return true;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      const float ra = h1[i1] * AR[3 * i2 + j] + h1[i2] * AR[3 * i1 + j], rb = h2[j1] * AR[3 * i + j2] + h2[j2] * AR[3 * i + j1];
      if (fabsf(t[i2] * R[3 * i1 + j] - t[i1] * R[3 * i2 + j]) > ra + rb + slack) return true;
    }
  return false;
}

// [EXT] mj_collision, part 1: candidate pairs in canonical order through the bounding-sphere + bounding-box filters; the survivors'
// pair ids go to S.u.co.surv in order.  Returns their number (capped; `overflow` set when the cap cut the list).
__device__ __forceinline__ int broadphase(const Dev &T, const int cap, int &overflow, const int lane) {
  int nsurv = 0;
  for (int base = 0; base < T.npair; base += 64) {
    const int p = base + lane;
    bool keep = false;
    if (p < T.npair) {
      const int g1 = T.p_g1[p], g2 = T.p_g2[p], ci1 = T.g_ci[g1], ci2 = T.g_ci[g2];
      float df[3] = {S.gpos[g2][0] - S.gpos[g1][0], S.gpos[g2][1] - S.gpos[g1][1], S.gpos[g2][2] - S.gpos[g1][2]};
      float c2[3], bc2[3] = {T.g_bc[g2][0], T.g_bc[g2][1], T.g_bc[g2][2]}, h2[3] = {T.g_bh[g2][0], T.g_bh[g2][1], T.g_bh[g2][2]};
      mat_vec(c2, S.gmat[ci2], bc2);
      for (int i = 0; i < 3; i++) c2[i] += S.gpos[g2][i];
      if (T.g_type[g1] != DM_GEOM_PLANE) {
        keep = sqrtf(dot3(df, df)) <= T.g_rbound[g1] + T.g_rbound[g2];
        if (keep) {
          float c1[3], bc1[3] = {T.g_bc[g1][0], T.g_bc[g1][1], T.g_bc[g1][2]}, h1[3] = {T.g_bh[g1][0], T.g_bh[g1][1], T.g_bh[g1][2]};
          mat_vec(c1, S.gmat[ci1], bc1);
          for (int i = 0; i < 3; i++) c1[i] += S.gpos[g1][i];
          keep = !obb_separated(c1, S.gmat[ci1], h1, c2, S.gmat[ci2], h2, 1e-4f);
        }
      } else {
        float nrm[3] = {S.gmat[ci1][2], S.gmat[ci1][5], S.gmat[ci1][8]};
        keep = !(T.g_rbound[g2] > 0) || dot3(df, nrm) <= T.g_rbound[g2];
        if (keep) {   // lowest point of the bounding box above the plane: no contact possible
          const float *M2 = S.gmat[ci2];
          float dc[3] = {c2[0] - S.gpos[g1][0], c2[1] - S.gpos[g1][1], c2[2] - S.gpos[g1][2]}, ext = 0;
          for (int j = 0; j < 3; j++) ext += fabsf(nrm[0] * M2[j] + nrm[1] * M2[3 + j] + nrm[2] * M2[6 + j]) * h2[j];
          keep = dot3(dc, nrm) - ext <= 1e-4f;
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    const int slot = nsurv + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
    if (keep) { if (slot < cap) S.u.co.surv[slot] = (int16_t)p; }
    nsurv += __popcll(m);
  }
  if (nsurv > cap) { overflow = 1; nsurv = cap; }
  return nsurv;
}

// [EXT] mj_collision, part 2: the narrowphase of ONE staged pair (geoms in W.geo / W.geoi): analytic routines for the pairs MuJoCo
// has them for, MPR for everything with a cylinder or a mesh.  Returns the number of contacts left in W.rc.
// out-of-line copies for the monolithic kernel (its register budget is the env phases'); the pair kernel inlines the bodies: the
// Geo views then stay in registers instead of one scratch copy per lane (they were passed by reference to the calls), and the
// kernel needs 190 instead of 226 VGPRs
__device__ __noinline__ int np_plane_mesh(Con *c, const Geo &p, const Geo &g, const int lane) { return np_plane_mesh_body(c, p, g, lane); }
__device__ __noinline__ int np_box_box(Con *c, const Geo &A, const Geo &Bx, double (*poly)[3], double (*tmp)[3]) { return np_box_box_body(c, A, Bx, poly, tmp); }

template <bool INL>
__device__ __forceinline__ int narrow_pair(const MeshPtrs &M, const NpStage &W, float *cache, const bool direct, const int pair,
                                           const int skip, const int lane) {
  // (in the monolithic kernel A and B go to scratch, one copy per lane, because the two out-of-line routines take them by reference.
  // Passing the staging pointers by value instead was 5 % SLOWER in the pair kernel — 5.07 against 4.81 ms per step — and needs the
  // pointers laundered, or hipcc 7.2 folds the constant LDS address into an unencodable `v_cmp_ne_u32 0, src_shared_base`.)
  Geo A, B;
  view_geo(M, W, 0, A);
  view_geo(M, W, 1, B);
  Con *rc = W.rc;
  int n = 0;
  const int t1 = A.type, t2 = B.type;
  if (t1 == DM_GEOM_PLANE) {
    if (t2 == DM_GEOM_SPHERE) n = np_plane_sphere(rc, A, B.pos, B.size[0]);
    else if (t2 == DM_GEOM_CYLINDER) n = np_plane_cylinder(rc, A, B);
    else if (t2 == DM_GEOM_BOX) n = np_plane_box(rc, A, B);
    else if (t2 == DM_GEOM_MESH && !(skip & SKIP_PLANE_MESH)) n = INL ? np_plane_mesh_body(rc, A, B, lane) : np_plane_mesh(rc, A, B, lane);
  } else if (t1 == DM_GEOM_SPHERE && t2 == DM_GEOM_SPHERE) n = np_sphere_sphere(rc, A.pos, A.size[0], B.pos, B.size[0]);
  else if (t1 == DM_GEOM_SPHERE && t2 == DM_GEOM_BOX) n = np_sphere_box(rc, A, B);
  else if (t1 == DM_GEOM_BOX && t2 == DM_GEOM_BOX) n = INL ? np_box_box_body(rc, A, B, W.poly0, W.poly1) : np_box_box(rc, A, B, W.poly0, W.poly1);
  else if (!(skip & SKIP_MPR)) n = np_convex(rc, A, B, (skip & SKIP_SEP_CACHE) ? nullptr : cache, direct, pair, W.ps, lane);
  return n;
}
// contact k of the staged pair -> the fp32 record the constraint stage reads: dist | pos 3 | frame 9 ([EXT] mju_makeFrame of the normal)
__device__ __forceinline__ void contact_record(const Con &c, float &dist, float *pos, float *fr) {
  dist = (float)c.dist;
  fr[0] = (float)c.n[0]; fr[1] = (float)c.n[1]; fr[2] = (float)c.n[2];
  for (int i = 3; i < 9; i++) fr[i] = 0;
  make_frame(fr);
  for (int i = 0; i < 3; i++) pos[i] = (float)c.pos[i];
}

}  // namespace g1
