// dm_g1_device.h — what every layer of the G1 engine shares: dimensions, the state-row and clip-row layouts, the model tables (Dev),
// the per-env LDS working set (Lds, g_S), the launch arguments of the step kernels (Launch) and of the pair kernel (PairLaunch, NpLds).
#pragma once
#define DM_ROBOT_G1 1
#define DmModel DmModelG1
#include "../../include/dm_model.h"
#undef DmModel
#include "../../include/deepmimic_g1_hip.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace g1 {

constexpr int NQ = 44, NV = 43, NU = 37, NB = 39, NG = 94, NJ = 38, NM = 434, NACT = 23, NOBS = 85, NREW = 23;
constexpr int MAXCON = DMG1_MAXCON, MAXROW = DMG1_MAXROW, MAXANC = 16, MAXSURV = 384, NCG = 48;   // NCG: geoms that collide (47)
constexpr int PAIRCAP = 128;    // split pipeline: surviving pairs per env and evaluation that the pair queue holds (monolithic: MAXSURV)
constexpr int NCH = 2;          // cluster chunks of 64 per hull: hulls of up to 128 clusters (g1_build_meshes checks)
constexpr int QM_STRIDE = 448;  // Euler: floats per env of the parked mass matrix (NM entries, rows of 64 B)
constexpr int STATE = 176;   // floats per env in the HBM state row
constexpr int S_QPOS = 0, S_QVEL = 44, S_WARM = 87, S_CTRL = 130, S_IDX = 167, S_EPLEN = 168, S_EPREW = 169, S_RCNT = 170, S_MOTION = 171;
constexpr int NOBS_C = DMG1_NOBS_COMBINED;   // DPCombinedEnv: 82 + extra contacts 8 + phase + player-action obs 7
// clip tables, per frame (written by dmg1_load_clip, read by step_enter and the task layer).  Clip row: 23 reward qpos | 23 reward
// qvel | root quat 4 | ee geom xpos 4 x 3 | root velocity xy 2.  Reset row: qpos 44 | qvel 43 | pad.  COM row: xyz | pad.
constexpr int CR_QPOS = 0, CR_QVEL = CR_QPOS + NREW, CR_ROOTQ = CR_QVEL + NREW, CR_EE = CR_ROOTQ + 4, CR_ROOTV = CR_EE + 12, CLIP_ROW = CR_ROOTV + 2;
constexpr int RESET_ROW = 88, RR_QPOS = 0, RR_QVEL = 44, COM_ROW = 4;
static_assert(CLIP_ROW == 64 && RR_QVEL >= RR_QPOS + NQ && RESET_ROW >= RR_QVEL + NV, "clip tables are allocated and indexed by these");
constexpr float MINVALF = 1e-15f, MAXVALF = 1e10f;
constexpr double MINVAL = 1e-15;
enum { MODE_STEP = 0, MODE_FORCED = 1, MODE_RESET = 2, MODE_SETSTATE = 3 };
enum { ROW_LIMIT = 0, ROW_CONTACT = 2, ROW_FRICTION = 3 };
// Launch::skip, the phases a launch leaves out.  The shipped library sets SKIP_SEP_CACHE alone (dmg1_set_null_cache, a test hook); the
// others are the switches of the diagnostic build (-DG1_PROFILE takes them from DMG1_SKIP), which the phase profiles are taken with.
enum {
  SKIP_PGS = 1,           // no PGS sweeps: fwd_constraint runs with zero iterations
  SKIP_COLLIDE = 2,       // no collision stage (monolithic kernel): zero contacts
  SKIP_PROJECT = 4,       // A = J M^-1 J^T is not built
  SKIP_ROWS = 8,          // no constraint rows
  SKIP_SOLVE = 16,        // the constraint solve sees zero rows
  SKIP_NARROW = 32,       // broadphase only (monolithic kernel): no survivor reaches the narrowphase
  SKIP_MPR = 64,          // narrowphase without the MPR pairs
  SKIP_PLANE_MESH = 128,  // narrowphase without the plane - mesh pairs
  SKIP_SEP_CACHE = 256,   // np_convex of the monolithic kernel gets a null separating-direction cache
};

struct Dev {   // read-only model tables (global memory, fp32)
  float timestep, tolerance, pgs_scale, K, B, solimp[5], total_mass_inv, gravity[3];
  float low_z, action_scale;
  int32_t iterations, npair, maxdepth, torso_body, floor_geom, rfoot_geom, lfoot_geom, ee_geom[4], extra_geom[8];
  int32_t rew_q[NREW], rew_v[NREW], rew_j[NREW];
  float qpos0[NQ];
  int32_t b_parent[40], b_depth[40], b_dof[40];
  float b_pos[40][3], b_quat[40][4], b_ipos[40][3], b_inertia[40][6], b_mass[40], b_invw[40];
  uint64_t b_desc[40];   // bit d: body d is in the subtree of b (incl. b)
  uint64_t b_chain[40];  // bit k: dof k moves body b
  int32_t d_body[44], d_nanc[44], d_madr[44], d_act[44];
  uint8_t d_anc[44][MAXANC];   // ancestors of dof k: parent, grand-parent, ...
  float d_axis[44][3], d_arm[44], d_damp[44], d_invw[44], d_floss[44], d_lo[44], d_hi[44], d_clo[44], d_chi[44];
  int32_t g_body[96], g_type[96], g_mesh[96], g_ci[96];   // g_ci: index into Lds::gmat, -1 for visual geoms
  float g_pos[96][3], g_mat[96][9], g_size[96][3], g_rbound[96], g_mu[96];
  float g_bc[96][3], g_bh[96][3];   // local bounding box of the geom (centre, half extents) for the OBB filter
  int16_t p_g1[1024], p_g2[1024];
  int32_t m_vadr[32], m_vnum[32], m_cadr[32], m_cnum[32];   // vertex range and cluster range of each mesh
  double m_center[32][3];
  uint8_t tri_a[128], tri_b[128];
  uint32_t f_tgt[44][64];   // factorisation step k, ancestor pairs p = lane (low half) and lane + 64 (high half): the qLD entry updated
  // fp64 copies of everything the pose chain of a body and the narrowphase read: the narrowphase is fp64, and so are its inputs
  // (a convex-convex contact normal depends discontinuously on the poses; fp32 poses moved it in ~3 % of thrashing env-steps)
  double timestep_d, qpos0_d[NQ], b_pos_d[40][3], b_quat_d[40][4], d_axis_d[44][3], g_pos_d[96][3], g_mat_d[96][9], g_size_d[96][3];
};

struct Lds {   // per-env working set (one wave): 19.2 KB, eight waves per CU
  float qpos[NQ], qvel[44], warm[44], ctrl[40];
  float xpos[40][3], xquat[40][4], xmat[40][9], xipos[40][3];
  float xpos_lo[40][3], xquat_lo[40][4];   // body pose in fp64 = (double)x + (double)x_lo: the fp32 consumers read the rounded value
  float x0q_lo[4];                         // the same for the normalised root quaternion the RK stages start from
  float xaxis[44][3];
  float gpos[96][3], gmat[NCG][9];   // rotation only of the geoms that collide (Dev::g_ci)
  float com[4];
  float cdof[44][6];
  float cvel[40][6];
  float qLD[NM + 2], dinv[44], dsq[44];
  float bias[44], fsm[44], qas[44], qacc[44], qfc[44], tmp[44];
  float x0q[NQ], x0v[44], accq[44], accv[44];
  int32_t info[8];   // ncon, nefc, nlimit, solver_iter, overflow, nsurv
#ifdef G1_PROFILE
  long long prof_t; unsigned prof[18];   // 16 used; 80 bytes keep the head of the working set a multiple of 16
#endif
  union {
    struct {   // smooth-dynamics scratch: dead once qacc_smooth is known
      float cinert[40][10], crb[40][10], cdofdot[44][6], cacc[40][6], cfrc[40][6];
    } sm;
    struct {   // contacts of the evaluation (kept for the observation) and the narrowphase staging (fp64, wave-uniform)
      float c_dist[MAXCON], c_pos[MAXCON][3], c_frame[MAXCON][9], c_mu[MAXCON];
      int32_t c_g1[MAXCON], c_g2[MAXCON];
      int16_t surv[MAXSURV];
      double geo[2][18];     // the two geoms of the pair being processed: pos 3 | mat 9 | size 3 | centre 3
      int32_t geoi[2][6];    // type, nvert, nclus, vertex start, cluster start, pad
      double rc[8][7];       // its contacts: dist, pos 3, normal 3
      double poly[2][16][3]; // box-box polygons
      double mpr_ps[4][9];   // MPR portal (v0..v3: v, v1, v2): wave-uniform state, 72 VGPRs if kept per lane
    } co;
    struct {   // low words of the RK stage's qpos: written by integrate_pos, read at the top of kinematics — between two evaluations,
      char skip[5680];   // when `sm` is dead; placed behind the end of `co` (the last contacts stay readable for the observation)
      float qlo[NQ];
    } rk;
  } u;
};

// The per-env working set is a file-scope __shared__ object: every phase is its own (out-of-line) function with its own
// register allocation, and all of them address it as LDS (ds_* instructions), not through generic pointers.
__shared__ Lds g_S;
#define S g_S
static_assert(sizeof(Lds) <= 20480, "eight waves per CU need <= 20 480 B of LDS per env");
static_assert(sizeof(((Lds *)0)->u.co) <= 5680 && sizeof(((Lds *)0)->u.rk) <= sizeof(((Lds *)0)->u.sm), "rk.qlo sits behind co, inside sm");

struct ClipDev {
  const float *rows;    // L x CLIP_ROW
  const float *reset;   // L x RESET_ROW
  const float *com;     // L x COM_ROW : mass-weighted body_xpos COM of the frame
  int32_t L, flags;
};

struct Launch {
  const Dev *T;
  const double *mesh_vert;   // hull vertices of all meshes, xyz, reordered into clusters of 64 (see g1_build_meshes)
  const int32_t *mesh_oidx;  // original index of each reordered vertex (tie-break of equal support values)
  const double *mesh_clus;   // per cluster: bounding-sphere centre xyz, radius
  float *state;              // N x STATE
  float *jt, *bt, *ar;       // per-env scratch: J^T [44][MAXROW], (D^-1/2 L^-T J^T) [44][MAXROW], A [MAXROW][MAXROW]
  float *rows;               // per-env scratch: R, aref -> b, force, friction-loss bound, meta (type | id << 2): [5][MAXROW]
  float *sepc;               // per-env separating-direction cache of the MPR pairs: [SEPC + 1][4]
  const int32_t *order;      // STEP: workgroup -> env: heaviest envs first (g1_schedule_kernel), the slot list of dmg1_step_active
                             // (an entry outside [0, N) ends its workgroup at once), or null
  int32_t *cost;             // STEP: per-env work estimate of this step, or null
  ClipDev clips[DMG1_MAX_CLIPS];   // DPEnv: the env's clip id picks one (multi-clip batches); DPCombinedEnv: 0..2 = walk, run, getup
  int32_t task, amnesty_steps, to_getup_len;
  int32_t nslots;            // workgroups of this launch that have an env (N, or the slots of dmg1_step_active); N stays the engine's
                             // env count: every per-env layout (state rows, queue blocks, ticket lists) is built on it
  int32_t N, mode, auto_reset, max_ep_length, run_forward, skip;   // skip: SKIP_* bits
  float vel_obs_scale, high_z, obs_bound;
  uint64_t seed;
  const float *actions, *in_qpos, *in_qvel, *in_warm;
  const uint8_t *mask;
  const int32_t *idx_init;
  float *obs, *rew, *terms, *terminal_obs, *debug;
  uint8_t *done;
  int32_t *reason;
  // ---- split pipeline (g1_env_kernel / g1_pair_kernel): per-env slot of the LDS working set + step context between launches, and
  // the pair queue of the collision stage
  char *ws;                  // N x WS_BYTES
  double *pq_geo;            // [N][PAIRCAP][36]: the two staged geoms of a surviving pair (fp64)
  int32_t *pq_pair;          // [N][PAIRCAP]: pair id of the env's s-th survivor (canonical order)
  int32_t *pq_cnt;           // [N][PAIRCAP]: contacts the pair kernel found
  float *pq_con;             // [N][PAIRCAP][8][16]: dist | pos 3 | frame 9 of each
  int32_t *tick;             // [2][N * PAIRCAP]: tickets (env << 8 | s): list 0 = support-query pairs (MPR, plane-mesh), 1 = analytic
  int32_t *qctr;             // per round: tickets in list 0, in list 1, queue head, pad
  float *sepc2;              // [N][1024][4]: separating-direction cache, one entry per (env, pair)
  int32_t round, pad3;
  float *qm;                 // Euler kernels: [N][QM_STRIDE], the unfactored M of the evaluation (park_m -> euler_damped_qacc); else null
};

struct PairLaunch {
  const Dev *T;
  const double *mesh_vert; const int32_t *mesh_oidx; const double *mesh_clus;
  const double *pq_geo; const int32_t *pq_pair; int32_t *pq_cnt; float *pq_con;
  const int32_t *tick; int32_t *qctr; float *sepc2;
  int32_t N, pad;
};
struct NpLds { double geo[2][18]; int32_t geoi[2][6]; double rc[8][7]; double poly[2][16][3]; double mpr_ps[4][9]; };

#define SYNC() __syncthreads()
#ifdef G1_PROFILE
#define PROF(k) do { const long long t_ = clock64(); if (threadIdx.x == 0) { S.prof[k] += (unsigned)(t_ - S.prof_t); } S.prof_t = t_; } while (0)
#else
#define PROF(k) do {} while (0)
#endif

}  // namespace g1
