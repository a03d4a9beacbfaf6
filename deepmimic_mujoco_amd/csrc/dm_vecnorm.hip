// dm_vecnorm.hip — SB3's VecNormalize on the device (include/deepmimic_vecnorm.h): fp64 running mean / variance of the observation
// columns and of the discounted returns, and the clipped transforms.  Shares nothing with the engines.  A training step is three
// launches: moments of row chunks, their merge in ascending chunk order into the running statistics, the transform.
// No atomics, no order that depends on timing: every sum is formed by one thread in index order.  The _sync entry points keep the
// statistics as base (agreed by all ranks) + acc (this rank's since then) and rebuild the running set from them; every
// merge of theirs is dm_vn_merge of the header.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/deepmimic_vecnorm.h"

namespace {

constexpr int BLOCK = 256;                // every kernel: four waves
constexpr int WAVES = BLOCK / 64;
constexpr int TILE = 64;                  // columns of a block: the lanes of a wave read consecutive columns of a row
constexpr int MIN_CHUNK = 64;             // rows of a moments chunk while N <= MIN_CHUNK * MAX_CHUNKS
constexpr int MAX_CHUNKS = 256;           // the merge walks them one by one: beyond this the chunks grow instead
constexpr int NORM_ROWS = 16;             // rows of a normalise block, four per wave
constexpr int UPD_BLOCK = 1024;           // update kernel: sixteen waves share the chunks of one column tile
constexpr int UPD_WAVES = UPD_BLOCK / 64;

thread_local char g_err[160];

int refuse(const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return DM_VECNORM_EINVAL;
}

// rows of one chunk, a multiple of WAVES; wave w of a chunk owns rows [w, w + 1) * rows / WAVES of it
int chunk_rows(int N) {
  if (N <= MIN_CHUNK * MAX_CHUNKS) return MIN_CHUNK;
  const int r = (int)(((long long)N + MAX_CHUNKS - 1) / MAX_CHUNKS);
  return (r + WAVES - 1) / WAVES * WAVES;
}

int chunk_count(int N) {
  const int r = chunk_rows(N);
  return (int)(((long long)N + r - 1) / r);
}

// Columns col0 .. col0 + ncols - 1 of the virtual table [N, D + 1]: column c < D is observation column c, column D is the discounted
// return returns * gamma + rew, which the first pass also stores.  part: [chunks, 2, D + 1] (mean, sum of squared deviations), then
// one double: the observation count as this launch found it, which the update launch reads instead of the count it rewrites.
struct MomentsArgs {
  const float *obs, *rew;
  const double *obs_count;
  double *returns, *part;
  double gamma;
  int N, D, col0, ncols, rows, chunks;
};

__device__ __forceinline__ double chan_mean(double ma, double na, double mb, double nb) { return ma + (mb - ma) * nb / (na + nb); }
__device__ __forceinline__ double chan_m2(double ma, double qa, double na, double mb, double qb, double nb) {
  const double d = mb - ma;
  return qa + qb + d * d * na * nb / (na + nb);
}

// grid (chunks, column tiles).  Two passes over the wave's rows of the chunk in fp64 (sum, then squared deviations from the wave's
// own mean: a column with a large mean and a small spread keeps its variance), then Chan's merge of the four waves in ascending
// order by wave 0.  One barrier, at the top level: no thread returns before it.
__global__ void __launch_bounds__(BLOCK) vecnorm_moments_kernel(MomentsArgs a) {
  __shared__ double s_mean[WAVES][TILE], s_m2[WAVES][TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ci = blockIdx.y * TILE + lane, col = a.col0 + ci;
  const bool live = ci < a.ncols;
  const bool is_ret = col == a.D;
  const int per_wave = a.rows / WAVES;
  const long long c0 = (long long)blockIdx.x * a.rows;
  long long r0 = c0 + (long long)wave * per_wave, r1 = r0 + per_wave;
  if (r0 > a.N) r0 = a.N;
  if (r1 > a.N) r1 = a.N;
  double mean = 0.0, m2 = 0.0;
  if (live && r1 > r0) {
    double sum = 0.0;
    if (is_ret) {
      for (long long r = r0; r < r1; r++) {
        const double v = a.returns[r] * a.gamma + (double)a.rew[r];
        a.returns[r] = v;
        sum += v;
      }
    } else {
      for (long long r = r0; r < r1; r++) sum += (double)a.obs[(size_t)r * a.D + col];
    }
    mean = sum / (double)(r1 - r0);
    if (is_ret) {
      for (long long r = r0; r < r1; r++) {
        const double d = a.returns[r] - mean;            // what this thread stored above
        m2 += d * d;
      }
    } else {
      for (long long r = r0; r < r1; r++) {
        const double d = (double)a.obs[(size_t)r * a.D + col] - mean;
        m2 += d * d;
      }
    }
  }
  s_mean[wave][lane] = mean;
  s_m2[wave][lane] = m2;
  __syncthreads();
  if (wave == 0 && live) {
    double n = 0.0, m = 0.0, q = 0.0;
    for (int w = 0; w < WAVES; w++) {
      long long w0 = c0 + (long long)w * per_wave, w1 = w0 + per_wave;
      if (w0 > a.N) w0 = a.N;
      if (w1 > a.N) w1 = a.N;
      const double nb = (double)(w1 - w0);
      if (nb > 0.0) {
        const double mb = s_mean[w][lane], qb = s_m2[w][lane];
        q = n > 0.0 ? chan_m2(m, q, n, mb, qb, nb) : qb;
        m = n > 0.0 ? chan_mean(m, n, mb, nb) : mb;
        n += nb;
      }
    }
    const size_t W = (size_t)a.D + 1;
    a.part[((size_t)blockIdx.x * 2 + 0) * W + col] = m;
    a.part[((size_t)blockIdx.x * 2 + 1) * W + col] = q;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.part[(size_t)a.chunks * 2 * ((size_t)a.D + 1)] = a.obs_count[0];
}

struct UpdateArgs {
  const double *part;
  double *obs_mean, *obs_var, *obs_count, *ret_stats;
  int N, D, col0, ncols, rows, chunks;
  const double *base;       // SYNC only: [2 D + 4], read
  double *acc;              // SYNC only: [2 D + 4]; the moments launch copied ITS observation count behind part
};

// grid: column tiles.  Wave w of sixteen merges its contiguous share of the chunks of column col0 + tile * 64 + lane in ascending
// order, wave 0 then merges the sixteen partial results in ascending order and folds the batch (mean, population variance, N) into the
// running statistics as RunningMeanStd.update_from_moments does.  One barrier, at the top level.  The observation count is read from
// the copy the moments launch left behind part, so the one thread that rewrites it races with no reader.
// SYNC: the batch is folded into acc instead, and the running statistics are rewritten as merge(base, acc); base is only read.
template <bool SYNC>
__global__ void __launch_bounds__(UPD_BLOCK) vecnorm_update_kernel(UpdateArgs a) {
  __shared__ double s_mean[UPD_WAVES][TILE], s_m2[UPD_WAVES][TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ci = blockIdx.x * TILE + lane, col = a.col0 + ci;
  const bool live = ci < a.ncols;
  const size_t W = (size_t)a.D + 1;
  const double obs_count = a.part[(size_t)a.chunks * 2 * W];
  const int per_wave = (a.chunks + UPD_WAVES - 1) / UPD_WAVES;
  int c0 = wave * per_wave, c1 = c0 + per_wave;
  if (c0 > a.chunks) c0 = a.chunks;
  if (c1 > a.chunks) c1 = a.chunks;
  double n = 0.0, m = 0.0, q = 0.0;
  if (live) {
    for (int c = c0; c < c1; c++) {
      const long long left = (long long)a.N - (long long)c * a.rows;
      const double nc = (double)(left < a.rows ? left : a.rows);
      const double mc = a.part[((size_t)c * 2 + 0) * W + col], qc = a.part[((size_t)c * 2 + 1) * W + col];
      q = c > c0 ? chan_m2(m, q, n, mc, qc, nc) : qc;
      m = c > c0 ? chan_mean(m, n, mc, nc) : mc;
      n += nc;
    }
  }
  s_mean[wave][lane] = m;
  s_m2[wave][lane] = q;
  __syncthreads();
  if (wave == 0 && live) {
    n = 0.0;
    m = 0.0;
    q = 0.0;
    for (int w = 0; w < UPD_WAVES; w++) {
      long long r0 = (long long)w * per_wave * a.rows, r1 = r0 + (long long)per_wave * a.rows;      // the rows of wave w's chunks
      if (r0 > a.N) r0 = a.N;
      if (r1 > a.N) r1 = a.N;
      const double nw = (double)(r1 - r0);
      if (nw > 0.0) {
        const double mw = s_mean[w][lane], qw = s_m2[w][lane];
        q = n > 0.0 ? chan_m2(m, q, n, mw, qw, nw) : qw;
        m = n > 0.0 ? chan_mean(m, n, mw, nw) : mw;
        n += nw;
      }
    }
    const double nb = (double)a.N;
    const double bv = q / nb;
    const bool is_ret = col == a.D;
    if constexpr (SYNC) {
      const int at_m = is_ret ? 2 * a.D + 1 : col, at_v = is_ret ? 2 * a.D + 2 : a.D + col, at_c = is_ret ? 2 * a.D + 3 : 2 * a.D;
      double am = a.acc[at_m], av = a.acc[at_v], ac = is_ret ? a.acc[at_c] : obs_count;
      dm_vn_merge(am, av, ac, m, bv, nb);
      double rm = a.base[at_m], rv = a.base[at_v], rc = a.base[at_c];
      dm_vn_merge(rm, rv, rc, am, av, ac);
      a.acc[at_m] = am;
      a.acc[at_v] = av;
      if (is_ret) {
        a.acc[at_c] = ac;
        a.ret_stats[0] = rm;
        a.ret_stats[1] = rv;
        a.ret_stats[2] = rc;
      } else {
        a.obs_mean[col] = rm;
        a.obs_var[col] = rv;
        if (col == 0) {                                  // the one writer of both observation counts; every reader took the copy
          a.acc[at_c] = ac;
          a.obs_count[0] = rc;
        }
      }
      return;                                            // past the only barrier
    }
    const double mean = is_ret ? a.ret_stats[0] : a.obs_mean[col], var = is_ret ? a.ret_stats[1] : a.obs_var[col];
    const double count = is_ret ? a.ret_stats[2] : obs_count;
    const double d = m - mean, tot = count + nb;
    const double new_mean = mean + d * nb / tot;
    const double new_var = (var * count + bv * nb + d * d * count * nb / tot) / tot;
    if (is_ret) {
      a.ret_stats[0] = new_mean;
      a.ret_stats[1] = new_var;
      a.ret_stats[2] = tot;
    } else {
      a.obs_mean[col] = new_mean;
      a.obs_var[col] = new_var;
    }
  }
  if (!SYNC && blockIdx.x == 0 && threadIdx.x == 0 && a.col0 == 0) a.obs_count[0] = obs_count + (double)a.N;
}

// grid: blocks over the world * (2 D + 4) doubles of gather.  Row `rank` = acc, every other row = 0.
__global__ void __launch_bounds__(BLOCK) vecnorm_sync_pack_kernel(const double *acc, double *gather, int S, int world, int rank) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (long long)world * S) return;
  const int r = (int)(i / S), j = (int)(i - (long long)r * S);
  gather[i] = r == rank ? acc[j] : 0.0;
}

struct SyncMergeArgs {
  const double *gather;
  double *base, *acc, *obs_mean, *obs_var, *obs_count, *ret_stats;
  int D, world;
};

constexpr int MERGE_ROWS = 8;             // rows of gather in flight per column before their merges start

// One block.  A thread owns column col of the virtual table (col = D: the returns), col + BLOCK, ...: it loads MERGE_ROWS rows of its
// column at a time (independent loads, consecutive lanes on consecutive addresses, the counts one address per wave) and merges them
// into base in ascending rank order; only that arithmetic is a chain.  Then running = base and acc = empty.  The old observation count
// of base is read by every thread before the one barrier and written after it.
__global__ void __launch_bounds__(BLOCK) vecnorm_sync_merge_kernel(SyncMergeArgs a) {
  const int D = a.D, S = 2 * D + 4;
  const double obs_count = a.base[2 * D];
  __syncthreads();
  for (int col = threadIdx.x; col <= D; col += BLOCK) {
    const bool is_ret = col == D;
    const int at_m = is_ret ? 2 * D + 1 : col, at_v = is_ret ? 2 * D + 2 : D + col, at_c = is_ret ? 2 * D + 3 : 2 * D;
    double m = a.base[at_m], v = a.base[at_v], c = is_ret ? a.base[at_c] : obs_count;
    for (int r0 = 0; r0 < a.world; r0 += MERGE_ROWS) {
      double gm[MERGE_ROWS], gv[MERGE_ROWS], gc[MERGE_ROWS];
#pragma unroll
      for (int k = 0; k < MERGE_ROWS; k++) {
        const bool in = r0 + k < a.world;
        const double *row = a.gather + (size_t)(in ? r0 + k : 0) * S;
        gm[k] = row[at_m];
        gv[k] = row[at_v];
        gc[k] = in ? row[at_c] : 0.0;                    // count 0: skipped
      }
#pragma unroll
      for (int k = 0; k < MERGE_ROWS; k++) dm_vn_merge(m, v, c, gm[k], gv[k], gc[k]);
    }
    a.base[at_m] = m;
    a.base[at_v] = v;
    a.acc[at_m] = 0.0;
    a.acc[at_v] = 0.0;
    if (is_ret) {
      a.base[at_c] = c;
      a.acc[at_c] = 0.0;
      a.ret_stats[0] = m;
      a.ret_stats[1] = v;
      a.ret_stats[2] = c;
    } else {
      a.obs_mean[col] = m;
      a.obs_var[col] = v;
      if (col == 0) {
        a.base[at_c] = c;
        a.acc[at_c] = 0.0;
        a.obs_count[0] = c;
      }
    }
  }
}

struct NormArgs {
  const float *obs, *tobs, *rew;
  float *obs_out, *tobs_out, *rew_out;
  const uint8_t *done;
  const double *obs_mean, *obs_var, *ret_stats;
  double *returns;          // NULL: not touched
  double epsilon, clip_obs, clip_reward;
  int n, D, norm_obs, norm_reward, zero_returns;      // zero_returns: 1 = of done envs, 2 = of every env (reset)
};

// The transform itself is dm_vn_norm_one of the header (shared with dm_sac_gather_norm).
// grid (row blocks of NORM_ROWS, column tiles); no barrier.  Thread (wave, lane) owns column tile * 64 + lane of rows wave, wave + 4,
// ... of its block: it reads an element, then writes it, so in-place pointers are safe.  The first NORM_ROWS threads of the blocks
// of column tile 0 handle the reward and the return of one row each.
__global__ void __launch_bounds__(BLOCK) vecnorm_normalize_kernel(NormArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * TILE + lane;
  const long long base = (long long)blockIdx.x * NORM_ROWS;
  if (col < a.D && (a.obs || a.tobs)) {
    const double mean = a.norm_obs ? a.obs_mean[col] : 0.0;
    const double scale = a.norm_obs ? sqrt(a.obs_var[col] + a.epsilon) : 1.0;
    for (int j = wave; j < NORM_ROWS; j += WAVES) {
      const long long r = base + j;
      if (r >= a.n) break;
      const size_t at = (size_t)r * a.D + col;
      if (a.obs) {
        const float x = a.obs[at];
        a.obs_out[at] = a.norm_obs ? dm_vn_norm_one((double)x, mean, scale, a.clip_obs) : x;
      }
      if (a.tobs) {
        const float x = a.tobs[at];
        a.tobs_out[at] = (a.norm_obs && a.done[r] != 0) ? dm_vn_norm_one((double)x, mean, scale, a.clip_obs) : x;
      }
    }
  }
  if (blockIdx.y == 0 && threadIdx.x < NORM_ROWS) {
    const long long r = base + threadIdx.x;
    if (r < a.n) {
      if (a.rew) {
        const float x = a.rew[r];
        a.rew_out[r] = a.norm_reward ? dm_vn_norm_one((double)x, 0.0, sqrt(a.ret_stats[1] + a.epsilon), a.clip_reward) : x;
      }
      if (a.returns && (a.zero_returns == 2 || (a.zero_returns == 1 && a.done[r] != 0))) a.returns[r] = 0.0;
    }
  }
}

int check(const DmVecNorm *v, bool stateful) {
  g_err[0] = 0;
  if (const char *why = dm_vn_struct_error(v)) return refuse(why);
  if (stateful) {
    if (!v->returns || !v->scratch) return refuse("null returns or scratch in DmVecNorm");
    if (v->scratch_bytes < dm_vecnorm_scratch_bytes(v->N, v->D)) return refuse("scratch smaller than dm_vecnorm_scratch_bytes(N, D)");
  }
  return DM_VECNORM_OK;
}

int check_sync(const DmVecNorm *v, const DmVecNormSync *y, bool stateful) {
  const int rc = check(v, stateful);
  if (rc != DM_VECNORM_OK) return rc;
  if (const char *why = dm_vn_sync_error(y)) return refuse(why);
  return DM_VECNORM_OK;
}

int launch_status() {
  if (hipGetLastError() == hipSuccess) return DM_VECNORM_OK;
  snprintf(g_err, sizeof g_err, "a launch was refused");
  return DM_VECNORM_EHIP;
}

// the two statistics launches over columns [col0, col0 + ncols) of the virtual table
// `y`: the _sync entry points; the observation count the moments launch copies for the update launch is then acc's
void launch_update(const DmVecNorm *v, const float *obs, const float *rew, int col0, int ncols, hipStream_t s, const DmVecNormSync *y = nullptr) {
  const int rows = chunk_rows(v->N), chunks = chunk_count(v->N);
  const MomentsArgs m = {obs, rew, y ? y->acc + 2 * v->D : v->obs_count, v->returns, v->scratch, v->gamma, v->N, v->D, col0, ncols, rows, chunks};
  hipLaunchKernelGGL(vecnorm_moments_kernel, dim3(chunks, (ncols + TILE - 1) / TILE), dim3(BLOCK), 0, s, m);
  const UpdateArgs u = {v->scratch, v->obs_mean, v->obs_var, v->obs_count, v->ret_stats, v->N, v->D, col0, ncols, rows, chunks,
                        y ? y->base : nullptr, y ? y->acc : nullptr};
  if (y)
    hipLaunchKernelGGL(vecnorm_update_kernel<true>, dim3((ncols + TILE - 1) / TILE), dim3(UPD_BLOCK), 0, s, u);
  else
    hipLaunchKernelGGL(vecnorm_update_kernel<false>, dim3((ncols + TILE - 1) / TILE), dim3(UPD_BLOCK), 0, s, u);
}

void launch_normalize(const NormArgs &a, hipStream_t s) {
  const int tiles = (a.obs || a.tobs) ? (a.D + TILE - 1) / TILE : 1;
  hipLaunchKernelGGL(vecnorm_normalize_kernel, dim3((unsigned)(((long long)a.n + NORM_ROWS - 1) / NORM_ROWS), tiles), dim3(BLOCK), 0, s, a);
}

}  // namespace

extern "C" long long dm_vecnorm_scratch_bytes(int N, int D) {
  if (N < 1 || D < 1) return DM_VECNORM_EINVAL;
  return ((long long)chunk_count(N) * 2 * ((long long)D + 1) + 1) * (long long)sizeof(double);
}

namespace {

// dm_vecnorm_step (y = NULL) and dm_vecnorm_step_sync after their struct checks
int step_checked(const DmVecNorm *v, const float *obs, const float *rew, const uint8_t *done, const float *tobs, float *obs_out,
                 float *rew_out, float *tobs_out, const DmVecNormSync *y, void *stream) {
  if (!obs || !rew || !done || !obs_out || !rew_out) return refuse("null step input or output");
  if ((tobs == nullptr) != (tobs_out == nullptr)) return refuse("tobs and tobs_out are given together or not at all");
  if (hipSetDevice(v->device) != hipSuccess) return DM_VECNORM_EHIP;
  if (v->training) {
    const int col0 = v->norm_obs ? 0 : v->D;             // the return column is updated whenever training
    launch_update(v, obs, rew, col0, v->D + 1 - col0, (hipStream_t)stream, y);
  }
  // an identity that would copy a buffer onto itself is left out
  const bool obs_same = !v->norm_obs && obs == obs_out, tobs_same = !v->norm_obs && tobs == tobs_out;
  const bool rew_same = !v->norm_reward && rew == rew_out;
  const NormArgs a = {obs_same ? nullptr : obs, tobs_same ? nullptr : tobs, rew_same ? nullptr : rew, obs_out, tobs_out, rew_out, done,
                      v->obs_mean, v->obs_var, v->ret_stats, v->returns, v->epsilon, v->clip_obs, v->clip_reward,
                      v->N, v->D, v->norm_obs, v->norm_reward, 1};
  launch_normalize(a, (hipStream_t)stream);
  return launch_status();
}

int reset_checked(const DmVecNorm *v, const float *obs, float *obs_out, const DmVecNormSync *y, void *stream) {
  if (!obs || !obs_out) return refuse("null reset input or output");
  if (hipSetDevice(v->device) != hipSuccess) return DM_VECNORM_EHIP;
  if (v->training && v->norm_obs) launch_update(v, obs, nullptr, 0, v->D, (hipStream_t)stream, y);
  const bool obs_same = !v->norm_obs && obs == obs_out;
  const NormArgs a = {obs_same ? nullptr : obs, nullptr, nullptr, obs_out, nullptr, nullptr, nullptr,
                      v->obs_mean, v->obs_var, v->ret_stats, v->returns, v->epsilon, v->clip_obs, v->clip_reward,
                      v->N, v->D, v->norm_obs, v->norm_reward, 2};
  launch_normalize(a, (hipStream_t)stream);
  return launch_status();
}

}  // namespace

extern "C" int dm_vecnorm_step(const DmVecNorm *v, const float *obs, const float *rew, const uint8_t *done, const float *tobs,
                               float *obs_out, float *rew_out, float *tobs_out, void *stream) {
  const int rc = check(v, true);
  return rc != DM_VECNORM_OK ? rc : step_checked(v, obs, rew, done, tobs, obs_out, rew_out, tobs_out, nullptr, stream);
}

extern "C" int dm_vecnorm_step_sync(const DmVecNorm *v, const float *obs, const float *rew, const uint8_t *done, const float *tobs,
                                    float *obs_out, float *rew_out, float *tobs_out, const DmVecNormSync *y, void *stream) {
  const int rc = check_sync(v, y, true);
  return rc != DM_VECNORM_OK ? rc : step_checked(v, obs, rew, done, tobs, obs_out, rew_out, tobs_out, y, stream);
}

extern "C" int dm_vecnorm_reset(const DmVecNorm *v, const float *obs, float *obs_out, void *stream) {
  const int rc = check(v, true);
  return rc != DM_VECNORM_OK ? rc : reset_checked(v, obs, obs_out, nullptr, stream);
}

extern "C" int dm_vecnorm_reset_sync(const DmVecNorm *v, const float *obs, float *obs_out, const DmVecNormSync *y, void *stream) {
  const int rc = check_sync(v, y, true);
  return rc != DM_VECNORM_OK ? rc : reset_checked(v, obs, obs_out, y, stream);
}

extern "C" int dm_vecnorm_sync_pack(const DmVecNorm *v, const DmVecNormSync *y, void *stream) {
  const int rc = check_sync(v, y, false);
  if (rc != DM_VECNORM_OK) return rc;
  if (hipSetDevice(v->device) != hipSuccess) return DM_VECNORM_EHIP;
  const int S = 2 * v->D + 4;
  const long long total = (long long)y->world * S;
  hipLaunchKernelGGL(vecnorm_sync_pack_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, y->acc,
                     y->gather, S, y->world, y->rank);
  return launch_status();
}

extern "C" int dm_vecnorm_sync_merge(const DmVecNorm *v, const DmVecNormSync *y, void *stream) {
  const int rc = check_sync(v, y, false);
  if (rc != DM_VECNORM_OK) return rc;
  if (hipSetDevice(v->device) != hipSuccess) return DM_VECNORM_EHIP;
  const SyncMergeArgs a = {y->gather, y->base, y->acc, v->obs_mean, v->obs_var, v->obs_count, v->ret_stats, v->D, y->world};
  hipLaunchKernelGGL(vecnorm_sync_merge_kernel, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, a);
  return launch_status();
}

extern "C" int dm_vecnorm_apply(const DmVecNorm *v, int n, const float *obs, float *obs_out, const float *rew, float *rew_out,
                                void *stream) {
  const int rc = check(v, false);
  if (rc != DM_VECNORM_OK) return rc;
  if (n < 1) return refuse("n < 1");
  if ((obs == nullptr) != (obs_out == nullptr) || (rew == nullptr) != (rew_out == nullptr)) return refuse("an input without its output");
  if (!obs && !rew) return refuse("neither observations nor rewards");
  if (hipSetDevice(v->device) != hipSuccess) return DM_VECNORM_EHIP;
  const NormArgs a = {obs, nullptr, rew, obs_out, nullptr, rew_out, nullptr,
                      v->obs_mean, v->obs_var, v->ret_stats, nullptr, v->epsilon, v->clip_obs, v->clip_reward,
                      n, v->D, v->norm_obs, v->norm_reward, 0};
  launch_normalize(a, (hipStream_t)stream);
  return launch_status();
}

extern "C" const char *dm_vecnorm_last_error(void) { return g_err; }
