// dm_trace.hip — episode debug log on the device (include/deepmimic_trace.h): a ring of the last K steps per env, written after
// every engine step from what the engine's get_state entry point returned, and frozen copies of the rings of the envs whose step
// ended with a chosen reason.  Shares nothing with the engines; copy semantics throughout (no arithmetic on a logged value).
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/deepmimic_trace.h"

namespace {

constexpr int TW_BLOCK = 256;             // entry kernel: one wave writes one env's entry
constexpr int TW_WAVES = TW_BLOCK / 64;
constexpr int TC_BLOCK = 1024;            // capture kernel: one workgroup; N is walked in chunks of TC_BLOCK envs
constexpr int TC_WAVES = TC_BLOCK / 64;

thread_local char g_err[160];

int refuse(const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return DM_TRACE_EINVAL;
}

struct TraceIn {
  const float *qpos, *qvel, *warm, *actions, *rew;
  const uint8_t *done;
  const int32_t *reason, *env_ids;
  int32_t nslots, kind;
  uint32_t reason_mask;
};

// No barrier.  The wave of slot s owns env env_ids[s]: it reads head[env] once, writes row head mod K and then bumps head.
__global__ void __launch_bounds__(TW_BLOCK) trace_write_kernel(DmTraceBufs b, TraceIn in) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * TW_WAVES + (threadIdx.x >> 6);
  if (slot >= in.nslots) return;
  const int env = in.env_ids ? in.env_ids[slot] : slot;
  if (env < 0 || env >= b.N) return;      // as dm_step_active skips it
  const uint32_t h = b.head[env];
  float *row = b.ring + ((size_t)env * b.K + h % (uint32_t)b.K) * b.W;
  const int o1 = b.nq, o2 = o1 + b.nv, o3 = o2 + b.nv, o4 = o3 + b.na;
  const bool step = in.kind == DM_TRACE_KIND_STEP;
  for (int j = lane; j < o4; j += 64) {
    float v;
    if (j < o1) v = in.qpos[(size_t)env * b.nq + j];
    else if (j < o2) v = in.qvel[(size_t)env * b.nv + (j - o1)];
    else if (j < o3) v = in.warm[(size_t)env * b.nv + (j - o2)];
    else v = step ? in.actions[(size_t)env * b.na + (j - o3)] : 0.0f;
    row[j] = v;
  }
  const int dn = step ? (in.done[env] != 0) : 0, rs = step ? in.reason[env] : 0;
  if (lane < DM_TRACE_TAIL) {
    float v;
    if (lane == 0) v = step ? in.rew[env] : 0.0f;
    else if (lane == 1) v = __int_as_float(dn);
    else if (lane == 2) v = __int_as_float(rs);
    else if (lane == 3) v = __int_as_float(in.kind);
    else v = __int_as_float((int)h);
    row[o4 + lane] = v;
  }
  if (lane == 0) {
    b.head[env] = h + 1u;
    if (dn && rs >= 0 && rs < 32 && ((in.reason_mask >> rs) & 1u)) b.trig[env] = 1;
  }
}

// One workgroup, launched after trace_write_kernel on the same stream.  The slot of a trigger is cap_count[0] + the number of
// triggering envs below it: ballot + popcount per wave, wave totals through LDS, no atomics, so the order is ascending env on
// every run.  Barriers: three per chunk, all at the top level of the chunk loop, whose trip count ceil(N / TC_BLOCK) is a launch
// argument.  The copy loops between them contain no barrier; their trip count nfile is computed from wave_total[] and values
// every thread holds alike.
__global__ void __launch_bounds__(TC_BLOCK) trace_capture_kernel(DmTraceBufs b) {
  __shared__ int wave_total[TC_WAVES];
  __shared__ int file_env[TC_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int filed0 = b.cap_count[0];      // read by every thread; thread 0 rewrites it after the last barrier
  int seen = 0;                           // triggers of the chunks already walked (the same value in every thread)
  for (int base = 0; base < b.N; base += TC_BLOCK) {
    const int env = base + tid;
    bool t = false;
    if (env < b.N && b.trig[env] != 0) {
      t = true;
      b.trig[env] = 0;                    // zero between calls
    }
    const unsigned long long ballot = __ballot(t);
    if (lane == 0) wave_total[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, chunk = 0;
    for (int w = 0; w < TC_WAVES; w++) {
      const int c = wave_total[w];
      if (w < wave) before += c;
      chunk += c;
    }
    const int first = filed0 + seen;      // slot of this chunk's first trigger
    int nfile = b.C - first;              // how many of this chunk's triggers still find a slot
    nfile = nfile < 0 ? 0 : (nfile > chunk ? chunk : nfile);
    const int rank = before + __popcll(ballot & ((1ull << lane) - 1ull));
    if (t && rank < nfile) file_env[rank] = env;     // rank < chunk <= TC_BLOCK
    __syncthreads();
    for (int f = 0; f < nfile; f++) {
      const int e = file_env[f], slot = first + f;   // slot < C
      const uint32_t h = b.head[e];
      const uint32_t rows = h < (uint32_t)b.K ? h : (uint32_t)b.K;
      const uint32_t oldest = h - rows;
      const float *src = b.ring + (size_t)e * b.K * b.W;
      float *dst = b.cap + (size_t)slot * b.K * b.W;
      for (uint32_t r = wave; r < rows; r += TC_WAVES) {
        const float *s = src + (size_t)((oldest + r) % (uint32_t)b.K) * b.W;
        for (int j = lane; j < b.W; j += 64) dst[(size_t)r * b.W + j] = s[j];
      }
      if (tid == 0) {
        const float *last = src + (size_t)((h - 1u) % (uint32_t)b.K) * b.W;      // a trigger has h >= 1
        b.cap_meta[4 * slot + 0] = e;
        b.cap_meta[4 * slot + 1] = (int)rows;
        b.cap_meta[4 * slot + 2] = (int)h;
        b.cap_meta[4 * slot + 3] = __float_as_int(last[b.W - 3]);
      }
    }
    seen += chunk;
    __syncthreads();                      // wave_total and file_env are rewritten by the next chunk
  }
  if (tid == 0) {
    const int filed = filed0 + seen;
    b.cap_count[0] = filed > b.C ? b.C : filed;
    b.cap_count[1] += seen;
  }
}

int check(const DmTraceBufs *b, const void *qpos, const void *qvel, const void *warm, int nslots) {
  g_err[0] = 0;
  if (!b) return refuse("null DmTraceBufs");
  if (!b->ring || !b->head || !b->cap || !b->cap_meta || !b->cap_count || !b->trig) return refuse("null buffer in DmTraceBufs");
  if (b->N < 1 || b->K < 2 || b->C < 1) return refuse("N < 1, K < 2 or C < 1");
  if (b->nq < 1 || b->nv < 1 || b->na < 1 || b->W != b->nq + 2 * b->nv + b->na + DM_TRACE_TAIL) return refuse("W != nq + 2 nv + na + 5");
  if (!qpos || !qvel || !warm) return refuse("null state pointer");
  if (nslots < 1 || nslots > b->N) return refuse("nslots outside [1, N]");
  if (b->device < 0) return refuse("device < 0");
  return DM_TRACE_OK;
}

int launch_status() {
  if (hipGetLastError() == hipSuccess) return DM_TRACE_OK;
  snprintf(g_err, sizeof g_err, "a launch was refused");
  return DM_TRACE_EHIP;
}

}  // namespace

extern "C" int dm_trace_record(const DmTraceBufs *bufs, const float *qpos, const float *qvel, const float *warm, const float *actions,
                               const float *rew, const uint8_t *done, const int32_t *reason, const int32_t *env_ids, int nslots,
                               uint32_t reason_mask, void *stream) {
  const int rc = check(bufs, qpos, qvel, warm, nslots);
  if (rc != DM_TRACE_OK) return rc;
  if (!actions || !rew || !done || !reason) return refuse("null step output");
  if (hipSetDevice(bufs->device) != hipSuccess) return DM_TRACE_EHIP;
  const TraceIn in = {qpos, qvel, warm, actions, rew, done, reason, env_ids, nslots, DM_TRACE_KIND_STEP, reason_mask};
  hipLaunchKernelGGL(trace_write_kernel, dim3((nslots + TW_WAVES - 1) / TW_WAVES), dim3(TW_BLOCK), 0, (hipStream_t)stream, *bufs, in);
  hipLaunchKernelGGL(trace_capture_kernel, dim3(1), dim3(TC_BLOCK), 0, (hipStream_t)stream, *bufs);
  return launch_status();
}

extern "C" int dm_trace_mark(const DmTraceBufs *bufs, const float *qpos, const float *qvel, const float *warm, const int32_t *env_ids,
                             int nslots, void *stream) {
  const int rc = check(bufs, qpos, qvel, warm, nslots);
  if (rc != DM_TRACE_OK) return rc;
  if (hipSetDevice(bufs->device) != hipSuccess) return DM_TRACE_EHIP;
  const TraceIn in = {qpos, qvel, warm, nullptr, nullptr, nullptr, nullptr, env_ids, nslots, DM_TRACE_KIND_MARK, 0u};
  hipLaunchKernelGGL(trace_write_kernel, dim3((nslots + TW_WAVES - 1) / TW_WAVES), dim3(TW_BLOCK), 0, (hipStream_t)stream, *bufs, in);
  return launch_status();
}

extern "C" const char *dm_trace_last_error(void) { return g_err; }
