// What the wide learners share beyond the fragment order of dm_wide_frag.h: the constants, the pack kernel, the loss section of the
// chain, the weight-gradient kernel and the host launcher.  dm_ppo_wide.hip carries every bf16 array as ONE plane, dm_ppo_wide3.hip
// as TWO (x = hi + lo, plane 0 = hi, plane 1 = lo at the one-plane element count); the code here is templated on that plane count
// P and on nothing else.  The chains (*_fwdbwd_kernel: tilings, ring depths, LDS layouts) stay in their files, and so do the
// __global__ entry points, a few lines each: their names are what profiles and rocprof commands show.
#ifndef DM_WIDE_COMMON_H
#define DM_WIDE_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dm_bf16.h"
#include "dm_launch.h"
#include "dm_ppo_common.h"
#include "dm_wide_frag.h"      // wide_b8, wide_f16, wide_f2bf, wide_pk2, wide_row, wide_frag, wide_ldfrag

namespace {

#ifdef WIDE_PROFILE   // diagnostic build: s_memtime at the phase boundaries of workgroup 0 (thread 0), printed at the end
#define WPROF(k) do { if (tid == 0 && blockIdx.x == 0) wprof[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define WPROF(k) do {} while (0)
#endif
constexpr int WIDE_BIAS_WGRAD_H1 = 512; // from this first-layer width up the bias gradients come from the weight-gradient launch
constexpr int WIDE_WG_WAVES = 4;        // waves of a weight-gradient workgroup: each takes a quarter of the workgroup's batch slice
constexpr int WIDE_MAX_SPLITK = 8;      // more slices than this and the fp32 atomics into one tile queue up (sk = 64 on a [256,128] net: 46 us)
constexpr int WIDE_R = 32, WIDE_NW = 8, WIDE_THREADS = 64 * WIDE_NW, WIDE_PART = 40;

// ---- the split rule of the two-plane learner (dm_ppo_wide3.hip, file header), the one place
__device__ __forceinline__ void wide3_split(float x, unsigned short &hi, unsigned short &lo) {
  hi = wide_f2bf(x);
  lo = wide_f2bf(x - bf16_widen(hi));
}
// two values at once: hi / lo as packed pairs (low half = a)
__device__ __forceinline__ void wide3_split2(float a, float b, unsigned &hi, unsigned &lo) {
  hi = wide_pk2(a, b);
  lo = wide_pk2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
__device__ __forceinline__ float wide3_join(unsigned short hi, unsigned short lo) { return bf16_widen(hi) + bf16_widen(lo); }

// ------------------------------------------------------------------------------------------------ pack
struct WidePackArgs {
  const float *W[2][3];
  unsigned short *pk[2];          // per trunk: W1 [H1][Dp] | W2 [H2][H1] | W2T [H1][H2] | W3 [32][H2] | W3T [H2][32], each in fragment order; plane by plane
  int D, Dp, H1, H2, A[2];
  long long total;                // elements of one PLANE of one trunk's packed block
  int pack_blocks;                // blocks [0, 2 * pack_blocks) pack, block 2 * pack_blocks = statistics, the rest clear zero_ptr
  const float *adv; int B, normalize; float *stats, *out8;
  float *zero_ptr; long long zero_floats; float *adam_state2;
};

template <int P>
__device__ __forceinline__ void wide_pack_body(const WidePackArgs &a) {
  const int blk = blockIdx.x;
  if (blk == 2 * a.pack_blocks) {
    if (a.B <= 8192) mlp_adv_stats(a.adv, a.B, a.normalize, a.stats, a.out8);     // every load in flight at once
    else ppo_prepare_body(a.adv, a.B, a.normalize, a.stats, a.out8, nullptr, 0);
    if (a.adam_state2 && threadIdx.x == 0) { a.adam_state2[0] = 0.f; a.adam_state2[1] += 1.f; }     // Adam's begin
    return;
  }
  if (blk > 2 * a.pack_blocks) {
    const long long i = ((long long)(blk - 2 * a.pack_blocks - 1) * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int c = 0; c < 4; c++) if (i + c < a.zero_floats) a.zero_ptr[i + c] = 0.f;
    return;
  }
  const int t = blk / a.pack_blocks;
  const long long n1 = (long long)a.H1 * a.Dp, n2 = (long long)a.H2 * a.H1, n3 = 32ll * a.H2;
  // one thread per 16-byte fragment (8 consecutive k of one row n) of each plane, every block in fragment order
  for (long long c = (long long)(blk % a.pack_blocks) * 256 + threadIdx.x; c < (a.total >> 3); c += (long long)a.pack_blocks * 256) {
    long long i = c << 3;
    int which, nks;
    if (i < n1) { which = 0; nks = a.Dp >> 4; }
    else if (i < n1 + n2) { which = 1; nks = a.H1 >> 4; i -= n1; }
    else if (i < n1 + 2 * n2) { which = 2; nks = a.H2 >> 4; i -= n1 + n2; }
    else if (i < n1 + 2 * n2 + n3) { which = 3; nks = a.H2 >> 4; i -= n1 + 2 * n2; }
    else { which = 4; nks = 2; i -= n1 + 2 * n2 + n3; }
    const long long ch = i >> 3;
    const int l = (int)(ch & 63), ks = (int)((ch >> 6) % nks), tt = (int)((ch >> 6) / nks);
    const int n = tt * 32 + (l & 31), k0 = ks * 16 + 8 * (l >> 5);
    unsigned short o[P][8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int k = k0 + j;
      float v;
      switch (which) {
        case 0: v = k < a.D ? a.W[t][0][(size_t)n * a.D + k] : 0.f; break;                 // W1 [H1][Dp]
        case 1: v = a.W[t][1][(size_t)n * a.H1 + k]; break;                                // W2 [H2][H1]
        case 2: v = a.W[t][1][(size_t)k * a.H1 + n]; break;                                // W2^T [H1][H2]
        case 3: v = n < a.A[t] ? a.W[t][2][(size_t)n * a.H2 + k] : 0.f; break;             // W3 [32][H2]
        default: v = k < a.A[t] ? a.W[t][2][(size_t)k * a.H2 + n] : 0.f; break;            // W3^T [H2][32]
      }
      if constexpr (P == 1) o[0][j] = wide_f2bf(v);
      else wide3_split(v, o[0][j], o[1][j]);
    }
    uint4 u[P];
#pragma unroll
    for (int pl = 0; pl < P; pl++) {
      u[pl].x = o[pl][0] | ((unsigned)o[pl][1] << 16); u[pl].y = o[pl][2] | ((unsigned)o[pl][3] << 16);
      u[pl].z = o[pl][4] | ((unsigned)o[pl][5] << 16); u[pl].w = o[pl][6] | ((unsigned)o[pl][7] << 16);
    }
#pragma unroll
    for (int pl = 0; pl < P; pl++) *reinterpret_cast<uint4 *>(a.pk[t] + pl * a.total + (c << 3)) = u[pl];
  }
}

// ------------------------------------------------------------------------------------------------ loss section of the chain
// the head's eight K-slices of the 32 x 32 output (red, [wave][register][lane]) -> outs [32][33], + bias
__device__ __forceinline__ void wide_head_sum(const float *red, float *outs, const float *b3, const int At, const int tid) {
  for (int e = tid; e < 1024; e += WIDE_THREADS) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WIDE_NW; w++) s += red[w * 1024 + e];
    const int l = e & 63, j = e >> 6, n = l & 31;
    outs[wide_row(j, l >> 5) * 33 + n] = s + (n < At ? b3[n] : 0.f);
  }
  __syncthreads();
}

// loss (arithmetic of ppo_loss_kernel) of the workgroup's 32 rows from outs: a half-wave per row, lane = action index; d out -> the
// P planes of dZ3s (LDS, row stride S3 bytes, planes WIDE_R * S3 bytes apart) and, transposed, of dz3T; the workgroup's 36 partial
// sums -> part; on narrow nets the head's bias gradient.  Args: the chain's argument struct (WideArgs / Wide3Args).
template <int P, class Args>
__device__ __forceinline__ void wide_loss_rows(const Args &a, const int trunk, const int tile, const int At, const int tid, const float *outs, float *accs,
                                               char *dZ3s, const int S3) {
  const int nt = a.B / WIDE_R, b0 = tile * WIDE_R, P3 = WIDE_R * S3;
  const size_t B = (size_t)a.B, pl3 = 32 * B;
  {
    const int j = tid & 31, hw = tid >> 5;                    // 16 half-waves, two rows each
    const bool ja = j < a.A;
    const float invB = 1.0f / (float)a.B, amean = a.stats[0], ainv = a.stats[1];
    float g_ls = 0.f, pg = 0.f, vl = 0.f, kl = 0.f, cf = 0.f;
    float ls = 0.f, iv = 0.f, lconst = 0.f;
    if (trunk == 0) {
      ls = ja ? a.log_std[j] : 0.f;
      iv = ja ? expf(-2.f * ls) : 0.f;
      float sum_ls = ls;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sum_ls += __shfl_xor(sum_ls, o);
      lconst = -sum_ls - 0.5f * 1.8378770664093453f * (float)a.A;
    }
    for (int m = hw; m < WIDE_R; m += 16) {
      const int b = b0 + m;
      float dz = 0.f;
      if (trunk == 0) {
        const float d = ja ? a.act[(size_t)b * a.A + j] - outs[m * 33 + j] : 0.f;
        const float z2 = d * d * iv;
        float zs = z2;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) zs += __shfl_xor(zs, o);
        const float logp = -0.5f * zs + lconst;
        const float a_n = (a.adv[b] - amean) * ainv;
        const float lr = logp - a.old_logp[b];
        const float ratio = expf(lr);
        const float rc = fminf(fmaxf(ratio, 1.f - a.clip), 1.f + a.clip);
        const float p1 = a_n * ratio, p2 = a_n * rc;
        const bool inside = (ratio >= 1.f - a.clip) && (ratio <= 1.f + a.clip);
        const float dr = (inside || p1 < p2) ? a_n : 0.f;
        const float dlogp = -invB * dr * ratio;
        dz = ja ? dlogp * d * iv : 0.f;
        g_ls += ja ? dlogp * (z2 - 1.f) : 0.f;
        if (j == 0) { pg += -fminf(p1, p2); kl += (ratio - 1.f) - lr; cf += (fabsf(ratio - 1.f) > a.clip) ? 1.f : 0.f; }
      } else {
        const float dv = outs[m * 33] - a.ret[b];
        dz = (j == 0) ? a.vf_coef * 2.f * invB * dv : 0.f;
        if (j == 0) vl += dv * dv;
      }
      unsigned short dzb[P];
      if constexpr (P == 1) dzb[0] = wide_f2bf(dz);
      else wide3_split(dz, dzb[0], dzb[1]);
#pragma unroll
      for (int pl = 0; pl < P; pl++) *reinterpret_cast<unsigned short *>(dZ3s + pl * P3 + m * S3 + 2 * j) = dzb[pl];
      const size_t at = wide_frag(j, b, (int)(B >> 4));
#pragma unroll
      for (int pl = 0; pl < P; pl++) a.dz3T[trunk][pl * pl3 + at] = dzb[pl];
    }
    accs[hw * 36 + j] = g_ls;
    if (j == 0) { accs[hw * 36 + 32] = pg; accs[hw * 36 + 33] = vl; accs[hw * 36 + 34] = kl; accs[hw * 36 + 35] = cf; }
  }
  __syncthreads();
  if (tid < 36) {   // this workgroup's partial sums (summed in fixed order by block 0 of the weight-gradient launch)
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) t += accs[i * 36 + tid];
    a.part[((size_t)trunk * nt + tile) * WIDE_PART + tid] = t;
  }
  // bias gradients = column sums of dZ (of hi + lo with two planes).  Wide nets: the weight-gradient launch forms them with one more
  // MFMA per k-step and plane against a fragment of ones (128 workgroups adding 32-row partial sums to the same 1 024 addresses from
  // here cost d layer 1 ~15 % of its time: 117.5 -> 112.4 us per optimizer step); narrow nets keep the sums here (their few
  // weight-gradient tiles would carry the extra MFMAs on the critical path: [256,128] 59.6 -> 65.2 us)
  if (a.bias_in_chain && tid < At) {
    float s = 0.f;
    for (int m = 0; m < WIDE_R; m++) {
      const char *zp = dZ3s + m * S3 + 2 * tid;
      if constexpr (P == 1) s += bf16_widen(*reinterpret_cast<const unsigned short *>(zp));
      else s += wide3_join(*reinterpret_cast<const unsigned short *>(zp), *reinterpret_cast<const unsigned short *>(zp + P3));
    }
    atomicAdd(&a.gb3[trunk][tid], s);
  }
}

// ------------------------------------------------------------------------------------------------ weight gradients
// dW = dZ^T X for the six layers.  Operands are the TRANSPOSED arrays the chain wrote, in fragment order: AT = dZ^T (O x B),
// XT = X^T (I x B): a wave's fragment load is 1 KB of consecutive bytes, the k-steps of a tile follow each other.  A workgroup of
// four waves owns four 32 x 32 tiles of dW — 64 x 64 (RO = CI = 2), or 32 x 128 for the heads (RO = 1) — and the whole batch (or
// 1 / splitk of it on small nets): every wave accumulates all four tiles over its quarter of the batch rows, the four partial
// blocks meet in LDS (64 KB: two workgroups per CU) and each wave finishes one tile — added to dW by its one owner when splitk == 1: no atomics,
// fixed summation order.  With two planes a tile and k-step take three MFMAs (lo.hi, hi.lo, hi.hi into one accumulator) and the
// bias gradient one MFMA per plane of dZ^T.  Measured on the way (us per optimizer step of the bf16 [1024,512] learner, 4 096 rows):
//   one wave per 32 x 128, four waves per workgroup re-reading X                                         216
//   one wave per 128 x 128 (16 accumulators: 928 spilled VGPRs)                                            375
//   one wave per 64 x 128, split-K 4-16 over workgroups with fp32 atomics                                  185 -> 132.6 (fragment order)
//   four waves per 64 x 128 splitting the batch inside the workgroup, no atomics (128 KB LDS: 164 workgroups)  125.6
//   ... with global split-K 2 on top (292 workgroups, atomics back)                                        136.2
//   four waves per 64 x 64, 64 KB LDS, two workgroups per CU (328 workgroups), two-k-step ring             122.7  <- this
// Block 0 sums the loss partials (fixed order).
template <int P> struct WideWgradIn { const unsigned short *AT, *XT; long long apl, xpl; };      // apl, xpl: elements of one plane of AT, XT
template <> struct WideWgradIn<1> { const unsigned short *AT, *XT; };
template <int P> struct WideWgradJob : WideWgradIn<P> { float *dW, *db; int O, I, ldw, ro, otiles, itiles, splitk, first, per; };
template <int P> struct WideWgradArgs {
  WideWgradJob<P> j[6];
  int njobs, nblocks, B;
  const float *part; int nblk, A; const float *log_std; float vf_coef, ent_coef; const float *stats; float *g_log_std, *out8, *loss_acc;
};

// KB: k-steps of a ring block (bf16: 2; a four-k-step ring: 126.0 against 122.7 us per optimizer step.  Two planes: 1, both planes
// of RO + CI fragments being 32 or 40 VGPRs a block already)
template <int P, int KB, int RO, int CI>
__device__ __forceinline__ void wide_wgrad_tile(const WideWgradJob<P> &J, const int Bn, const int ot, const int it, const int ks, const int wave,
                                                const int lane, float *wl) {
  constexpr int NT = RO * CI;                    // 32 x 32 tiles of dW per wave (a multiple of 4)
  const int r = lane & 31, h = lane >> 5;
  const int o0 = ot * 32 * RO, i0 = it * 32 * CI;
  const size_t B = (size_t)Bn;
  // batch rows of this workgroup's split, in units of 64 rows; the four waves take a quarter of the units each
  const int units = (Bn / J.splitk) >> 6, u0 = wave * units / WIDE_WG_WAVES, u1 = (wave + 1) * units / WIDE_WG_WAVES;
  const int k0 = ks * (Bn / J.splitk) + u0 * 64;
  const size_t tstride = (B >> 4) * 512;                        // elements of one 32-feature tile: (B / 16) k-steps of 512
  const unsigned short *ap = J.AT + (size_t)(o0 >> 5) * tstride + ((size_t)(k0 >> 4) * 64 + lane) * 8;
  const unsigned short *xp = J.XT + (size_t)(i0 >> 5) * tstride + ((size_t)(k0 >> 4) * 64 + lane) * 8;
  size_t apl = 0, xpl = 0;
  if constexpr (P == 2) { apl = (size_t)J.apl; xpl = (size_t)J.xpl; }
  bool oa[RO], ia[CI];
#pragma unroll
  for (int p = 0; p < RO; p++) oa[p] = (o0 + 32 * p + r) < J.O;
#pragma unroll
  for (int q = 0; q < CI; q++) ia[q] = (i0 + 32 * q + r) < J.I;
  wide_f16 acc[RO][CI];
#pragma unroll
  for (int p = 0; p < RO; p++)
#pragma unroll
    for (int q = 0; q < CI; q++)
#pragma unroll
      for (int j = 0; j < 16; j++) acc[p][q][j] = 0.f;
  // bias gradient db = dZ^T 1: the workgroups of the first input tile multiply their dZ^T fragments by a fragment of ones as well
  // (every column of that 32 x 32 product is the row sum; bf16 1.0 = 0x3F80)
  const bool bias = J.db != nullptr && it == 0;
  const wide_b8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  wide_f16 accb[RO];
#pragma unroll
  for (int p = 0; p < RO; p++)
#pragma unroll
    for (int j = 0; j < 16; j++) accb[p][j] = 0.f;
  const wide_b8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // two-deep ring of register blocks of KB k-steps: the loads of the next block are in flight under the MFMAs of this one
  wide_b8 av[RO][KB][P], xv[CI][KB][P], aw[RO][KB][P], xw[CI][KB][P];
  auto load_blk = [&](wide_b8 (&A_)[RO][KB][P], wide_b8 (&X_)[CI][KB][P], const int kk) {
#pragma unroll
    for (int i = 0; i < KB; i++) {
#pragma unroll
      for (int p = 0; p < RO; p++)
#pragma unroll
        for (int pl = 0; pl < P; pl++) A_[p][i][pl] = oa[p] ? *reinterpret_cast<const wide_b8 *>(ap + pl * apl + p * tstride + (size_t)(kk + i) * 512) : zero;
#pragma unroll
      for (int q = 0; q < CI; q++)
#pragma unroll
        for (int pl = 0; pl < P; pl++) X_[q][i][pl] = ia[q] ? *reinterpret_cast<const wide_b8 *>(xp + pl * xpl + q * tstride + (size_t)(kk + i) * 512) : zero;
    }
  };
  auto mma_blk = [&](const wide_b8 (&A_)[RO][KB][P], const wide_b8 (&X_)[CI][KB][P]) {
#pragma unroll
    for (int i = 0; i < KB; i++) {
      if constexpr (P == 2) {
#pragma unroll
        for (int p = 0; p < RO; p++)
#pragma unroll
          for (int q = 0; q < CI; q++) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_[p][i][1], X_[q][i][0], acc[p][q], 0, 0, 0);
#pragma unroll
        for (int p = 0; p < RO; p++)
#pragma unroll
          for (int q = 0; q < CI; q++) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_[p][i][0], X_[q][i][1], acc[p][q], 0, 0, 0);
      }
#pragma unroll
      for (int p = 0; p < RO; p++)
#pragma unroll
        for (int q = 0; q < CI; q++) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_[p][i][0], X_[q][i][0], acc[p][q], 0, 0, 0);
    }
    if (bias) {
#pragma unroll
      for (int i = 0; i < KB; i++)
#pragma unroll
        for (int pl = P - 1; pl >= 0; pl--)
#pragma unroll
          for (int p = 0; p < RO; p++) accb[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_[p][i][pl], ones, accb[p], 0, 0, 0);
    }
  };
  const int nks = (u1 - u0) * 4;                     // k-steps of 16 rows: a multiple of 4 (of 2 KB), possibly 0
  if (nks > 0) load_blk(av, xv, 0);
  for (int kk = 0; kk < nks; kk += 2 * KB) {
    // nks % 4 == 0, so a round's second block always exists; only one-k-step rings say so to the compiler (for KB = 2 dropping the
    // test moves 1 900 of wide_wgrad_kernel's 4 274 instructions, which are held to what was measured)
    const bool second = KB == 1 || kk + KB < nks;
    if (second) load_blk(aw, xw, kk + KB);
    mma_blk(av, xv);
    if (kk + 2 * KB < nks) load_blk(av, xv, kk + 2 * KB);
    if (second) mma_blk(aw, xw);
  }
  if (bias && r == 0) {
#pragma unroll
    for (int p = 0; p < RO; p++)
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int row = o0 + 32 * p + wide_row(j, h);
        if (row < J.O) atomicAdd(&J.db[row], accb[p][j]);      // 4 waves x splitk adds per address
      }
  }
  // the four partial blocks meet in LDS, four tiles at a time ([wave][tile][register][lane]: lane-contiguous, conflict-free); wave w
  // then owns tile 4 ph + w: fixed summation order, and with splitk == 1 a plain add by the tile's one owner (no atomics, bit-reproducible gradients)
#pragma unroll
  for (int ph = 0; ph < NT / 4; ph++) {
    if (ph) __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
      const int t = 4 * ph + tt;
#pragma unroll
      for (int j = 0; j < 16; j++) wl[((wave * 4 + tt) << 10) + j * 64 + lane] = acc[t / CI][t % CI][j];
    }
    const int t = 4 * ph + wave, p = t / CI, q = t % CI;
    const bool live = (i0 + 32 * q + r) < J.I;
    // gradients are ACCUMULATED (deepmimic_hip.h), also where a tile has one owner: its present values are requested before the
    // barrier, so the round trip passes under the LDS exchange
    float old[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int row = o0 + 32 * p + wide_row(j, h);
      old[j] = (J.splitk == 1 && live && row < J.O) ? J.dW[(size_t)row * J.ldw + i0 + 32 * q + r] : 0.f;
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WIDE_WG_WAVES; w++) v += wl[((w * 4 + wave) << 10) + j * 64 + lane];
        const int row = o0 + 32 * p + wide_row(j, h);
        if (row < J.O) {
          float *dst = &J.dW[(size_t)row * J.ldw + i0 + 32 * q + r];
          if (J.splitk == 1) *dst = old[j] + v; else atomicAdd(dst, v);
        }
      }
    }
  }
}

// wl: the workgroup's dynamic LDS, 4 waves x 4 tiles x 4 KB
template <int P, int KB>
__device__ __forceinline__ void wide_wgrad_body(const WideWgradArgs<P> &a, float *wl) {
  const int blk = (int)blockIdx.x - 1, tid = threadIdx.x;
  if (blk < 0) {   // block 0 (dispatched first): loss scalars and the log_std gradient from the per-workgroup partials, in a fixed order
    // thread l sums the rows l, l + 256, .. of a trunk's [nblk][40] table (ten independent 16-byte loads per row: the loads of
    // all rows are in flight together; a first version walked the rows with 36 lanes and paid ~32 dependent L2 misses: 40 us,
    // the whole launch's length for a small net), the 64 lane sums meet in LDS
    __shared__ float red[2][36];
    float (*lsum)[41] = reinterpret_cast<float (*)[41]>(wl);      // [256][41]
    const float *part = a.part;      // both read once, ahead of the row loops
    const int nblk = a.nblk;
    for (int t = 0; t < 2; t++) {
      float acc[WIDE_PART];
#pragma unroll
      for (int e = 0; e < WIDE_PART; e++) acc[e] = 0.f;
      for (int i = tid; i < nblk; i += 64 * WIDE_WG_WAVES) {
        const float4 *row = reinterpret_cast<const float4 *>(part + ((size_t)t * nblk + i) * WIDE_PART);
#pragma unroll
        for (int e = 0; e < WIDE_PART / 4; e++) { const float4 v = row[e]; acc[4 * e] += v.x; acc[4 * e + 1] += v.y; acc[4 * e + 2] += v.z; acc[4 * e + 3] += v.w; }
      }
#pragma unroll
      for (int e = 0; e < 36; e++) lsum[tid][e] = acc[e];
      __syncthreads();
      if (tid < 36) {
        float s0 = 0.f;
        for (int l = 0; l < 64 * WIDE_WG_WAVES; l++) s0 += lsum[l][tid];
        red[t][tid] = s0;
      }
      __syncthreads();
    }
    __syncthreads();
    if (tid < a.A) a.g_log_std[tid] += red[0][tid] - a.ent_coef;
    if (tid == 0) {
      const float invB = 1.0f / (float)a.B;
      float ent = 0.f;
      for (int j = 0; j < a.A; j++) ent += 0.5f + 0.5f * 1.8378770664093453f + a.log_std[j];
      const float pg = red[0][32] * invB, vl = red[1][33] * invB;
      a.out8[1] = pg; a.out8[2] = vl; a.out8[3] = ent; a.out8[4] = red[0][34] * invB; a.out8[5] = red[0][35] * invB;
      a.out8[0] = pg + a.vf_coef * vl - a.ent_coef * ent;
      a.out8[6] = a.stats[0]; a.out8[7] = a.stats[1];
      if (a.loss_acc) { a.loss_acc[0] += a.out8[0]; a.loss_acc[1] += 1.f; }
    }
    return;
  }
  int jq = 0;
  for (int i = 1; i < a.njobs; i++) if (blk >= a.j[i].first) jq = i;
  const WideWgradJob<P> &J = a.j[jq];
  // workgroups go round the eight XCDs in launch order.  A job's tiles are numbered (split, output tile, input tile), input tile
  // fastest, and XCD x takes the x-th eighth of that order: the workgroups that read one slice of the batch — and, inside it, one
  // block of dZ^T rows — share an L2, which then holds their operands once (dW2 of a trunk: 2.5 MB per XCD)
  const int loc = blk - J.first;
  int rem = (loc & 7) * J.per + (loc >> 3);
  if ((loc >> 3) >= J.per || rem >= J.splitk * J.otiles * J.itiles) return;
  const int it = rem % J.itiles; rem /= J.itiles;
  const int ot = rem % J.otiles, ks = rem / J.otiles;
  if (J.ro == 2) wide_wgrad_tile<P, KB, 2, 2>(J, a.B, ot, it, ks, tid >> 6, tid & 63, wl);
  else wide_wgrad_tile<P, KB, 1, 4>(J, a.B, ot, it, ks, tid >> 6, tid & 63, wl);
}

// ------------------------------------------------------------------------------------------------ host
inline int wide_dp(int D) { return (D + 15) & ~15; }
inline long long wide_plane_elems(int D, int H1, int H2) { return (long long)H1 * wide_dp(D) + 2ll * H2 * H1 + 64ll * H2; }     // one plane of a trunk's packed block
inline bool wide_pointers_ok(const DmPpoWideStep *s) {
  if (!s->obs || !s->act || !s->adv || !s->ret || !s->old_logp || !s->log_std || !s->g_log_std || !s->xbT || !s->part || !s->stats8 || !s->out8) return false;
  for (int t = 0; t < 2; t++) {
    if (!s->wpk[t] || !s->h1T[t] || !s->dz1T[t] || !s->h2T[t] || !s->dz2T[t] || !s->dz3T[t]) return false;
    for (int l = 0; l < 3; l++) if (!s->W[t][l] || !s->b[t][l] || !s->gW[t][l] || !s->gb[t][l]) return false;
  }
  return true;
}

// The three launches of one minibatch (plain, stream-ordered, capturable) for a SUPPORTED shape.  ChainArgs: the chain's argument
// struct; lds: the chain's dynamic LDS bytes.
template <int P, class ChainArgs>
int wide_launch(const DmPpoWideStep *s, hipStream_t st, void (*pack)(WidePackArgs), void (*chain)(ChainArgs), void (*wgrad)(WideWgradArgs<P>), const int lds) {
  if (!wide_pointers_ok(s)) return DM_EINVAL;
  static int lds_set_for = -1;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return DM_EHIP;
  if (lds_set_for != dev) {   // per device, outside capture: the warm-up calls before a capture pass here
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(chain), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return DM_EHIP;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(wgrad), hipFuncAttributeMaxDynamicSharedMemorySize, WIDE_WG_WAVES * 4 * 4096) != hipSuccess) return DM_EHIP;
    lds_set_for = dev;
  }
  const int Dp = wide_dp(s->D);
  const long long total = wide_plane_elems(s->D, s->H1, s->H2);
  WidePackArgs p;
  memset(&p, 0, sizeof p);
  for (int t = 0; t < 2; t++) { for (int l = 0; l < 3; l++) p.W[t][l] = s->W[t][l]; p.pk[t] = (unsigned short *)s->wpk[t]; }
  p.D = s->D; p.Dp = Dp; p.H1 = s->H1; p.H2 = s->H2; p.A[0] = s->A; p.A[1] = 1;
  p.total = total;
  p.pack_blocks = 1152;      // ~one 16-byte fragment (of each plane) per thread for the [1024,512] net (256 blocks: 11.4 us, the loop serialised four strided reads per thread)
  p.adv = s->adv; p.B = s->B; p.normalize = s->normalize_advantage; p.stats = s->stats8; p.out8 = s->out8;
  p.zero_ptr = s->zero_ptr; p.zero_floats = s->zero_ptr ? s->zero_floats : 0; p.adam_state2 = s->adam_state2;
  const int zero_blocks = (int)((p.zero_floats + 1023) / 1024);
  hipLaunchKernelGGL(pack, dim3(2 * p.pack_blocks + 1 + zero_blocks), dim3(256), 0, st, p);
  ChainArgs a;
  memset(&a, 0, sizeof a);
  a.B = s->B; a.D = s->D; a.Dp = Dp; a.H1 = s->H1; a.H2 = s->H2; a.A = s->A;
  if constexpr (P == 2) a.total = total;
  a.obs = s->obs; a.act = s->act; a.adv = s->adv; a.ret = s->ret; a.old_logp = s->old_logp; a.log_std = s->log_std; a.stats = s->stats8;
  for (int t = 0; t < 2; t++) {
    a.pk[t] = (const unsigned short *)s->wpk[t];
    a.b1[t] = s->b[t][0]; a.b2[t] = s->b[t][1]; a.b3[t] = s->b[t][2];
    a.gb1[t] = s->gb[t][0]; a.gb2[t] = s->gb[t][1]; a.gb3[t] = s->gb[t][2];
    a.h1T[t] = (unsigned short *)s->h1T[t]; a.dz1T[t] = (unsigned short *)s->dz1T[t]; a.h2T[t] = (unsigned short *)s->h2T[t];
    a.dz2T[t] = (unsigned short *)s->dz2T[t]; a.dz3T[t] = (unsigned short *)s->dz3T[t];
  }
  a.xbT = (unsigned short *)s->xbT; a.part = s->part; a.clip = s->clip_range; a.vf_coef = s->vf_coef;
  const bool bias_wgrad = s->H1 >= WIDE_BIAS_WGRAD_H1;
  a.bias_in_chain = bias_wgrad ? 0 : 1;
  hipLaunchKernelGGL(chain, dim3(2 * (s->B / WIDE_R)), dim3(WIDE_THREADS), lds, st, a);
  // weight gradients: per trunk dW2 (the big one), dW1, dW3; split-K chosen so that every job brings ~64-128 workgroups.
  // AN / XN: rows of the transposed operands, whose planes are rows x B elements each
  WideWgradArgs<P> g;
  memset(&g, 0, sizeof g);
  int first = 0, nj = 0;
  auto add = [&](const void *AT, int AN, const void *XT, int XN, float *dW, float *db, int O, int I, int ldw, int ro, int want) {
    WideWgradJob<P> &J = g.j[nj++];
    J.AT = (const unsigned short *)AT; J.XT = (const unsigned short *)XT; J.dW = dW; J.db = db; J.O = O; J.I = I; J.ldw = ldw; J.ro = ro;
    if constexpr (P == 2) { J.apl = (long long)AN * s->B; J.xpl = (long long)XN * s->B; }
    J.otiles = (O + 32 * ro - 1) / (32 * ro);
    J.itiles = (I + 32 * (4 / ro) - 1) / (32 * (4 / ro));
    int sk = 1;
    while (sk < WIDE_MAX_SPLITK && J.otiles * J.itiles * sk * 2 <= want && (s->B / (sk * 2)) % 64 == 0) sk *= 2;     // want: workgroups
    J.splitk = sk; J.first = first;                       // first % 8 == 0: a job's local block id & 7 is its XCD
    J.per = (J.otiles * J.itiles * sk + 7) / 8;
    first += 8 * J.per;
  };
  for (int t = 0; t < 2; t++) {
    add(s->dz2T[t], s->H2, s->h1T[t], s->H1, s->gW[t][1], bias_wgrad ? s->gb[t][1] : nullptr, s->H2, s->H1, s->H1, 2, 128);
    add(s->dz1T[t], s->H1, s->xbT, (Dp + 31) & ~31, s->gW[t][0], bias_wgrad ? s->gb[t][0] : nullptr, s->H1, s->D, s->D, 2, 32);
    add(s->dz3T[t], 32, s->h2T[t], s->H2, s->gW[t][2], bias_wgrad ? s->gb[t][2] : nullptr, t ? 1 : s->A, s->H2, s->H2, 1, 4);
  }
  g.njobs = nj; g.nblocks = first; g.B = s->B;
  g.part = s->part; g.nblk = s->B / WIDE_R; g.A = s->A; g.log_std = s->log_std; g.vf_coef = s->vf_coef; g.ent_coef = s->ent_coef; g.stats = s->stats8;
  g.g_log_std = s->g_log_std; g.out8 = s->out8; g.loss_acc = s->loss_acc;
  hipLaunchKernelGGL(wgrad, dim3(first + 1), dim3(64 * WIDE_WG_WAVES), WIDE_WG_WAVES * 4 * 4096, st, g);
  return dm_launch_status();
}

}  // namespace
#endif
