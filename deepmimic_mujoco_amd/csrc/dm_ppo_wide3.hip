// One PPO minibatch of the WIDE actor-critic MLP (net_arch = [1024, 512]) at fp32 accuracy on the bf16 matrix pipe ("bf16x3").
//
// Reference: src/sb3_ppo.py:254-271,307-312 -> [EXT] SB3 PPO.train on MlpPolicy, an fp32 learner.  dm_ppo_wide.hip carries bf16
// operands (gradients 0.5-1 % from the unrounded chain); the exact fp32 MFMA runs at the vector rate.  Here every operand of every
// product is SPLIT, x = hi + lo with
//     hi = rne_bf16(x),  lo = rne_bf16(x - float(hi))        (the subtraction is exact in fp32; so is float(hi) + float(lo))
// and a product is three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator: hi.hi + hi.lo + lo.hi; lo.lo (<= 2^-18 relative) is never
// formed.  Rounding points are those of dm_ppo_wide.hip, each now a split: observations, every weight in the five packed layouts,
// h1 and h2 after tanh, dZ3, dZ2, dZ1.  Every non-matrix use of an operand (tanh' = 1 - h^2, the column sums) sees hi + lo.  Head
// output, loss arithmetic, gradients, master weights and Adam are fp32.
//
// Launches (plain, stream-ordered, capturable; the structure of dm_ppo_wide.hip):
//   1. wide3_pack_kernel    fp32 weights -> two bf16 planes in the five fragment-order layouts; advantage statistics; optional folds
//   2. wide3_fwdbwd_kernel  eight waves carry 32 minibatch rows of one trunk forward, through the loss, and back
//   3. wide3_wgrad_kernel   dW = dZ^T X of the six layers from the transposed two-plane arrays the chain left; loss scalars (block 0)
// Every two-plane array is plane 0 (hi) followed by plane 1 (lo) at the one-plane element count, each in the fragment order of
// dm_wide_frag.h.
//
// LDS of the chain.  Two planes of the bf16 kernel's 32 rows of X, H1, H2, dZ2, dZ3 do not fit in 160 KB at [1024,512].  So:
//   * layer 1 is produced in CHUNKS of 256 columns (eight 32-column tiles: one per wave; 33 KB for both planes) and layer 2's
//     accumulators — at most two 32 x 32 tiles per wave (H2 <= 512), held in registers across the chunks — consume each chunk at once;
//   * dZ2 is written IN PLACE over H2 (the lane that owns an accumulator element reads h2 and writes dz2 at that element);
//   * dZ1 goes straight to global memory, and layer 1's tanh' reads the h1T planes this workgroup wrote itself (global, L2-hot);
//   * the head's eight partial tiles reuse the chunk buffer.
// X 15 KB + chunk 33 KB + H2 / dZ2 65 KB + dZ3 5 KB + loss 6.4 KB = 124.4 KB at [1024,512], D = 112; H1 does not enter.
// Bias gradients: H1 >= 512: the weight-gradient launch multiplies BOTH planes of dZ^T by a fragment of ones (column sums of
// hi + lo, fp32 accumulation); H1 < 512: the chain sums its unrounded fp32 dZ2 / dZ1 and the split dZ3, as the bf16 kernel does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dm_bf16.h"
#include "dm_launch.h"
#include "dm_ppo_common.h"
#include "dm_wide_frag.h"

namespace {

// ---- the split rule (file header), the one place
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
// acc += a b without lo.lo
__device__ __forceinline__ wide_f16 wide3_mma(const wide_b8 ah, const wide_b8 al, const wide_b8 bh, const wide_b8 bl, wide_f16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

#ifdef WIDE_PROFILE   // diagnostic build: s_memtime at the phase boundaries of workgroup 0 (thread 0), printed at the end
#define WPROF(k) do { if (tid == 0 && blockIdx.x == 0) wprof[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define WPROF(k) do {} while (0)
#endif
constexpr int WIDE3_BIAS_WGRAD_H1 = 512; // from this first-layer width up the bias gradients come from the weight-gradient launch
constexpr int WIDE3_WG_WAVES = 4;        // waves of a weight-gradient workgroup: each takes a quarter of the workgroup's batch slice
constexpr int WIDE3_MAX_SPLITK = 8;
constexpr int WIDE3_R = 32, WIDE3_NW = 8, WIDE3_THREADS = 64 * WIDE3_NW, WIDE3_PART = 40;
constexpr int WIDE3_CHUNK = 32 * WIDE3_NW;   // layer-1 columns per chunk: one tile per wave

struct Wide3PackArgs {
  const float *W[2][3];
  unsigned short *pk[2];          // per trunk: W1 [H1][Dp] | W2 [H2][H1] | W2T [H1][H2] | W3 [32][H2] | W3T [H2][32], plane 0 then plane 1
  int D, Dp, H1, H2, A[2];
  long long total;                // elements of one PLANE of one trunk's packed block
  int pack_blocks;                // blocks [0, 2 * pack_blocks) pack, block 2 * pack_blocks = statistics, the rest clear zero_ptr
  const float *adv; int B, normalize; float *stats, *out8;
  float *zero_ptr; long long zero_floats; float *adam_state2;
};

__global__ void __launch_bounds__(256) wide3_pack_kernel(Wide3PackArgs a) {
  const int blk = blockIdx.x;
  if (blk == 2 * a.pack_blocks) {
    if (a.B <= 8192) mlp_adv_stats(a.adv, a.B, a.normalize, a.stats, a.out8);
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
    unsigned short oh[8], ol[8];
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
      wide3_split(v, oh[j], ol[j]);
    }
    uint4 u, w;
    u.x = oh[0] | ((unsigned)oh[1] << 16); u.y = oh[2] | ((unsigned)oh[3] << 16); u.z = oh[4] | ((unsigned)oh[5] << 16); u.w = oh[6] | ((unsigned)oh[7] << 16);
    w.x = ol[0] | ((unsigned)ol[1] << 16); w.y = ol[2] | ((unsigned)ol[3] << 16); w.z = ol[4] | ((unsigned)ol[5] << 16); w.w = ol[6] | ((unsigned)ol[7] << 16);
    *reinterpret_cast<uint4 *>(a.pk[t] + (c << 3)) = u;
    *reinterpret_cast<uint4 *>(a.pk[t] + a.total + (c << 3)) = w;
  }
}

struct Wide3Args {
  int B, D, Dp, H1, H2, A;
  const float *obs, *act, *adv, *ret, *old_logp, *log_std, *stats;
  const unsigned short *pk[2];
  long long total;                 // elements of one plane of a trunk's packed block
  const float *b1[2], *b2[2], *b3[2];
  float *gb1[2], *gb2[2], *gb3[2];
  unsigned short *xbT, *h1T[2], *dz1T[2], *h2T[2], *dz2T[2], *dz3T[2];   // two planes of [features][B] bf16 each
  float *part;
  float clip, vf_coef;
  int bias_in_chain;
};

// four consecutive batch rows row0 .. row0 + 3 (row0 % 4 == 0) of one feature column, split, as 8 bytes of each plane of the transposed
// (features x batch) array in fragment order; pl = elements of one plane
__device__ __forceinline__ void wide3_store_t4(unsigned short *T, size_t pl, size_t B, int col, int row0, float v0, float v1, float v2, float v3) {
  uint2 uh, ul;
  wide3_split2(v0, v1, uh.x, ul.x);
  wide3_split2(v2, v3, uh.y, ul.y);
  const size_t at = wide_frag(col, row0, (int)(B >> 4));
  *reinterpret_cast<uint2 *>(T + at) = uh;
  *reinterpret_cast<uint2 *>(T + pl + at) = ul;
}
// the same four values also into the two LDS planes (rows lrow0 .. lrow0 + 3 of column col, row stride `stride` bytes, lpl bytes per plane)
__device__ __forceinline__ void wide3_put4(char *L, int lpl, int stride, int lrow0, int col, unsigned short *T, size_t pl, size_t B, int gcol, int grow0,
                                           float v0, float v1, float v2, float v3) {
  uint2 uh, ul;
  wide3_split2(v0, v1, uh.x, ul.x);
  wide3_split2(v2, v3, uh.y, ul.y);
  char *p = L + lrow0 * stride + 2 * col;
  *reinterpret_cast<unsigned short *>(p) = (unsigned short)uh.x;
  *reinterpret_cast<unsigned short *>(p + stride) = (unsigned short)(uh.x >> 16);
  *reinterpret_cast<unsigned short *>(p + 2 * stride) = (unsigned short)uh.y;
  *reinterpret_cast<unsigned short *>(p + 3 * stride) = (unsigned short)(uh.y >> 16);
  p += lpl;
  *reinterpret_cast<unsigned short *>(p) = (unsigned short)ul.x;
  *reinterpret_cast<unsigned short *>(p + stride) = (unsigned short)(ul.x >> 16);
  *reinterpret_cast<unsigned short *>(p + 2 * stride) = (unsigned short)ul.y;
  *reinterpret_cast<unsigned short *>(p + 3 * stride) = (unsigned short)(ul.y >> 16);
  const size_t at = wide_frag(gcol, grow0, (int)(B >> 4));
  *reinterpret_cast<uint2 *>(T + at) = uh;
  *reinterpret_cast<uint2 *>(T + pl + at) = ul;
}

// acc[q] += A x (weight tile q) over nks k-steps (a multiple of 2 KB).  A: two LDS planes, this lane's row (ah; + apl bytes for lo;
// + 32 bytes per k-step).  Weights: two planes in L2 (wh for this lane; + wpl elements for lo; + tstride per tile; + 512 per k-step),
// through a two-deep ring of register blocks of KB k-steps: the next block's loads are in flight under this block's MFMAs.
template <int NT, int KB>
__device__ __forceinline__ void wide3_stream(wide_f16 (&acc)[NT], const char *ah, const int apl, const unsigned short *wh, const size_t wpl,
                                             const size_t tstride, const int nks) {
  wide_b8 ph[NT][KB], pl[NT][KB], qh[NT][KB], ql[NT][KB];
  auto ld = [&](wide_b8 (&H)[NT][KB], wide_b8 (&L)[NT][KB], const int k0) {
#pragma unroll
    for (int q = 0; q < NT; q++)
#pragma unroll
      for (int i = 0; i < KB; i++) {
        H[q][i] = *reinterpret_cast<const wide_b8 *>(wh + q * tstride + (size_t)(k0 + i) * 512);
        L[q][i] = *reinterpret_cast<const wide_b8 *>(wh + wpl + q * tstride + (size_t)(k0 + i) * 512);
      }
  };
  auto mm = [&](const wide_b8 (&H)[NT][KB], const wide_b8 (&L)[NT][KB], const int k0) {
#pragma unroll
    for (int i = 0; i < KB; i++) {
      const wide_b8 a_h = *reinterpret_cast<const wide_b8 *>(ah + (k0 + i) * 32);
      const wide_b8 a_l = *reinterpret_cast<const wide_b8 *>(ah + apl + (k0 + i) * 32);
#pragma unroll
      for (int q = 0; q < NT; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l, H[q][i], acc[q], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < NT; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, L[q][i], acc[q], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < NT; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, H[q][i], acc[q], 0, 0, 0);
    }
  };
  ld(ph, pl, 0);
  for (int k = 0; k < nks; k += 2 * KB) {
    ld(qh, ql, k + KB);
    mm(ph, pl, k);
    if (k + 2 * KB < nks) ld(ph, pl, k + 2 * KB);
    mm(qh, ql, k + KB);
  }
}

__global__ void __launch_bounds__(WIDE3_THREADS) wide3_fwdbwd_kernel(Wide3Args a) {
  extern __shared__ __align__(16) char wide3_lds[];
  // workgroups go round the eight XCDs in launch order: even XCDs take the policy trunk, odd ones the value trunk, so an XCD's L2
  // streams ONE trunk's weights
#ifdef WIDE_PROFILE
  unsigned long long wprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  const int nt = a.B / WIDE3_R, id = blockIdx.x;
  int trunk, tile;
  if ((nt & 3) == 0) { const int xcd = id & 7; trunk = xcd & 1; tile = (id >> 3) * 4 + (xcd >> 1); }
  else { trunk = id / nt; tile = id % nt; }
  const int b0 = tile * WIDE3_R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int Dp = a.Dp, H1 = a.H1, H2 = a.H2, At = trunk ? 1 : a.A;      // head width: actions (policy trunk) / 1 (value trunk)
  const size_t B = (size_t)a.B;
  const int SX = 2 * Dp + 16, SC = 2 * WIDE3_CHUNK + 16, S2 = 2 * H2 + 16, S3 = 64 + 16;     // row strides (bytes)
  const int PX = WIDE3_R * SX, PC = WIDE3_R * SC, P2 = WIDE3_R * S2, P3 = WIDE3_R * S3;      // bytes of one plane
  char *Xs = wide3_lds, *Cs = Xs + 2 * PX, *H2s = Cs + 2 * PC, *dZ3s = H2s + 2 * P2;
  float *red = reinterpret_cast<float *>(Cs);                   // head: eight K-slices of the 32 x 32 output (32 KB <= 2 PC; the chunks are consumed by then)
  float *outs = reinterpret_cast<float *>(dZ3s + 2 * P3);       // [32][33] head outputs (+ bias)
  float *accs = outs + 32 * 33;                                 // [16][36] loss partials of the half-waves
  const size_t wpl = (size_t)a.total;
  const unsigned short *W1 = a.pk[trunk], *W2 = W1 + (size_t)H1 * Dp, *W2T = W2 + (size_t)H2 * H1, *W3 = W2T + (size_t)H1 * H2,
                       *W3T = W3 + 32 * (size_t)H2;
  const size_t plX = (size_t)((Dp + 31) & ~31) * B, pl1 = (size_t)H1 * B, pl2 = (size_t)H2 * B, pl3 = 32 * B;      // plane sizes of the transposed arrays

  WPROF(0);
  // ---- observations -> split rows (zero-padded to Dp); trunk 0 also files them, transposed, for the weight gradient of layer 1
  for (int i = tid; i < WIDE3_R * Dp; i += WIDE3_THREADS) {
    const int k = i >> 5, m = i & 31;
    unsigned short vh, vl;
    wide3_split(k < a.D ? a.obs[(size_t)(b0 + m) * a.D + k] : 0.f, vh, vl);
    *reinterpret_cast<unsigned short *>(Xs + m * SX + 2 * k) = vh;
    *reinterpret_cast<unsigned short *>(Xs + PX + m * SX + 2 * k) = vl;
    if (trunk == 0) { const size_t at = wide_frag(k, b0 + m, (int)(B >> 4)); a.xbT[at] = vh; a.xbT[plX + at] = vl; }
  }
  __syncthreads();

  WPROF(1);
  // ---- layers 1 and 2, chunk by chunk: wave w forms tile 8 c + w of H1 = tanh(X W1^T + b1) (A = X rows from LDS, B = W1 rows from
  // L2, at most seven k-steps, all requested together), the workgroup meets, and the waves that own tiles of layer 2 (two each) add
  // the chunk's sixteen k-steps of H1 W2^T to their accumulators
  const bool own2 = 2 * wave < (H2 >> 5);
  wide_f16 acc2[2];
#pragma unroll
  for (int j = 0; j < 16; j++) { acc2[0][j] = 0.f; acc2[1][j] = 0.f; }
  {
    const int nks1 = Dp >> 4;
    const wide_b8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < H1 / WIDE3_CHUNK; c++) {
      {
        const int t = c * WIDE3_NW + wave;
        wide_b8 bh[7], bl[7];
#pragma unroll
        for (int ks = 0; ks < 7; ks++) {   // no branch: a repeated fragment, unused
          bh[ks] = wide_ldfrag(W1, t, ks < nks1 ? ks : nks1 - 1, nks1, lane);
          bl[ks] = wide_ldfrag(W1 + wpl, t, ks < nks1 ? ks : nks1 - 1, nks1, lane);
        }
        const float bias = a.b1[trunk][t * 32 + r];
        wide_f16 acc;
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 7; ks++) {   // straight-line: the k-steps beyond Dp multiply by zero A fragments
          const char *xp = Xs + r * SX + ((ks < nks1 ? ks : 0) * 16 + 8 * h) * 2;
          const wide_b8 x_h = *reinterpret_cast<const wide_b8 *>(xp), x_l = *reinterpret_cast<const wide_b8 *>(xp + PX);
          acc = wide3_mma(ks < nks1 ? x_h : zero8, ks < nks1 ? x_l : zero8, bh[ks], bl[ks], acc);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; i++) v[i] = ppo_fast_tanh(acc[4 * q + i] + bias);
          wide3_put4(Cs, PC, SC, 8 * q + 4 * h, wave * 32 + r, a.h1T[trunk], pl1, B, t * 32 + r, b0 + 8 * q + 4 * h, v[0], v[1], v[2], v[3]);
        }
      }
      __syncthreads();
      if (own2) {
        const int t0 = 2 * wave;
        const unsigned short *wr = W2 + (((size_t)t0 * (H1 >> 4) + (size_t)c * (WIDE3_CHUNK >> 4)) * 64 + lane) * 8;
        wide3_stream<2, 4>(acc2, Cs + r * SC + 16 * h, PC, wr, wpl, (size_t)(H1 >> 4) * 512, WIDE3_CHUNK >> 4);
      }
      __syncthreads();      // the next chunk overwrites Cs
    }
  }
  WPROF(2);
  if (own2) {
    const int n0 = 2 * wave * 32 + r, n1 = n0 + 32;
    const float bias0 = a.b2[trunk][n0], bias1 = a.b2[trunk][n1];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float v[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { v[i] = ppo_fast_tanh(acc2[0][4 * q + i] + bias0); w[i] = ppo_fast_tanh(acc2[1][4 * q + i] + bias1); }
      wide3_put4(H2s, P2, S2, 8 * q + 4 * h, n0, a.h2T[trunk], pl2, B, n0, b0 + 8 * q + 4 * h, v[0], v[1], v[2], v[3]);
      wide3_put4(H2s, P2, S2, 8 * q + 4 * h, n1, a.h2T[trunk], pl2, B, n1, b0 + 8 * q + 4 * h, w[0], w[1], w[2], w[3]);
    }
  }
  __syncthreads();

  WPROF(3);
  // ---- head: out = H2 W3^T (32 columns, padded): K split over the eight waves, partial tiles summed through LDS
  {
    wide_f16 acc;
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = 0.f;
    const int kper = (H2 >> 4) / WIDE3_NW;                     // k-steps per wave (H2 = 512: 4)
    for (int q = 0; q < kper; q++) {
      const int ks = wave * kper + q;
      const char *hp = H2s + r * S2 + (ks * 16 + 8 * h) * 2;
      acc = wide3_mma(*reinterpret_cast<const wide_b8 *>(hp), *reinterpret_cast<const wide_b8 *>(hp + P2), wide_ldfrag(W3, 0, ks, H2 >> 4, lane),
                      wide_ldfrag(W3 + wpl, 0, ks, H2 >> 4, lane), acc);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) red[wave * 1024 + j * 64 + lane] = acc[j];
  }
  __syncthreads();
  for (int e = tid; e < 1024; e += WIDE3_THREADS) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WIDE3_NW; w++) s += red[w * 1024 + e];
    const int l = e & 63, j = e >> 6, n = l & 31;
    outs[wide_row(j, l >> 5) * 33 + n] = s + (n < At ? a.b3[trunk][n] : 0.f);
  }
  __syncthreads();

  WPROF(4);
  // ---- loss (arithmetic of ppo_loss_kernel): a half-wave per row, lane = action index; d out -> dZ3s (split) and, transposed, global
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
    for (int m = hw; m < WIDE3_R; m += 16) {
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
      unsigned short dh, dl;
      wide3_split(dz, dh, dl);
      *reinterpret_cast<unsigned short *>(dZ3s + m * S3 + 2 * j) = dh;
      *reinterpret_cast<unsigned short *>(dZ3s + P3 + m * S3 + 2 * j) = dl;
      const size_t at = wide_frag(j, b, (int)(B >> 4));
      a.dz3T[trunk][at] = dh;
      a.dz3T[trunk][pl3 + at] = dl;
    }
    accs[hw * 36 + j] = g_ls;
    if (j == 0) { accs[hw * 36 + 32] = pg; accs[hw * 36 + 33] = vl; accs[hw * 36 + 34] = kl; accs[hw * 36 + 35] = cf; }
  }
  __syncthreads();
  if (tid < 36) {   // this workgroup's partial sums (summed in fixed order by the weight-gradient launch's first block)
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) t += accs[i * 36 + tid];
    a.part[((size_t)trunk * nt + tile) * WIDE3_PART + tid] = t;
  }
  // bias gradients = column sums of dZ (file header): narrow nets keep them here
  if (a.bias_in_chain && tid < At) {
    float s = 0.f;
    for (int m = 0; m < WIDE3_R; m++)
      s += wide3_join(*reinterpret_cast<const unsigned short *>(dZ3s + m * S3 + 2 * tid), *reinterpret_cast<const unsigned short *>(dZ3s + P3 + m * S3 + 2 * tid));
    atomicAdd(&a.gb3[trunk][tid], s);
  }

  WPROF(5);
  // ---- d layer 2: dZ2 = (dZ3 W3) x (1 - H2^2), written over H2 by the lane that read it.  A = dZ3 rows (K = 32: two k-steps),
  // B[k = a][col = n] = W3T row n
  if (own2) {
    const int t0 = 2 * wave;
    wide_f16 acc0, acc1;
#pragma unroll
    for (int j = 0; j < 16; j++) { acc0[j] = 0.f; acc1[j] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const char *zp = dZ3s + r * S3 + (ks * 16 + 8 * h) * 2;
      const wide_b8 z_h = *reinterpret_cast<const wide_b8 *>(zp), z_l = *reinterpret_cast<const wide_b8 *>(zp + P3);
      acc0 = wide3_mma(z_h, z_l, wide_ldfrag(W3T, t0, ks, 2, lane), wide_ldfrag(W3T + wpl, t0, ks, 2, lane), acc0);
      acc1 = wide3_mma(z_h, z_l, wide_ldfrag(W3T, t0 + 1, ks, 2, lane), wide_ldfrag(W3T + wpl, t0 + 1, ks, 2, lane), acc1);
    }
    const int n0 = t0 * 32 + r, n1 = n0 + 32;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float v[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const char *hp = H2s + (8 * q + 4 * h + i) * S2;
        const float x0 = wide3_join(*reinterpret_cast<const unsigned short *>(hp + 2 * n0), *reinterpret_cast<const unsigned short *>(hp + P2 + 2 * n0));
        const float x1 = wide3_join(*reinterpret_cast<const unsigned short *>(hp + 2 * n1), *reinterpret_cast<const unsigned short *>(hp + P2 + 2 * n1));
        v[i] = acc0[4 * q + i] * (1.f - x0 * x0); w[i] = acc1[4 * q + i] * (1.f - x1 * x1);
      }
      wide3_put4(H2s, P2, S2, 8 * q + 4 * h, n0, a.dz2T[trunk], pl2, B, n0, b0 + 8 * q + 4 * h, v[0], v[1], v[2], v[3]);
      wide3_put4(H2s, P2, S2, 8 * q + 4 * h, n1, a.dz2T[trunk], pl2, B, n1, b0 + 8 * q + 4 * h, w[0], w[1], w[2], w[3]);
      s0 += (v[0] + v[1]) + (v[2] + v[3]); s1 += (w[0] + w[1]) + (w[2] + w[3]);
    }
    if (a.bias_in_chain) {
      s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32);
      if (h == 0) { atomicAdd(&a.gb2[trunk][n0], s0); atomicAdd(&a.gb2[trunk][n1], s1); }
    }
  }
  __syncthreads();

  WPROF(6);
  // ---- d layer 1: dZ1 = (dZ2 W2) x (1 - H1^2).  A = dZ2 rows (K = H2, now where H2 was), B[k = n][col = k1] = W2T row k1; four
  // 32-column tiles per wave share every A fragment; tanh' from the h1T planes this workgroup wrote (its own stores, behind barriers)
  for (int t0 = 4 * wave; t0 < (H1 >> 5); t0 += 4 * WIDE3_NW) {
    wide_f16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int j = 0; j < 16; j++) acc[q][j] = 0.f;
    const unsigned short *wrow = W2T + ((size_t)t0 * (H2 >> 4) * 64 + lane) * 8;
    wide3_stream<4, 1>(acc, H2s + r * S2 + 16 * h, P2, wrow, wpl, (size_t)(H2 >> 4) * 512, H2 >> 4);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int n = (t0 + q) * 32 + r;
      uint2 xh[4], xl[4];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const size_t at = wide_frag(n, b0 + 8 * g + 4 * h, (int)(B >> 4));
        xh[g] = *reinterpret_cast<const uint2 *>(a.h1T[trunk] + at);
        xl[g] = *reinterpret_cast<const uint2 *>(a.h1T[trunk] + pl1 + at);
      }
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float x0 = wide3_join((unsigned short)xh[g].x, (unsigned short)xl[g].x), x1 = wide3_join((unsigned short)(xh[g].x >> 16), (unsigned short)(xl[g].x >> 16));
        const float x2 = wide3_join((unsigned short)xh[g].y, (unsigned short)xl[g].y), x3 = wide3_join((unsigned short)(xh[g].y >> 16), (unsigned short)(xl[g].y >> 16));
        const float v0 = acc[q][4 * g] * (1.f - x0 * x0), v1 = acc[q][4 * g + 1] * (1.f - x1 * x1);
        const float v2 = acc[q][4 * g + 2] * (1.f - x2 * x2), v3 = acc[q][4 * g + 3] * (1.f - x3 * x3);
        wide3_store_t4(a.dz1T[trunk], pl1, B, n, b0 + 8 * g + 4 * h, v0, v1, v2, v3);
        s += (v0 + v1) + (v2 + v3);
      }
      if (a.bias_in_chain) {
        s += __shfl_xor(s, 32);
        if (h == 0) atomicAdd(&a.gb1[trunk][n], s);
      }
    }
  }
#ifdef WIDE_PROFILE
  __syncthreads();
  WPROF(7);
  if (threadIdx.x == 0 && blockIdx.x == 0)
    printf("wide3_fwdbwd wg0 ticks: obs %llu layers12 %llu tanh2 %llu head %llu loss %llu dlayer2 %llu dlayer1 %llu\n", wprof[1] - wprof[0], wprof[2] - wprof[1],
           wprof[3] - wprof[2], wprof[4] - wprof[3], wprof[5] - wprof[4], wprof[6] - wprof[5], wprof[7] - wprof[6]);
#endif
}

// dW = dZ^T X for the six layers, as wide_wgrad_kernel of dm_ppo_wide.hip: four waves own four 32 x 32 tiles of dW, split the batch
// between them and meet in LDS; with split-K 1 a tile has one owner, a fixed summation order and no atomics.  Both operands are
// two-plane arrays: three MFMAs per tile and k-step, and for the bias gradient one MFMA per plane of dZ^T against a fragment of ones.
struct Wide3WgradJob { const unsigned short *AT, *XT; long long apl, xpl; float *dW, *db; int O, I, ldw, ro, otiles, itiles, splitk, first, per; };
struct Wide3WgradArgs {
  Wide3WgradJob j[6];
  int njobs, nblocks, B;
  const float *part; int nblk, A; const float *log_std; float vf_coef, ent_coef; const float *stats; float *g_log_std, *out8, *loss_acc;
};

template <int RO, int CI>
__device__ __forceinline__ void wide3_wgrad_tile(const Wide3WgradJob &J, const int Bn, const int ot, const int it, const int ks, const int wave, const int lane,
                                                 float *wl) {
  constexpr int NT = RO * CI;                    // 32 x 32 tiles of dW per wave (a multiple of 4)
  const int r = lane & 31, h = lane >> 5;
  const int o0 = ot * 32 * RO, i0 = it * 32 * CI;
  const size_t B = (size_t)Bn;
  // batch rows of this workgroup's split, in units of 64 rows; the four waves take a quarter of the units each
  const int units = (Bn / J.splitk) >> 6, u0 = wave * units / WIDE3_WG_WAVES, u1 = (wave + 1) * units / WIDE3_WG_WAVES;
  const int k0 = ks * (Bn / J.splitk) + u0 * 64;
  const size_t tstride = (B >> 4) * 512;                        // elements of one 32-feature tile: (B / 16) k-steps of 512
  const unsigned short *ap = J.AT + (size_t)(o0 >> 5) * tstride + ((size_t)(k0 >> 4) * 64 + lane) * 8;
  const unsigned short *xp = J.XT + (size_t)(i0 >> 5) * tstride + ((size_t)(k0 >> 4) * 64 + lane) * 8;
  const size_t apl = (size_t)J.apl, xpl = (size_t)J.xpl;
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
  const bool bias = J.db != nullptr && it == 0;
  const wide_b8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  wide_f16 accb[RO];
#pragma unroll
  for (int p = 0; p < RO; p++)
#pragma unroll
    for (int j = 0; j < 16; j++) accb[p][j] = 0.f;
  const wide_b8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // two-deep ring of one k-step (both planes of RO + CI fragments: 32 or 40 VGPRs a block)
  wide_b8 ah[RO], al[RO], xh[CI], xl[CI], bh[RO], bl[RO], yh[CI], yl[CI];
  auto load_blk = [&](wide_b8 (&Ah)[RO], wide_b8 (&Al)[RO], wide_b8 (&Xh)[CI], wide_b8 (&Xl)[CI], const int kk) {
#pragma unroll
    for (int p = 0; p < RO; p++) {
      Ah[p] = oa[p] ? *reinterpret_cast<const wide_b8 *>(ap + p * tstride + (size_t)kk * 512) : zero;
      Al[p] = oa[p] ? *reinterpret_cast<const wide_b8 *>(ap + apl + p * tstride + (size_t)kk * 512) : zero;
    }
#pragma unroll
    for (int q = 0; q < CI; q++) {
      Xh[q] = ia[q] ? *reinterpret_cast<const wide_b8 *>(xp + q * tstride + (size_t)kk * 512) : zero;
      Xl[q] = ia[q] ? *reinterpret_cast<const wide_b8 *>(xp + xpl + q * tstride + (size_t)kk * 512) : zero;
    }
  };
  auto mma_blk = [&](const wide_b8 (&Ah)[RO], const wide_b8 (&Al)[RO], const wide_b8 (&Xh)[CI], const wide_b8 (&Xl)[CI]) {
#pragma unroll
    for (int p = 0; p < RO; p++)
#pragma unroll
      for (int q = 0; q < CI; q++) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al[p], Xh[q], acc[p][q], 0, 0, 0);
#pragma unroll
    for (int p = 0; p < RO; p++)
#pragma unroll
      for (int q = 0; q < CI; q++) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah[p], Xl[q], acc[p][q], 0, 0, 0);
#pragma unroll
    for (int p = 0; p < RO; p++)
#pragma unroll
      for (int q = 0; q < CI; q++) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah[p], Xh[q], acc[p][q], 0, 0, 0);
    if (bias) {
#pragma unroll
      for (int p = 0; p < RO; p++) accb[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al[p], ones, accb[p], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < RO; p++) accb[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah[p], ones, accb[p], 0, 0, 0);
    }
  };
  const int nks = (u1 - u0) * 4;                     // k-steps of 16 rows: a multiple of 4, possibly 0
  if (nks > 0) load_blk(ah, al, xh, xl, 0);
  for (int kk = 0; kk < nks; kk += 2) {
    load_blk(bh, bl, yh, yl, kk + 1);
    mma_blk(ah, al, xh, xl);
    if (kk + 2 < nks) load_blk(ah, al, xh, xl, kk + 2);
    mma_blk(bh, bl, yh, yl);
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
  // the four partial blocks meet in LDS, four tiles at a time ([wave][tile][register][lane]); wave w then owns tile 4 ph + w: fixed
  // summation order, and with splitk == 1 a plain add by the tile's one owner (no atomics, bit-reproducible gradients)
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
    // gradients are ACCUMULATED (deepmimic_hip.h), also where a tile has one owner: its present values are requested before the barrier
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
        for (int w = 0; w < WIDE3_WG_WAVES; w++) v += wl[((w * 4 + wave) << 10) + j * 64 + lane];
        const int row = o0 + 32 * p + wide_row(j, h);
        if (row < J.O) {
          float *dst = &J.dW[(size_t)row * J.ldw + i0 + 32 * q + r];
          if (J.splitk == 1) *dst = old[j] + v; else atomicAdd(dst, v);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(64 * WIDE3_WG_WAVES, 2) wide3_wgrad_kernel(Wide3WgradArgs a) {
  extern __shared__ __align__(16) float wide3_wl[];      // 4 waves x 4 tiles x 4 KB
  const int blk = (int)blockIdx.x - 1, tid = threadIdx.x;
  if (blk < 0) {   // block 0 (dispatched first): loss scalars and the log_std gradient from the per-workgroup partials, in a fixed order
    __shared__ float red[2][36];
    float (*lsum)[41] = reinterpret_cast<float (*)[41]>(wide3_wl);      // [256][41]
    for (int t = 0; t < 2; t++) {
      float acc[WIDE3_PART];
#pragma unroll
      for (int e = 0; e < WIDE3_PART; e++) acc[e] = 0.f;
      for (int i = tid; i < a.nblk; i += 64 * WIDE3_WG_WAVES) {
        const float4 *row = reinterpret_cast<const float4 *>(a.part + ((size_t)t * a.nblk + i) * WIDE3_PART);
#pragma unroll
        for (int e = 0; e < WIDE3_PART / 4; e++) { const float4 v = row[e]; acc[4 * e] += v.x; acc[4 * e + 1] += v.y; acc[4 * e + 2] += v.z; acc[4 * e + 3] += v.w; }
      }
#pragma unroll
      for (int e = 0; e < 36; e++) lsum[tid][e] = acc[e];
      __syncthreads();
      if (tid < 36) {
        float s0 = 0.f;
        for (int l = 0; l < 64 * WIDE3_WG_WAVES; l++) s0 += lsum[l][tid];
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
  const Wide3WgradJob &J = a.j[jq];
  // XCD x takes the x-th eighth of a job's (split, output tile, input tile) order, input tile fastest (dm_ppo_wide.hip)
  const int loc = blk - J.first;
  int rem = (loc & 7) * J.per + (loc >> 3);
  if ((loc >> 3) >= J.per || rem >= J.splitk * J.otiles * J.itiles) return;
  const int it = rem % J.itiles; rem /= J.itiles;
  const int ot = rem % J.otiles, ks = rem / J.otiles;
  if (J.ro == 2) wide3_wgrad_tile<2, 2>(J, a.B, ot, it, ks, tid >> 6, tid & 63, wide3_wl);
  else wide3_wgrad_tile<1, 4>(J, a.B, ot, it, ks, tid >> 6, tid & 63, wide3_wl);
}

inline int wide3_dp(int D) { return (D + 15) & ~15; }
inline long long wide3_plane_elems(int D, int H1, int H2) { return (long long)H1 * wide3_dp(D) + 2ll * H2 * H1 + 64ll * H2; }
inline int wide3_lds_bytes(int D, int H2) {
  return 2 * WIDE3_R * (2 * wide3_dp(D) + 16) + 2 * WIDE3_R * (2 * WIDE3_CHUNK + 16) + 2 * WIDE3_R * (2 * H2 + 16) + 2 * WIDE3_R * 80 + (32 * 33 + 16 * 36) * 4;
}
inline bool wide3_supported(int B, int D, int H1, int H2, int A) {
  return B >= 64 && B % 64 == 0 && D >= 1 && D <= 112 && H1 % 256 == 0 && H1 >= 256 && H1 <= 1024 && H2 % 128 == 0 && H2 >= 128 && H2 <= 512 && A >= 1 &&
         A <= 32 && wide3_lds_bytes(D, H2) <= 160 * 1024;
}

}  // namespace

extern "C" long long dm_ppo_wide3_packed_elems(int D, int H1, int H2) { return 2 * wide3_plane_elems(D, H1, H2); }
extern "C" int dm_ppo_wide3_supported(int B, int D, int H1, int H2, int A) { return wide3_supported(B, D, H1, H2, A) ? 1 : 0; }

extern "C" int dm_ppo_wide3_grad(const DmPpoWide3Step *s, void *stream) {
  if (!s || !wide3_supported(s->B, s->D, s->H1, s->H2, s->A)) return DM_EINVAL;
  if (!s->obs || !s->act || !s->adv || !s->ret || !s->old_logp || !s->log_std || !s->g_log_std || !s->xbT || !s->part || !s->stats8 || !s->out8) return DM_EINVAL;
  for (int t = 0; t < 2; t++) {
    if (!s->wpk[t] || !s->h1T[t] || !s->dz1T[t] || !s->h2T[t] || !s->dz2T[t] || !s->dz3T[t]) return DM_EINVAL;
    for (int l = 0; l < 3; l++) if (!s->W[t][l] || !s->b[t][l] || !s->gW[t][l] || !s->gb[t][l]) return DM_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  static int lds_set_for = -1;
  const int lds = wide3_lds_bytes(s->D, s->H2);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return DM_EHIP;
  if (lds_set_for != dev) {   // per device, outside capture: the warm-up calls before a capture pass here
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(wide3_fwdbwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return DM_EHIP;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(wide3_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, WIDE3_WG_WAVES * 4 * 4096) != hipSuccess) return DM_EHIP;
    lds_set_for = dev;
  }
  const int Dp = wide3_dp(s->D);
  const long long total = wide3_plane_elems(s->D, s->H1, s->H2);
  Wide3PackArgs p;
  memset(&p, 0, sizeof p);
  for (int t = 0; t < 2; t++) { for (int l = 0; l < 3; l++) p.W[t][l] = s->W[t][l]; p.pk[t] = (unsigned short *)s->wpk[t]; }
  p.D = s->D; p.Dp = Dp; p.H1 = s->H1; p.H2 = s->H2; p.A[0] = s->A; p.A[1] = 1;
  p.total = total;
  p.pack_blocks = 1152;      // ~one fragment (of each plane) per thread for the [1024,512] net
  p.adv = s->adv; p.B = s->B; p.normalize = s->normalize_advantage; p.stats = s->stats8; p.out8 = s->out8;
  p.zero_ptr = s->zero_ptr; p.zero_floats = s->zero_ptr ? s->zero_floats : 0; p.adam_state2 = s->adam_state2;
  const int zero_blocks = (int)((p.zero_floats + 1023) / 1024);
  hipLaunchKernelGGL(wide3_pack_kernel, dim3(2 * p.pack_blocks + 1 + zero_blocks), dim3(256), 0, st, p);
  Wide3Args a;
  memset(&a, 0, sizeof a);
  a.B = s->B; a.D = s->D; a.Dp = Dp; a.H1 = s->H1; a.H2 = s->H2; a.A = s->A; a.total = total;
  a.obs = s->obs; a.act = s->act; a.adv = s->adv; a.ret = s->ret; a.old_logp = s->old_logp; a.log_std = s->log_std; a.stats = s->stats8;
  for (int t = 0; t < 2; t++) {
    a.pk[t] = (const unsigned short *)s->wpk[t];
    a.b1[t] = s->b[t][0]; a.b2[t] = s->b[t][1]; a.b3[t] = s->b[t][2];
    a.gb1[t] = s->gb[t][0]; a.gb2[t] = s->gb[t][1]; a.gb3[t] = s->gb[t][2];
    a.h1T[t] = (unsigned short *)s->h1T[t]; a.dz1T[t] = (unsigned short *)s->dz1T[t]; a.h2T[t] = (unsigned short *)s->h2T[t];
    a.dz2T[t] = (unsigned short *)s->dz2T[t]; a.dz3T[t] = (unsigned short *)s->dz3T[t];
  }
  a.xbT = (unsigned short *)s->xbT; a.part = s->part; a.clip = s->clip_range; a.vf_coef = s->vf_coef;
  const bool bias_wgrad = s->H1 >= WIDE3_BIAS_WGRAD_H1;
  a.bias_in_chain = bias_wgrad ? 0 : 1;
  hipLaunchKernelGGL(wide3_fwdbwd_kernel, dim3(2 * (s->B / WIDE3_R)), dim3(WIDE3_THREADS), lds, st, a);
  // weight gradients: per trunk dW2 (the big one), dW1, dW3; split-K chosen so that every job brings ~64-128 workgroups
  Wide3WgradArgs g;
  memset(&g, 0, sizeof g);
  int first = 0, nj = 0;
  const long long Bl = s->B, plX = (long long)((Dp + 31) & ~31) * Bl;
  auto add = [&](const void *AT, long long apl, const void *XT, long long xpl, float *dW, float *db, int O, int I, int ldw, int ro, int want) {
    Wide3WgradJob &J = g.j[nj++];
    J.AT = (const unsigned short *)AT; J.XT = (const unsigned short *)XT; J.apl = apl; J.xpl = xpl; J.dW = dW; J.db = db; J.O = O; J.I = I; J.ldw = ldw; J.ro = ro;
    J.otiles = (O + 32 * ro - 1) / (32 * ro);
    J.itiles = (I + 32 * (4 / ro) - 1) / (32 * (4 / ro));
    int sk = 1;
    while (sk < WIDE3_MAX_SPLITK && J.otiles * J.itiles * sk * 2 <= want && (s->B / (sk * 2)) % 64 == 0) sk *= 2;     // want: workgroups
    J.splitk = sk; J.first = first;                       // first % 8 == 0: a job's local block id & 7 is its XCD
    J.per = (J.otiles * J.itiles * sk + 7) / 8;
    first += 8 * J.per;
  };
  for (int t = 0; t < 2; t++) {
    add(s->dz2T[t], s->H2 * Bl, s->h1T[t], s->H1 * Bl, s->gW[t][1], bias_wgrad ? s->gb[t][1] : nullptr, s->H2, s->H1, s->H1, 2, 128);
    add(s->dz1T[t], s->H1 * Bl, s->xbT, plX, s->gW[t][0], bias_wgrad ? s->gb[t][0] : nullptr, s->H1, s->D, s->D, 2, 32);
    add(s->dz3T[t], 32 * Bl, s->h2T[t], s->H2 * Bl, s->gW[t][2], bias_wgrad ? s->gb[t][2] : nullptr, t ? 1 : s->A, s->H2, s->H2, 1, 4);
  }
  g.njobs = nj; g.nblocks = first; g.B = s->B;
  g.part = s->part; g.nblk = s->B / WIDE3_R; g.A = s->A; g.log_std = s->log_std; g.vf_coef = s->vf_coef; g.ent_coef = s->ent_coef; g.stats = s->stats8;
  g.g_log_std = s->g_log_std; g.out8 = s->out8; g.loss_acc = s->loss_acc;
  hipLaunchKernelGGL(wide3_wgrad_kernel, dim3(first + 1), dim3(64 * WIDE3_WG_WAVES), WIDE3_WG_WAVES * 4 * 4096, st, g);
  return dm_launch_status();
}
