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
#include "dm_wide_common.h"    // constants, WPROF, the split rule, pack, loss section, weight gradients, host launcher (P = 2 planes)

namespace {

// acc += a b without lo.lo
__device__ __forceinline__ wide_f16 wide3_mma(const wide_b8 ah, const wide_b8 al, const wide_b8 bh, const wide_b8 bl, wide_f16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

constexpr int WIDE3_CHUNK = 32 * WIDE_NW;   // layer-1 columns per chunk: one tile per wave

__global__ void __launch_bounds__(256) wide3_pack_kernel(WidePackArgs a) { wide_pack_body<2>(a); }

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

__global__ void __launch_bounds__(WIDE_THREADS) wide3_fwdbwd_kernel(Wide3Args a) {
  extern __shared__ __align__(16) char wide3_lds[];
  // workgroups go round the eight XCDs in launch order: even XCDs take the policy trunk, odd ones the value trunk, so an XCD's L2
  // streams ONE trunk's weights
#ifdef WIDE_PROFILE
  unsigned long long wprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  const int nt = a.B / WIDE_R, id = blockIdx.x;
  int trunk, tile;
  if ((nt & 3) == 0) { const int xcd = id & 7; trunk = xcd & 1; tile = (id >> 3) * 4 + (xcd >> 1); }
  else { trunk = id / nt; tile = id % nt; }
  const int b0 = tile * WIDE_R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int Dp = a.Dp, H1 = a.H1, H2 = a.H2, At = trunk ? 1 : a.A;      // head width: actions (policy trunk) / 1 (value trunk)
  const size_t B = (size_t)a.B;
  const int SX = 2 * Dp + 16, SC = 2 * WIDE3_CHUNK + 16, S2 = 2 * H2 + 16, S3 = 64 + 16;     // row strides (bytes)
  const int PX = WIDE_R * SX, PC = WIDE_R * SC, P2 = WIDE_R * S2, P3 = WIDE_R * S3;      // bytes of one plane
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
  for (int i = tid; i < WIDE_R * Dp; i += WIDE_THREADS) {
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
        const int t = c * WIDE_NW + wave;
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
    const int kper = (H2 >> 4) / WIDE_NW;                     // k-steps per wave (H2 = 512: 4)
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
  wide_head_sum(red, outs, a.b3[trunk], At, tid);

  WPROF(4);
  // ---- loss: d out -> dZ3s (split) and, transposed, global; loss partials; on narrow nets the head's bias gradient
  wide_loss_rows<2>(a, trunk, tile, At, tid, outs, accs, dZ3s, S3);

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
  for (int t0 = 4 * wave; t0 < (H1 >> 5); t0 += 4 * WIDE_NW) {
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

// dW = dZ^T X of the six layers from the two-plane arrays: dm_wide_common.h, a ring of one k-step
__global__ void __launch_bounds__(64 * WIDE_WG_WAVES, 2) wide3_wgrad_kernel(WideWgradArgs<2> a) {
  extern __shared__ __align__(16) float wide3_wl[];      // 4 waves x 4 tiles x 4 KB
  wide_wgrad_body<2, 1>(a, wide3_wl);
}

inline int wide3_lds_bytes(int D, int H2) {
  return 2 * WIDE_R * (2 * wide_dp(D) + 16) + 2 * WIDE_R * (2 * WIDE3_CHUNK + 16) + 2 * WIDE_R * (2 * H2 + 16) + 2 * WIDE_R * 80 + (32 * 33 + 16 * 36) * 4;
}
inline bool wide3_supported(int B, int D, int H1, int H2, int A) {
  return B >= 64 && B % 64 == 0 && D >= 1 && D <= 112 && H1 % 256 == 0 && H1 >= 256 && H1 <= 1024 && H2 % 128 == 0 && H2 >= 128 && H2 <= 512 && A >= 1 &&
         A <= 32 && wide3_lds_bytes(D, H2) <= 160 * 1024;
}

}  // namespace

extern "C" long long dm_ppo_wide3_packed_elems(int D, int H1, int H2) { return 2 * wide_plane_elems(D, H1, H2); }
extern "C" int dm_ppo_wide3_supported(int B, int D, int H1, int H2, int A) { return wide3_supported(B, D, H1, H2, A) ? 1 : 0; }

extern "C" int dm_ppo_wide3_grad(const DmPpoWide3Step *s, void *stream) {
  if (!s || !wide3_supported(s->B, s->D, s->H1, s->H2, s->A)) return DM_EINVAL;
  return wide_launch<2, Wide3Args>(s, (hipStream_t)stream, wide3_pack_kernel, wide3_fwdbwd_kernel, wide3_wgrad_kernel, wide3_lds_bytes(s->D, s->H2));
}
