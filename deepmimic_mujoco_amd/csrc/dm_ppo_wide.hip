// One PPO minibatch of the WIDE actor-critic MLP (net_arch = [1024, 512], the net BASELINE configs 3-5 name) on the bf16 matrix pipe.
//
// Reference: src/sb3_ppo.py:254-271,307-312 -> [EXT] SB3 PPO.train on MlpPolicy: per minibatch evaluate_actions (both trunks), the
// clipped-surrogate / value / entropy loss, backward through both trunks.  The library path of this net is six ~55 us fp32 GEMMs per
// trunk on a two-stream dependency chain plus a dozen small launches (0.39 ms per optimizer step; with bf16 library GEMMs 0.37 ms: the
// chain, not the GEMMs, bounds it).  Here the whole forward / loss / input-gradient chain of BOTH trunks is ONE launch:
//   1. wide_pack_kernel    fp32 master weights -> bf16 in the two layouts the chain reads (W for X W^T, W^T for dZ W); advantage
//                          statistics; optional folds: clearing the gradient arena, Adam's begin                            (1 launch)
//   2. wide_fwdbwd_kernel  a workgroup of eight waves carries 32 minibatch rows of one trunk through layer 1, layer 2, the head, the
//                          loss (the arithmetic of ppo_loss_kernel), and back: d head, d layer 2 (x tanh'), d layer 1 (x tanh');
//                          activations live in LDS as bf16 (64 + 32 + 32 KB), every product is v_mfma_f32_32x32x16_bf16 with fp32
//                          accumulation, weights stream from L2 in FRAGMENT order (below): one operand load of a wave is 1 KB of
//                          consecutive bytes; outputs: the bf16 activations / pre-activation gradients the weight gradients need,
//                          per-workgroup loss partials, and on narrow nets the bias gradients (column sums, fp32 atomics)     (1 launch)
//   3. wide_wgrad_kernel   dW = dZ^T X of all six layers: the chain leaves its activations and pre-activation gradients TRANSPOSED
//                          (features x batch) in the same fragment order, written straight from the accumulator registers (four
//                          consecutive batch rows of a column are 8 bytes of a fragment); a workgroup of four waves owns four
//                          32 x 32 tiles of dW, the waves split the batch and meet in LDS (plain adds on wide nets, split-K
//                          with fp32 atomics only on narrow ones); the bias gradients of wide nets come from one more MFMA per
//                          k-step against a fragment of ones; block 0 sums the loss partials                                 (1 launch)
// Fragment order of a matrix M[N][K] (N % 32 == 0, K % 16 == 0) that feeds v_mfma_f32_32x32x16_bf16 as the operand with row / column
// index n and reduction index k: element (n, k) lives at ((((n >> 5) * (K >> 4) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (n & 31)) * 8
// + (k & 7)) — tile of 32 rows, k-step of 16, then the 64 lanes' 16-byte fragments in lane order.  A wave's load of one fragment is
// base + lane * 16 bytes: eight full 128-byte lines.  (Row-major operands made every load touch 32 lines for 32 bytes each and lean
// on the 32 KB vector L1 to hold 512 half-used lines across k-steps: 92 us for the chain, 58 us for the weight gradients; now 43 + 38.)
// fp32 master weights, fp32 loss arithmetic, fp32 gradients and Adam; bf16 operands of the products only (north_star: "MFMA used
// only for the policy-MLP GEMMs").
#include "dm_wide_common.h"    // constants, WPROF, pack, loss section, weight gradients, host launcher (P = 1 plane)

namespace {

__global__ void __launch_bounds__(256) wide_pack_kernel(WidePackArgs a) { wide_pack_body<1>(a); }

struct WideArgs {
  int B, D, Dp, H1, H2, A;
  const float *obs, *act, *adv, *ret, *old_logp, *log_std, *stats;
  const unsigned short *pk[2];
  const float *b1[2], *b2[2], *b3[2];
  float *gb1[2], *gb2[2], *gb3[2];
  unsigned short *xbT, *h1T[2], *dz1T[2], *h2T[2], *dz2T[2], *dz3T[2];   // [features][B] bf16
  float *part;
  float clip, vf_coef;
  int bias_in_chain;               // 1: the chain adds its 32-row column sums of dZ to the bias gradients (small nets); 0: the weight-gradient launch forms them
};

// four consecutive batch rows row0 .. row0 + 3 (row0 % 4 == 0) of one feature column — accumulator registers 4 q .. 4 q + 3 of a
// lane — as 8 bytes of the transposed (features x batch) array in fragment order
__device__ __forceinline__ void wide_store_t4(unsigned short *T, size_t B, int col, int row0, float v0, float v1, float v2, float v3) {
  uint2 u;
  u.x = wide_pk2(v0, v1);
  u.y = wide_pk2(v2, v3);
  *reinterpret_cast<uint2 *>(T + wide_frag(col, row0, (int)(B >> 4))) = u;
}

// the same four values also into the LDS copy of the activations (rows row0 .. row0 + 3 of column col, row stride `stride` bytes)
__device__ __forceinline__ void wide_put4(char *L, int stride, int lrow0, int col, unsigned short *T, size_t B, int grow0, float v0, float v1,
                                          float v2, float v3) {
  uint2 u;
  u.x = wide_pk2(v0, v1);
  u.y = wide_pk2(v2, v3);
  char *p = L + lrow0 * stride + 2 * col;
  *reinterpret_cast<unsigned short *>(p) = (unsigned short)u.x;
  *reinterpret_cast<unsigned short *>(p + stride) = (unsigned short)(u.x >> 16);
  *reinterpret_cast<unsigned short *>(p + 2 * stride) = (unsigned short)u.y;
  *reinterpret_cast<unsigned short *>(p + 3 * stride) = (unsigned short)(u.y >> 16);
  *reinterpret_cast<uint2 *>(T + wide_frag(col, grow0, (int)(B >> 4))) = u;
}

__global__ void __launch_bounds__(WIDE_THREADS) wide_fwdbwd_kernel(WideArgs a) {
  extern __shared__ __align__(16) char wide_lds[];
  // workgroups go round the eight XCDs in launch order: even XCDs take the policy trunk, odd ones the value trunk, so an XCD's L2
  // streams ONE trunk's 2.3 MB of weights (both trunks: 4.6 MB against 4 MB of L2)
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
  const int SX = 2 * Dp + 16, S1 = 2 * H1 + 16, S2 = 2 * H2 + 16, S3 = 64 + 16;     // row strides (bytes): 16-byte reads of 32 rows spread over the banks
  const int RZ = WIDE_R * S2 > WIDE_NW * 4096 ? WIDE_R * S2 : WIDE_NW * 4096;      // dZ2s shares its block with the head's partial tiles
  char *Xs = wide_lds, *H1s = Xs + WIDE_R * SX, *H2s = H1s + WIDE_R * S1, *dZ2s = H2s + WIDE_R * S2, *dZ3s = dZ2s + RZ;
  float *red = reinterpret_cast<float *>(dZ2s);                 // head: eight K-slices of the 32 x 32 output (32 KB; dZ2s is not live yet)
  float *outs = reinterpret_cast<float *>(dZ3s + WIDE_R * S3);  // [32][33] head outputs (+ bias)
  float *accs = outs + 32 * 33;                                 // [16][36] loss partials of the half-waves
  const unsigned short *W1 = a.pk[trunk], *W2 = W1 + (size_t)H1 * Dp, *W2T = W2 + (size_t)H2 * H1, *W3 = W2T + (size_t)H1 * H2,
                       *W3T = W3 + 32 * (size_t)H2;

  WPROF(0);
  // ---- observations -> bf16 rows (zero-padded to Dp); trunk 0 also files them, transposed, for the weight gradient of layer 1
  for (int i = tid; i < WIDE_R * Dp; i += WIDE_THREADS) {
    const int k = i >> 5, m = i & 31;                                  // (consecutive threads: consecutive rows of one column)
    const unsigned short v = wide_f2bf(k < a.D ? a.obs[(size_t)(b0 + m) * a.D + k] : 0.f);
    *reinterpret_cast<unsigned short *>(Xs + m * SX + 2 * k) = v;
    if (trunk == 0) a.xbT[wide_frag(k, b0 + m, (int)(B >> 4))] = v;
  }
  __syncthreads();

  WPROF(1);
  // ---- layer 1: H1 = tanh(X W1^T + b1).  A = X rows from LDS (lane: row r, k = 8 h + j), B = W1 rows from L2 (lane: column r)
  // (the weight fragments of a tile — at most seven k-steps — are requested together, and those of the wave's NEXT tile before this
  // tile's MFMAs: with one load per k-step inside the loop every MFMA waited for its own L2 round trip and this layer, a ninth of
  // layer 2's work, took as long as layer 2: 25 k of the kernel's 102 k ticks)
  {
    const int nks1 = Dp >> 4, ntile = H1 >> 5;
    const wide_b8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    wide_b8 pa[7], pb[7];
    float ba = 0.f, bb = 0.f;                     // the tile's bias travels with its weights (a load after the MFMAs is an exposed round trip)
    auto ld = [&](wide_b8 (&P)[7], float &bias, const int t) {
#pragma unroll
      for (int ks = 0; ks < 7; ks++) P[ks] = wide_ldfrag(W1, t, ks < nks1 ? ks : nks1 - 1, nks1, lane);   // no branch: a repeated fragment, unused
      bias = a.b1[trunk][t * 32 + r];
    };
    auto run = [&](const wide_b8 (&P)[7], const float bias, const int t) {
      wide_f16 acc;
#pragma unroll
      for (int j = 0; j < 16; j++) acc[j] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 7; ks++) {   // straight-line: the k-steps beyond Dp multiply by a zero A fragment
        const wide_b8 a0 = *reinterpret_cast<const wide_b8 *>(Xs + r * SX + ((ks < nks1 ? ks : 0) * 16 + 8 * h) * 2);
        const wide_b8 av = ks < nks1 ? a0 : zero8;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, P[ks], acc, 0, 0, 0);
      }
      const int n = t * 32 + r;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = ppo_fast_tanh(acc[4 * q + i] + bias);
        wide_put4(H1s, S1, 8 * q + 4 * h, n, a.h1T[trunk], B, b0 + 8 * q + 4 * h, v[0], v[1], v[2], v[3]);
      }
    };
    int t = wave;
    if (t < ntile) ld(pa, ba, t);
    for (; t < ntile; t += 2 * WIDE_NW) {
      if (t + WIDE_NW < ntile) ld(pb, bb, t + WIDE_NW);
      run(pa, ba, t);
      if (t + 2 * WIDE_NW < ntile) ld(pa, ba, t + 2 * WIDE_NW);
      if (t + WIDE_NW < ntile) run(pb, bb, t + WIDE_NW);
    }
  }
  __syncthreads();

  WPROF(2);
  // ---- layer 2: H2 = tanh(H1 W2^T + b2): two 32-column tiles per wave per pass share every A fragment; the weight rows stream
  // from L2 through a two-deep ring of register blocks (eight k-steps each), so sixteen loads per lane are always in flight
  for (int t0 = 2 * wave; t0 < (H2 >> 5); t0 += 2 * WIDE_NW) {
    wide_f16 acc0, acc1;
#pragma unroll
    for (int j = 0; j < 16; j++) { acc0[j] = 0.f; acc1[j] = 0.f; }
    const char *ap = H1s + r * S1 + 16 * h;
    const int n0 = t0 * 32 + r, n1 = n0 + 32;
    const float bias0 = a.b2[trunk][n0], bias1 = a.b2[trunk][n1];      // requested with the first weights, used after the k loop
    // fragments of tile t0 / t0 + 1: k-step ks at wr + ks * 512 elements (1 KB per wave), consecutive k-steps consecutive in memory
    const unsigned short *wr0 = W2 + ((size_t)t0 * (H1 >> 4) * 64 + lane) * 8, *wr1 = wr0 + (size_t)(H1 >> 4) * 512;
    constexpr int KB = 8;
    wide_b8 p0[KB], p1[KB], q0[KB], q1[KB];
    const int nblk = (H1 >> 4) / KB;                       // H1 % 256 == 0: an even number of blocks
#pragma unroll
    for (int i = 0; i < KB; i++) { p0[i] = *reinterpret_cast<const wide_b8 *>(wr0 + i * 512); p1[i] = *reinterpret_cast<const wide_b8 *>(wr1 + i * 512); }
    for (int kb = 0; kb < nblk; kb += 2) {
#pragma unroll
      for (int i = 0; i < KB; i++) { q0[i] = *reinterpret_cast<const wide_b8 *>(wr0 + ((kb + 1) * KB + i) * 512); q1[i] = *reinterpret_cast<const wide_b8 *>(wr1 + ((kb + 1) * KB + i) * 512); }
#pragma unroll
      for (int i = 0; i < KB; i++) {
        const wide_b8 av = *reinterpret_cast<const wide_b8 *>(ap + (kb * KB + i) * 32);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, p0[i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, p1[i], acc1, 0, 0, 0);
      }
      if (kb + 2 < nblk) {
#pragma unroll
        for (int i = 0; i < KB; i++) { p0[i] = *reinterpret_cast<const wide_b8 *>(wr0 + ((kb + 2) * KB + i) * 512); p1[i] = *reinterpret_cast<const wide_b8 *>(wr1 + ((kb + 2) * KB + i) * 512); }
      }
#pragma unroll
      for (int i = 0; i < KB; i++) {
        const wide_b8 av = *reinterpret_cast<const wide_b8 *>(ap + ((kb + 1) * KB + i) * 32);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q0[i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q1[i], acc1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float v[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { v[i] = ppo_fast_tanh(acc0[4 * q + i] + bias0); w[i] = ppo_fast_tanh(acc1[4 * q + i] + bias1); }
      wide_put4(H2s, S2, 8 * q + 4 * h, n0, a.h2T[trunk], B, b0 + 8 * q + 4 * h, v[0], v[1], v[2], v[3]);
      wide_put4(H2s, S2, 8 * q + 4 * h, n1, a.h2T[trunk], B, b0 + 8 * q + 4 * h, w[0], w[1], w[2], w[3]);
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
      const wide_b8 av = *reinterpret_cast<const wide_b8 *>(H2s + r * S2 + (ks * 16 + 8 * h) * 2);
      const wide_b8 bv = wide_ldfrag(W3, 0, ks, H2 >> 4, lane);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) red[wave * 1024 + j * 64 + lane] = acc[j];
  }
  __syncthreads();
  wide_head_sum(red, outs, a.b3[trunk], At, tid);

  WPROF(4);
  // ---- loss: d out -> dZ3s (bf16) and, transposed, HBM; loss partials; on narrow nets the head's bias gradient
  wide_loss_rows<1>(a, trunk, tile, At, tid, outs, accs, dZ3s, S3);

  WPROF(5);
  // ---- d layer 2: dZ2 = (dZ3 W3) x (1 - H2^2).  A = dZ3 rows (K = 32: two k-steps), B[k = a][col = n] = W3T row n
  for (int t0 = 2 * wave; t0 < (H2 >> 5); t0 += 2 * WIDE_NW) {
    wide_f16 acc0, acc1;
#pragma unroll
    for (int j = 0; j < 16; j++) { acc0[j] = 0.f; acc1[j] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const wide_b8 av = *reinterpret_cast<const wide_b8 *>(dZ3s + r * S3 + (ks * 16 + 8 * h) * 2);
      const wide_b8 b0v = wide_ldfrag(W3T, t0, ks, 2, lane), b1v = wide_ldfrag(W3T, t0 + 1, ks, 2, lane);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b0v, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b1v, acc1, 0, 0, 0);
    }
    const int n0 = t0 * 32 + r, n1 = n0 + 32;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float v[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int m = 8 * q + 4 * h + i;
        const float x0 = bf16_widen(*reinterpret_cast<const unsigned short *>(H2s + m * S2 + 2 * n0));
        const float x1 = bf16_widen(*reinterpret_cast<const unsigned short *>(H2s + m * S2 + 2 * n1));
        v[i] = acc0[4 * q + i] * (1.f - x0 * x0); w[i] = acc1[4 * q + i] * (1.f - x1 * x1);
      }
      wide_put4(dZ2s, S2, 8 * q + 4 * h, n0, a.dz2T[trunk], B, b0 + 8 * q + 4 * h, v[0], v[1], v[2], v[3]);
      wide_put4(dZ2s, S2, 8 * q + 4 * h, n1, a.dz2T[trunk], B, b0 + 8 * q + 4 * h, w[0], w[1], w[2], w[3]);
      s0 += (v[0] + v[1]) + (v[2] + v[3]); s1 += (w[0] + w[1]) + (w[2] + w[3]);
    }
    if (a.bias_in_chain) {
      s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32);
      if (h == 0) { atomicAdd(&a.gb2[trunk][n0], s0); atomicAdd(&a.gb2[trunk][n1], s1); }
    }
  }
  __syncthreads();

  WPROF(6);
  // ---- d layer 1: dZ1 = (dZ2 W2) x (1 - H1^2).  A = dZ2 rows (K = H2), B[k = n][col = k1] = W2T row k1; four 32-column tiles per
  // wave share every A fragment; weight rows through a two-deep ring of four-k-step register blocks
  for (int t0 = 4 * wave; t0 < (H1 >> 5); t0 += 4 * WIDE_NW) {
    wide_f16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int j = 0; j < 16; j++) acc[q][j] = 0.f;
    const char *ap = dZ2s + r * S2 + 16 * h;
    const unsigned short *wrow = W2T + ((size_t)t0 * (H2 >> 4) * 64 + lane) * 8;     // tile t0 + q: + q * (H2 / 16) * 512 elements
    const size_t tstride = (size_t)(H2 >> 4) * 512;
    constexpr int KB = 4;
    wide_b8 pb[4][KB], qb[4][KB];
    const int nblk = (H2 >> 4) / KB;                       // H2 % 128 == 0: an even number of blocks
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int i = 0; i < KB; i++) pb[q][i] = *reinterpret_cast<const wide_b8 *>(wrow + q * tstride + i * 512);
    for (int kb = 0; kb < nblk; kb += 2) {
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < KB; i++) qb[q][i] = *reinterpret_cast<const wide_b8 *>(wrow + q * tstride + ((kb + 1) * KB + i) * 512);
#pragma unroll
      for (int i = 0; i < KB; i++) {
        const wide_b8 av = *reinterpret_cast<const wide_b8 *>(ap + (kb * KB + i) * 32);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, pb[q][i], acc[q], 0, 0, 0);
      }
      if (kb + 2 < nblk) {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
          for (int i = 0; i < KB; i++) pb[q][i] = *reinterpret_cast<const wide_b8 *>(wrow + q * tstride + ((kb + 2) * KB + i) * 512);
      }
#pragma unroll
      for (int i = 0; i < KB; i++) {
        const wide_b8 av = *reinterpret_cast<const wide_b8 *>(ap + ((kb + 1) * KB + i) * 32);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, qb[q][i], acc[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int n = (t0 + q) * 32 + r;
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float x = bf16_widen(*reinterpret_cast<const unsigned short *>(H1s + (8 * g + 4 * h + i) * S1 + 2 * n));
          v[i] = acc[q][4 * g + i] * (1.f - x * x);
        }
        wide_store_t4(a.dz1T[trunk], B, n, b0 + 8 * g + 4 * h, v[0], v[1], v[2], v[3]);
        s += (v[0] + v[1]) + (v[2] + v[3]);
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
    printf("wide_fwdbwd wg0 ticks: obs %llu layer1 %llu layer2 %llu head %llu loss %llu dlayer2 %llu dlayer1 %llu\n", wprof[1] - wprof[0], wprof[2] - wprof[1],
           wprof[3] - wprof[2], wprof[4] - wprof[3], wprof[5] - wprof[4], wprof[6] - wprof[5], wprof[7] - wprof[6]);
#endif
}

// dW = dZ^T X of the six layers and, in block 0, the loss scalars: dm_wide_common.h, a ring of two k-steps
__global__ void __launch_bounds__(64 * WIDE_WG_WAVES, 2) wide_wgrad_kernel(WideWgradArgs<1> a) {
  extern __shared__ __align__(16) float wide_wl[];      // 4 waves x 4 tiles x 4 KB
  wide_wgrad_body<1, 2>(a, wide_wl);
}

inline int wide_lds_bytes(int D, int H1, int H2) {
  const int z2 = WIDE_R * (2 * H2 + 16), rz = z2 > WIDE_NW * 4096 ? z2 : WIDE_NW * 4096;
  return WIDE_R * (2 * wide_dp(D) + 16) + WIDE_R * (2 * H1 + 16) + z2 + rz + WIDE_R * 80 + (32 * 33 + 16 * 36) * 4;
}
inline bool wide_supported(int B, int D, int H1, int H2, int A) {
  return B >= 64 && B % 64 == 0 && D >= 1 && D <= 112 && H1 % 256 == 0 && H1 >= 256 && H1 <= 1024 && H2 % 128 == 0 && H2 >= 128 && H2 <= 512 && A >= 1 &&
         A <= 32 && wide_lds_bytes(D, H1, H2) <= 160 * 1024;
}

}  // namespace

extern "C" long long dm_ppo_wide_packed_elems(int D, int H1, int H2) { return wide_plane_elems(D, H1, H2); }
extern "C" int dm_ppo_wide_dp(int D) { return wide_dp(D); }
extern "C" int dm_ppo_wide_supported(int B, int D, int H1, int H2, int A) { return wide_supported(B, D, H1, H2, A) ? 1 : 0; }

extern "C" int dm_ppo_wide_grad(const DmPpoWideStep *s, void *stream) {
  if (!s || !wide_supported(s->B, s->D, s->H1, s->H2, s->A)) return DM_EINVAL;
  return wide_launch<1, WideArgs>(s, (hipStream_t)stream, wide_pack_kernel, wide_fwdbwd_kernel, wide_wgrad_kernel, wide_lds_bytes(s->D, s->H1, s->H2));
}
