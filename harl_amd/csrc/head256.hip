// head256.hip -- plain action heads of 33..64 outputs on a 256-wide head input (gfx950): Categorical and DiagGaussian, log-prob
// pass and training pass (loss + backward up to dz_L).
//
// The 64 / 128-wide kernels of heads.hip hold x_hat_L of a slab in registers across the loss (H/8 float4 per lane: 128 VGPRs at
// H = 256) next to z[64], dzh[64] and the backward's H/32 accumulator tiles (128 more).  That does not fit a lane, so here x_hat_L
// is never held whole:
//
//   forward   z^T[64 x 32] = W'[64 x 256] x_hat_L^T on v_mfma_f32_32x32x2_f32, straight from the ATL image.  The float4 a lane
//             loads ARE the B operand: lane (i, h) holds sample i, and its partner lane i + 32 the feature 4 further on -- the
//             k-pair of the instruction -- so the activations need no transpose and no LDS round trip.  The A operand
//             W'[d][f .. f + 3 (+ 4 h)] is one ds_read_b128 of the row-major weight image wl[64][256 + 4] (staged once per
//             workgroup; the 4 floats of padding put the 16 rows of a read phase on 64 different banks).  x_hat_L streams
//             through half a slab (four K panels of 32 features, sixteen float4) ahead of the accumulators -- two output tiles
//             times four chains, one per K panel of a half (head256_fwd: shorter fp32 chains); 256 MFMAs per slab.
//             fp32 operands, no split: the products are exact to fp32 like the VALU heads', and at one wave per SIMD the matrix
//             pipe time of a slab (256 x 64 cycles) is about the time HBM needs to deliver it.
//   exchange  lane (i, h) then holds the 32 outputs d with bit 2 of d equal to h.  One v_permlane32_swap per accumulator
//             register hands both lanes both values: z[64] in every lane, as actor_sample / gauss_wide_sample expect.  The bias
//             is added here.
//   loss      actor_sample<64, true, ...> / gauss_wide_sample (heads_common.h): the arithmetic of the 64 / 128-wide heads, bit
//             for bit.
//   backward  dx_hat^T = W'^T dzh on the same MFMA, 64 features (two accumulator tiles) at a time: the panel's eight float4 of
//             x_hat_L are read again (the wave read them a few microseconds earlier: L2), its ONE ReLU-mask word per lane is
//             loaded as the panel starts, the LayerNorm means are the closed forms s1, s2 of the sample functions (see
//             head_bwd_stream), and dz_L leaves with the panel's float4 stores.  A operand: ds_read_b32 of the same image.
//   dhead     the ATL(64) image of store_dhead; the head's weight gradient is the ordinary ATL GEMM (dw_part = NULL).
#include "head256.h"

using namespace harl;

#include "heads_common.h"

namespace {

constexpr int H256 = 256;
constexpr int WLD = H256 + 4;  // row stride of wl: rows d, d + 1 start 4 banks apart

// wl[d][f] = W'[d][f] (rows >= act_dim zero); cst[0..64) = bias, cst[4 * 64 + d] = row sums, in stage_head's order of addition
__device__ __forceinline__ void stage_head256(float *wl, float *cst, const float *__restrict__ Whp, const float *__restrict__ bhp,
                                              int act_dim) {
  constexpr int DAP = LS_W;
  if ((reinterpret_cast<uintptr_t>(Whp) & 15) == 0) {
    for (int e4 = threadIdx.x; e4 < DAP * (H256 / 4); e4 += WG_THREADS) {
      const int d = e4 / (H256 / 4), k = 4 * (e4 % (H256 / 4));
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (d < act_dim) v = *reinterpret_cast<const f32x4 *>(Whp + d * H256 + k);
      *reinterpret_cast<f32x4 *>(wl + d * WLD + k) = v;
    }
  } else {
    for (int e = threadIdx.x; e < DAP * H256; e += WG_THREADS) {
      const int d = e / H256, k = e % H256;
      wl[d * WLD + k] = d < act_dim ? Whp[e] : 0.f;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < DAP; e += WG_THREADS) {
    cst[e] = e < act_dim ? bhp[e] : 0.f;
    float rs = 0.f;
    for (int f = 0; f < H256; ++f) rs += wl[e * WLD + f];
    cst[4 * DAP + e] = rs;
  }
}

// Half `g` of a slab's K range (features 128 g .. 128 g + 127 = four K panels of 32): the sixteen float4 of a lane
__device__ __forceinline__ void load_khalf(const float *__restrict__ xL, long slab, int g, int lane, f32x4 (&x)[16]) {
  const f32x4 *xp = reinterpret_cast<const f32x4 *>(xL + slab * (long)(H256 * SLAB)) + (16 * g) * WAVE + lane;
#pragma unroll
  for (int q = 0; q < 16; ++q) x[q] = xp[q * WAVE];
}

// z[d] = bias[d] + sum_f x_hat[f] W'[d][f] for the 64 head outputs, in both lanes of a sample.  `xn`: the first K half of this
// slab on entry; CARRY (log-prob pass): the first K half of slab `next` on return.  The training pass requests it behind the
// loss instead (k_head256), in flight while the backward's MFMAs run: 64 registers fewer live across actor_sample.
// Four accumulation chains per output tile, K panel j of a half on chain j: a sum of 256 products as four fp32 chains of 32
// two-product steps and a pairwise combine instead of one chain of 128 (a Gaussian head of 64 dimensions multiplies 64 ratios
// that each carry the rounding of its z; measured in profiles/r23_head64_256.md), and eight independent MFMAs back to back.
template <bool CARRY>
__device__ __forceinline__ void head256_fwd(const float *__restrict__ xL, long slab, long next, int lane, const float *wl,
                                            const float *cst, f32x4 (&xn)[16], float (&z)[LS_W]) {
  const int i = lane & 31, h = lane >> 5;
  const float *wa = wl + i * WLD + 4 * h;  // A[m = i][k = h] of k-step (q, c): W'[32 tile + i][feature(q) + c + 4 h]
  f32x16 acc[8];  // [chain j][tile]
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll 1
  for (int g = 0; g < 2; ++g) {
    f32x4 xv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) xv[q] = xn[q];
    if (g == 0) load_khalf(xL, slab, 1, lane, xn);
    else if (CARRY) load_khalf(xL, next, 0, lane, xn);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 a[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[2 * j] = *reinterpret_cast<const f32x4 *>(wa + 128 * g + 32 * j + 8 * q);
        a[2 * j + 1] = *reinterpret_cast<const f32x4 *>(wa + 32 * WLD + 128 * g + 32 * j + 8 * q);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[2 * j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * j][c], xv[4 * j + q][c], acc[2 * j], 0, 0, 0);
          acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * j + 1][c], xv[4 * j + q][c], acc[2 * j + 1], 0, 0, 0);
        }
    }
  }
  // register r of tile t: output d0 = 32 t + (r & 3) + 8 (r >> 2) in lane half 0, d0 + 4 in half 1.  v_permlane32_swap with both
  // operands = the register returns {half 0's value, half 1's value} in every lane (see wave_sum32, common.h).
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d0 = 32 * t + (r & 3) + 8 * (r >> 2);
      const unsigned u = __float_as_uint((acc[t][r] + acc[2 + t][r]) + (acc[4 + t][r] + acc[6 + t][r]));
      const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
      z[d0] = __uint_as_float(p[0]) + cst[d0];
      z[d0 + 4] = __uint_as_float(p[1]) + cst[d0 + 4];
    }
  __builtin_amdgcn_sched_barrier(0);  // (nothing of the loss moves up between the MFMAs: it spilled the Categorical training pass)
}

// dz_L of a slab, 64 features at a time (head_bwd_regs_bits's arithmetic per element; see head_bwd_stream for s1, s2)
__device__ __forceinline__ void head256_bwd(const float *__restrict__ xL, const uint32_t *__restrict__ mask_in, float rstd,
                                            long slab, int lane, const float *wl, const float (&dzh)[LS_W], float s1, float s2,
                                            float *__restrict__ dz_out) {
  constexpr int NW = 4;  // ReLU-mask words per lane at H = 256: word p = the 32 registers of panel p, MSB-first (common.h)
  const int i = lane & 31, h = lane >> 5;
  s1 *= (1.0f / H256);
  s2 *= (1.0f / H256);
  const f32x4 *xp = reinterpret_cast<const f32x4 *>(xL + slab * (long)(H256 * SLAB)) + lane;
  f32x4 *op = reinterpret_cast<f32x4 *>(dz_out + slab * (long)(H256 * SLAB)) + lane;
  const float *wa = wl + h * WLD + i;  // A[m = i][k = h] of k-step st, tile t of panel p: W'[2 st + h][64 p + 32 t + i]
  const unsigned hm = 0u - (unsigned)h;
#pragma unroll 1
  for (int p = 0; p < H256 / 64; ++p) {
    uint32_t b = mask_in[(slab * NW + p) * WAVE + lane];
    f32x4 xs[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) xs[q] = xp[(8 * p + q) * WAVE];
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
    for (int st = 0; st < LS_W / 2; ++st) {  // (entries >= act_dim of dzh are zero)
      const float bsel = __uint_as_float((__float_as_uint(dzh[2 * st + 1]) & hm) | (__float_as_uint(dzh[2 * st]) & ~hm));
#pragma unroll
      for (int t = 0; t < 2; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * st * WLD + 64 * p + 32 * t], bsel, acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float dx = acc[(4 * q + c) >> 4][(4 * q + c) & 15];
        const float da = rstd * (dx - s1 - xs[q][c] * s2);
        o[c] = (int)b < 0 ? da : 0.f;
        b <<= 1;
      }
      op[(8 * p + q) * WAVE] = o;
    }
  }
}

template <bool DISCRETE, bool TRAIN>
__global__ __launch_bounds__(WG_THREADS, 1) void k_head256(ActorArgs A) {
  constexpr int DAP = LS_W;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *wl = lds;                 // [64][WLD]
  float *cst = wl + DAP * WLD;     // bias, sigma, logsigma, dsigma_dlogstd, rowsum, 1/sigma, 1/sigma^2  [DAP each]
  float *red = cst + 7 * DAP;      // [4][PS_STRIDE]
  // Gaussian only (as k_gauss_head_wide):
  double *cd = reinterpret_cast<double *>(red + 4 * PS_STRIDE);  // fp64: 0.5 / sigma^2, log sigma + log sqrt(2 pi)  [DAP each]
  float *lst = reinterpret_cast<float *>(cd + 2 * DAP);          // TRAIN: [4 waves][LS_W][LS_TS] log_std tiles
  float *lsr = lst + WAVES_PER_WG * LS_W * LS_TS;                // TRAIN: [4 waves][LS_W]
  if (!DISCRETE && TRAIN)
    for (int e = threadIdx.x; e < WAVES_PER_WG * LS_W * LS_TS; e += WG_THREADS) lst[e] = 0.f;
  stage_head256(wl, cst, A.Whp, A.bhp, A.act_dim);
  if (!DISCRETE) {
    for (int e = threadIdx.x; e < DAP; e += WG_THREADS) {
      float sg = 0.5f, sig = 1.f, lsig = 0.f, dsd = 0.f;
      double sigd = 1.0;
      if (e < A.act_dim) {  // distributions.py:86-89: std = sigmoid(log_std / x_coef) * y_coef
        sg = 1.0f / (1.0f + expf(-A.log_std[e] / A.std_x_coef));
        sig = sg * A.std_y_coef;
        lsig = logf(sig);
        dsd = A.std_y_coef * sg * (1.f - sg) / A.std_x_coef;
        sigd = (double)A.std_y_coef / (1.0 + exp(-(double)A.log_std[e] / (double)A.std_x_coef));
      }
      cst[DAP + e] = sig;
      cst[2 * DAP + e] = lsig;
      cst[3 * DAP + e] = dsd;
      cst[5 * DAP + e] = 1.0f / sig;
      cst[6 * DAP + e] = 1.0f / (sig * sig);
      cd[e] = 0.5 / (sigd * sigd);  // the importance weight's own log-probs (gauss_wide_sample)
      cd[DAP + e] = log(sigd) + 0.91893853320467274178;
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = wave_id();
  const int i = lane & 31;
  float *lsw = lst + wave * (LS_W * LS_TS);

  float adv_mean = 0.f, adv_den = 1.f;
  if (TRAIN && A.adv_moments) {  // happo.py:122-127
    const double cnt = A.adv_moments[2];
    const double m = A.adv_moments[0] / cnt;
    const double var = A.adv_moments[1] / cnt - m * m;
    adv_mean = (float)m;
    adv_den = 1.0f / ((float)sqrt(var > 0 ? var : 0.0) + 1e-5f);  // reciprocal (the sample functions multiply)
  }
  // per-lane partial sums: 0 loss*active, 1 active, 2 ent*active, 3 ratio, 4 count (actor_sample's row has 64 unused slots behind)
  float sc[DISCRETE ? 8 + DAP : 8];
#pragma unroll
  for (int k = 0; k < (DISCRETE ? 8 + DAP : 8); ++k) sc[k] = 0.f;

  const long slab_first = (long)blockIdx.x * WAVES_PER_WG + wave, slab_step = (long)gridDim.x * WAVES_PER_WG;
  f32x4 xn[16];
  if (slab_first < A.n_slabs) load_khalf(A.xL, slab_first, 0, lane, xn);
  for (long slab = slab_first; slab < A.n_slabs; slab += slab_step) {
    const long next = slab + slab_step < A.n_slabs ? slab + slab_step : slab;
    float z[DAP], dzh[DAP];
    float s1, s2;
    if constexpr (DISCRETE) {
      ActorRow<DAP> row;  // (requested in front of the product: its loads land while the matrix pipe works)
      actor_row_load<DAP, true, TRAIN>(A, slab, lane, row);
      head256_fwd<!TRAIN>(A.xL, slab, next, lane, wl, cst, xn, z);
      if (!actor_sample<DAP, true, TRAIN>(A, cst, z, slab, lane, adv_mean, adv_den, sc, dzh, s1, s2, row)) continue;
    } else {
      head256_fwd<!TRAIN>(A.xL, slab, next, lane, wl, cst, xn, z);
      if (!gauss_wide_sample<TRAIN>(A, cst, cd, z, slab, lane, adv_mean, adv_den, sc, dzh, s1, s2, lsw)) continue;
    }
    if constexpr (TRAIN) {
      store_dhead<DAP>(A.dhead, slab, lane, dzh);
      load_khalf(A.xL, next, 0, lane, xn);  // (in flight while the backward's MFMAs run)
      head256_bwd(A.xL, A.relu_mask, A.rstd[slab * SLAB + i], slab, lane, wl, dzh, s1, s2, A.dzL);
    }
  }

  if constexpr (TRAIN) {
    float sc8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) sc8[k] = sc[k];
    block_reduce_store<8>(sc8, red, A.part_scalars + (long)blockIdx.x * PS_STRIDE);  // (its barrier: every wave's tile is complete)
    if constexpr (!DISCRETE) {  // part_ls epilogue of k_gauss_head_wide
      float t = 0.f;            // lane = dimension: the wave's 32 sample lanes in order
#pragma unroll 8
      for (int s = 0; s < SLAB; ++s) t += lsw[lane * LS_TS + s];
      lsr[wave * LS_W + lane] = t;
      __syncthreads();
      if (threadIdx.x < LS_W)
        A.part_ls[(long)blockIdx.x * LS_W + threadIdx.x] = (lsr[threadIdx.x] + lsr[LS_W + threadIdx.x]) +
                                                           (lsr[2 * LS_W + threadIdx.x] + lsr[3 * LS_W + threadIdx.x]);
    }
  }
}

// =============================================================================================
// HATRPO Fisher-vector product, head part, for a Categorical head of 33..64 actions on a 256-wide head input
// (k_actor_head_fvp<H, 64, true>'s arithmetic, heads.hip; trpo_util.py:132-158), built like k_head256: neither x_hat_L nor its
// tangent is ever held whole.
//
//   forward   z = W' x_hat, zd = W'_dot x_hat + W' x_hat_dot in ONE sweep over both ATL images, each read from HBM once per slab,
//             on the MFMA form of head256_fwd with BOTH weight images resident in LDS (wl, wdl: [64][256 + 4] each).  Per k-step
//             and output tile three products; the A fragment of W' serves both B operands and the B fragment of x_hat both A
//             fragments: 768 MFMAs per slab.  The images stream a QUARTER of a slab ahead (two K panels of 32 features, eight
//             float4 per image): with 2 x 128 accumulator registers a half of two images (128 registers current + 128
//             prefetched) does not fit next to them.
//   chains    z keeps head256_fwd's four chains per tile -- K panel p of the slab on chain p & 3, in head256_fwd's order, so z
//             is head256_fwd's z bit for bit.  zd gets TWO per tile, K panel p on chain p & 1, both of its products on the chain
//             of their panel (the W'_dot x_hat products are issued with z's, the W' x_hat_dot ones four MFMAs later): 192
//             accumulator registers.  With four chains for zd as well (256: every AGPR) the compiler kept 12 .. 16 bytes of
//             scratch per lane whatever else was tried (profiles/r24_trpo_head64_256.md); zd enters dzh linearly, without the
//             cancellation that made z's chain length matter.  The K loop is unrolled whole: rolled over the halves, the
//             accumulators were spilled at the loop's back edge.
//   exchange  one v_permlane32_swap per accumulator register, for z (kept before the bias: zlin) and for zd (+ b'_dot).
//   Hessian   k_actor_head_fvp's Categorical branch in registers; the availability row is folded into two mask words per lane
//             BEFORE the sweep, entries >= act_dim take part as logits of -1e10 like unavailable ones (exp = 0 exactly: the sums
//             are those of the d < act_dim loops), and the masked logit is re-formed from zlin where it is used, so that next to
//             zd and dzh only zlin is live.
//   backward  store_dhead<64>, s1 / s2, head256_bwd -- unchanged; the next slab's first quarter is requested in front of it.
// =============================================================================================
constexpr int CST256 = 5 * LS_W;  // a stage_head256 constant block: bias at 0, row sums at 4 * 64

// Quarter `u` of a slab's K range (features 64 u .. 64 u + 63 = two K panels of 32): the eight float4 of a lane
__device__ __forceinline__ void load_kquarter(const float *__restrict__ xL, long slab, int u, int lane, f32x4 (&x)[8]) {
  const f32x4 *xp = reinterpret_cast<const f32x4 *>(xL + slab * (long)(H256 * SLAB)) + (8 * u) * WAVE + lane;
#pragma unroll
  for (int q = 0; q < 8; ++q) x[q] = xp[q * WAVE];
}

// zl[d] = sum_f x_hat[f] W'[d][f] (no bias) and zd[d] = b'_dot[d] + sum_f (x_hat[f] W'_dot[d][f] + x_hat_dot[f] W'[d][f]), in
// both lanes of a sample.  xn / xdn: the first K quarter of this slab's two images on entry.
__device__ __forceinline__ void head256_fvp_fwd(const float *__restrict__ xL, const float *__restrict__ xLd, long slab, int lane, const float *wl, const float *wdl, const float *cdt, f32x4 (&xn)[8],
                                                f32x4 (&xdn)[8], float (&zl)[LS_W], float (&zd)[LS_W]) {
  const int i = lane & 31, h = lane >> 5;
  const float *wa = wl + i * WLD + 4 * h, *wda = wdl + i * WLD + 4 * h;  // A[m = i][k = h], as head256_fwd
  f32x16 acc[8], accd[4];  // [chain][tile]: four chains for z, two for zd
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[t][r] = 0.f;
      if (t < 4) accd[t][r] = 0.f;
    }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {  // quarter u = 2 g + uu: K panels 2 u, 2 u + 1 -> chains 2 uu, 2 uu + 1
      f32x4 xv[8], xdv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        xv[q] = xn[q];
        xdv[q] = xdn[q];
      }
      if (uu == 0 || g == 0) {  // (the next slab's first quarter is requested behind the Hessian: k_head256_fvp)
        load_kquarter(xL, slab, 2 * g + uu + 1, lane, xn);
        load_kquarter(xLd, slab, 2 * g + uu + 1, lane, xdn);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 a[4], ad[4];  // [panel jj][tile]
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int o = 32 * t * WLD + 128 * g + 64 * uu + 32 * jj + 8 * q;
            a[2 * jj + t] = *reinterpret_cast<const f32x4 *>(wa + o);
            ad[2 * jj + t] = *reinterpret_cast<const f32x4 *>(wda + o);
          }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const int ch = 2 * (2 * uu + jj) + t;
              acc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * jj + t][c], xv[4 * jj + q][c], acc[ch], 0, 0, 0);
              accd[2 * jj + t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad[2 * jj + t][c], xv[4 * jj + q][c], accd[2 * jj + t], 0, 0, 0);
            }
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              accd[2 * jj + t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * jj + t][c], xdv[4 * jj + q][c], accd[2 * jj + t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // (the weight reads of later steps stay where they are: hoisted, they spill)
      }
    }
  }
  // (register r of tile t: output d0 = 32 t + (r & 3) + 8 (r >> 2) in lane half 0, d0 + 4 in half 1 -- see head256_fwd)
  asm volatile("" : "+v"(cdt));  // (one base register and immediate offsets: as constants the 64 LDS addresses sit in SGPRs, which spill)
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d0 = 32 * t + (r & 3) + 8 * (r >> 2);
      const unsigned u = __float_as_uint((acc[t][r] + acc[2 + t][r]) + (acc[4 + t][r] + acc[6 + t][r]));
      const unsigned ud = __float_as_uint(accd[t][r] + accd[2 + t][r]);
      const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
      const auto pd = __builtin_amdgcn_permlane32_swap(ud, ud, false, false);
      zl[d0] = __uint_as_float(p[0]);
      zl[d0 + 4] = __uint_as_float(p[1]);
      zd[d0] = __uint_as_float(pd[0]) + cdt[d0];
      zd[d0 + 4] = __uint_as_float(pd[1]) + cdt[d0 + 4];
    }
  __builtin_amdgcn_sched_barrier(0);  // (nothing of the Hessian moves up between the MFMAs, as in head256_fwd)
}

__global__ __launch_bounds__(WG_THREADS, 1) void k_head256_fvp(FvpArgs A) {
  constexpr int DAP = LS_W;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *wl = lds;               // [64][WLD]  W'
  float *wdl = wl + DAP * WLD;   // [64][WLD]  W'_dot
  float *cst = wdl + DAP * WLD;  // bias, row sums of W'
  float *cdt = cst + CST256;     // bias_dot (+ the row sums of W'_dot, unused)
  stage_head256(wl, cst, A.Whp, A.bhp, A.act_dim);
  stage_head256(wdl, cdt, A.Whdp, A.bhdp, A.act_dim);
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = wave_id();
  const int i = lane & 31;
  const int D = A.act_dim;
  const long slab_first = (long)blockIdx.x * WAVES_PER_WG + wave, slab_step = (long)gridDim.x * WAVES_PER_WG;
  f32x4 xn[8], xdn[8];
  if (slab_first < A.n_slabs) {
    load_kquarter(A.xL, slab_first, 0, lane, xn);
    load_kquarter(A.xLdot, slab_first, 0, lane, xdn);
  }
  for (long slab = slab_first; slab < A.n_slabs; slab += slab_step) {
    const long next = slab + slab_step < A.n_slabs ? slab + slab_step : slab;
    int ls = 0;
    asm volatile("" : "+v"(ls));
    ls = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, ls));  // (a slab's addresses are formed in the slab: carried from the kernel's top, they spill)
    // bit d of un[d >> 5]: entry d exists and is available (the row is read in front of the product; clamped index: no load
    // under a per-entry branch)
    uint32_t un[2] = {0u, 0u};
    {
      const long j = slab * SLAB + (ls & 31);
      const long jc = j < A.M ? j : A.M - 1;  // (a padding sequence's own row instead of row M - 1: its dzh is 0 either way)
      const float *av = A.avail ? A.avail + jc * D : A.Whp;  // (absent: a mapped dummy row, not consulted)
#pragma unroll
      for (int c = 0; c < DAP / 16; ++c) {
        int Dc = D;
        asm volatile("" : "+s"(Dc));  // opaque per chunk: hoisted out of the slab loop, the 64 width tests live in SGPRs that spill
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int d = 16 * c + k;
          const float v = av[d < Dc ? d : 0];
          if (d < Dc && !(A.avail && v == 0.f)) un[d >> 5] |= 1u << (d & 31);
        }
        __builtin_amdgcn_sched_barrier(0);  // (sixteen loads in flight at a time, and none between the MFMAs)
      }
    }
    float zl[DAP], zd[DAP], dzh[DAP];
    head256_fvp_fwd(A.xL, A.xLdot, slab, ls, wl, wdl, cdt, xn, xdn, zl, zd);

    // Entries >= D ride along at -1e10 like unavailable ones: the maximum is an available logit, so their exp is exactly 0 and
    // every sum below is the sum of k_actor_head_fvp's d < D loop.  Four sweeps of four chunks: the mask word is re-read as an
    // opaque value per chunk and nothing crosses a chunk's end -- left free, hipcc keeps the 64 lane masks of the first sweep
    // in SGPRs for the other three and interleaves all 128 exponentials, and both spill.
#define HEAD256_FVP_CHUNK(BODY)                                                   \
  _Pragma("unroll") for (int c = 0; c < DAP / 16; ++c) {                          \
    uint32_t w = un[c >> 1] >> (16 * (c & 1));                                    \
    const float *cs = cst;                                                        \
    asm volatile("" : "+v"(w), "+v"(cs)); /* (cs: immediate offsets from ONE base) */  \
    _Pragma("unroll") for (int k = 0; k < 16; ++k) {                              \
      const int d = 16 * c + k;                                                   \
      const bool open = (w >> k) & 1u;                                            \
      const float zm = open ? zl[d] + cs[d] : -1e10f;  /* the masked logit */     \
      BODY                                                                        \
    }                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                            \
  }
    float mx = -3.0e38f;
    HEAD256_FVP_CHUNK(mx = fmaxf(mx, zm);)
    float se = 0.f;
    HEAD256_FVP_CHUNK(se += expf(zm - mx);)
    const float lse = mx + logf(se);
    float S = 0.f, sum_zd = 0.f;
    HEAD256_FVP_CHUNK(const float pr = expf(zm - lse); dzh[d] = pr; if (open) { S += pr * zd[d]; sum_zd += zd[d]; })
    const float sum_dq = sum_zd - (float)D * S;  // sum over ALL D entries of q_dot_d = [unmasked] zd_d - S
    float s1 = 0.f, s2 = 0.f;
    int lb = ls;
    asm volatile("" : "+v"(lb));  // (the row's validity and the backward's addresses are formed here, not carried across the sweep)
    const long j = slab * SLAB + (lb & 31);
    const bool valid = j < A.M && (A.m_pad == 0 || (j % A.m_pad) < A.m_valid);
    HEAD256_FVP_CHUNK((void)zm; dzh[d] = open && valid ? (zd[d] - S) - dzh[d] * sum_dq : 0.f;  // log-softmax backward of dq = q_dot
                      s1 += dzh[d] * cs[4 * DAP + d]; s2 += dzh[d] * zl[d];)
#undef HEAD256_FVP_CHUNK
    store_dhead<DAP>(A.dhead, slab, lb, dzh);
    load_kquarter(A.xL, next, 0, lb, xn);  // (in flight while the backward's MFMAs run)
    load_kquarter(A.xLdot, next, 0, lb, xdn);
    head256_bwd(A.xL, A.relu_mask, A.rstd[slab * SLAB + (lb & 31)], slab, lb, wl, dzh, s1, s2, A.dzL);
  }
}

template <bool DISCRETE, bool TRAIN>
void launch(const ActorArgs &A, int grid, hipStream_t s) {
  size_t fl = (size_t)LS_W * WLD + 7 * LS_W + 4 * PS_STRIDE;  // 65 KiB of weights + constants + the scalar reduction
  if (!DISCRETE) fl += 2 * 2 * LS_W;                          // 2 x LS_W doubles
  if (!DISCRETE && TRAIN) fl += (size_t)WAVES_PER_WG * LS_W * LS_TS + (size_t)WAVES_PER_WG * LS_W;  // log_std tiles + wave sums: 101.5 KiB
  const size_t shm = fl * sizeof(float);
  allow_big_lds(k_head256<DISCRETE, TRAIN>, shm);
  hipLaunchKernelGGL((k_head256<DISCRETE, TRAIN>), dim3(grid), dim3(WG_THREADS), shm, s, A);
}
}  // namespace

void harl::launch_head256(const void *actor_args, bool discrete, bool train, int grid, hipStream_t s) {
  const ActorArgs &A = *static_cast<const ActorArgs *>(actor_args);
  if (discrete) {
    if (train) launch<true, true>(A, grid, s);
    else launch<true, false>(A, grid, s);
  } else {
    if (train) launch<false, true>(A, grid, s);
    else launch<false, false>(A, grid, s);
  }
}

void harl::launch_head256_fvp(const void *fvp_args, int grid, hipStream_t s) {
  const FvpArgs &A = *static_cast<const FvpArgs *>(fvp_args);
  const size_t shm = ((size_t)2 * LS_W * WLD + 2 * CST256) * sizeof(float);  // two weight images + constants: 132.5 KiB
  allow_big_lds(k_head256_fvp, shm);
  hipLaunchKernelGGL(k_head256_fvp, dim3(grid), dim3(WG_THREADS), shm, s, A);
}
