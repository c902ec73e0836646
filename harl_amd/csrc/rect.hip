// rect.hip -- layers with a 256-wide side and a narrower one (harl/models/base/mlp.py:7-70 with hidden_sizes such as
// [256, 128], [128, 256] or [256, 128, 64]), gfx950.  Opt-in route HARL_MIXED_256=1 (harl_amd/configs.py).
//
// panel.hip walks K in panels because three bf16 images of a 256-row matrix do not fit the LDS; its k_panel is built around
// eight accumulator tiles (128 registers) and a 32-column panel.  A layer 256 -> 64 / 128 has 2 / 4 output row tiles, and its
// backward (rows = 256 input features) reduces over 64 / 128 columns only.  k_panel_rect<MT, MODE> is the K-panel walk for
// MT = 2 / 4 / 8 row tiles with the geometry chosen per MT:
//
//   unit      A SUB-PANEL is 32 columns (2 k-steps of v_mfma_f32_32x32x16_bf16) of all 32 MT rows: 3 terms x MT x 2 fragments
//             x 1 KiB.  It is what split_gemm<MT, 2> multiplies and what a short last panel is counted in.
//   panel     8 / MT sub-panels = 48 KiB of images whatever MT is: 128 columns at MT = 2, 64 at MT = 4, 32 at MT = 8.  A
//             256-column reduction is 2 / 4 / 8 panels, i.e. a quarter / half the barriers of k_panel at MT = 2 / 4.  KP = 96 at
//             MT = 4 is one full panel and one of a single sub-panel.
//   slabs     one slab (32 rows) per wave, four per workgroup iteration as in k_panel: the matrix streams from L2 once per 128
//             rows and the tail logic (dead waves of the last iteration stage and meet every barrier, write nothing) is the same.
//   prefetch  a panel is 1024 fragments per term = 4 per thread = 32 fp32 weights.  They are loaded into registers for panel
//             p + 1 BEFORE panel p is multiplied and split into LDS after it, so the L2 latency of the weights lies under the
//             MFMAs instead of in front of them (k_panel loads, splits and writes between two barriers).  The slab's own x
//             columns of panel p are loaded in front of that prefetch: vector loads return in order, and the first MFMA must
//             not wait for the weights of the NEXT panel.
//   MT 2 / 4  32 / 64 accumulator registers: the kernel fits 256 registers, __launch_bounds__(256, 2), ONE 48 KiB buffer and
//             two workgroups per CU (96 of 160 KiB).  The second wave of a SIMD multiplies while the first splits weights or
//             runs its LayerNorm epilogue -- overlap a second buffer in the same workgroup cannot give, because a wave's own
//             split and its own MFMAs are one instruction stream.  Two barriers per panel (filled / drained).
//   MT 8      128 accumulator registers + the LayerNorm backward's x_hat and output (3 x 128 live at its peak): one wave per
//             SIMD, as k_panel.  Nothing shares the SIMD, and 160 KiB belong to one workgroup: TWO 48 KiB buffers, panel p + 1
//             is written while others still read panel p, one barrier per panel (8 per slab where k_panel has 16).
//   forward  : x_hat_out = norm(relu(W' x_in + b'))            x_in = ATL(KP) image, KP a multiple of 32 up to 512
//   backward : dz_in = relu' . LNbwd(W'^T dz_out)               (HI, HO) over {64, 128, 256}^2
//   tangent  : x_out_dot = LNjac(mask . (W'_dot x_in + b'_dot [+ W' x_in_dot]))   HATRPO's Fisher-vector product on these trunks
//              (opt-in HARL_TRPO_MIXED_256=1): both products are ONE stream of sub-panels through the same prefetch pipeline
//   ACT 1..4 : forward x_hat_out = norm(act(W' x_in + b')), backward dz_in = act'(a) . LNbwd(W'^T dz_out) for leaky_relu / tanh /
//              sigmoid / selu (opt-in HARL_ACT_256=1): the same walk, another epilogue (see k_panel_rect); tangent x_out_dot =
//              LNjac(act'(a) . (W'_dot x_in + b'_dot [+ W' x_in_dot])) (opt-in HARL_TRPO_ACT_256=1): MODE 2's stream, another epilogue
// The GEMM is split_mfma.h's exact three-term bf16 split, six products, fp32 accumulation; x_hat / ReLU mask words / rstd
// leave in the layouts of the 64 / 128-wide layer kernels (fwd_epilogue.h) and of k_panel, so the head kernels,
// harl_mlp_dw_partials and harl_mlp_bwd_dx read them unchanged.  Rows past M inside the last slab are computed like any
// other: they never enter a sum because dz is 0 there (the loss kernels write it so, and LNbwd of a zero row is a zero row).
#include "common.h"
#include "act_funcs.h"
#include "split_mfma.h"
#include "../../include/harl_hip.h"

using namespace harl;

namespace {
int bad(const char *m) {
  set_error(m);
  return -2;
}

constexpr int PANEL_FRAGS = 1024;                    // u32x4 fragments per term and panel (16 KiB): 8 / MT sub-panels
constexpr int PER_THREAD = PANEL_FRAGS / WG_THREADS;  // 4 fragments = 32 fp32 weights per thread and panel

// the fp32 weights of panel p (sub-panels NSUB p .. NSUB p + nsub - 1) that this thread splits, into registers.
//   TRANSPOSED = false: A[row][k] = Wp[row * ldw + k]  (k < kvalid, else 0)       forward, Wp = [32 MT][ldw]
//   TRANSPOSED = true : A[row][k] = Wp[k * ldw + row]                              backward dX, Wp = [K][32 MT]
// Fragment e of a panel: sub-panel e / (128 MT), then [tile][k-step j][lane] as split_gemm<MT, 2> reads it.
// Addresses: fragment u of a thread differs from its fragment 0 by a whole sub-panel or by whole row tiles, and register c of
// a fragment by the constant feat_base(c), so every load is (scalar base of (u, c)) + ONE lane offset per thread -- 32 lane
// addresses would otherwise stay live across the panel loop, next to the accumulators of two waves per SIMD.
// TWO (the tangent's two-operand reduction): the reduction is ONE stream of sub-panels, of which the first n_first belong to
// (Wp, ldw, kvalid) and the following ones to the second matrix (W2 = [32 MT][ld2], every column valid).  Which of the two a
// sub-panel reads is workgroup-uniform, so it costs scalar selects and one more lane offset per thread; a panel may hold
// sub-panels of both.  TWO = false never looks at the three extra arguments.
template <int MT, bool TRANSPOSED, bool TWO>
__device__ __forceinline__ void load_panel(float (&w)[PER_THREAD][8], const float *__restrict__ Wp, int ldw, int kvalid,
                                           const float *__restrict__ W2, int ld2, int n_first, int p, int nsub) {
  static_assert(!(TWO && TRANSPOSED), "the two-operand stream is a forward-form reduction");
  constexpr int SUB = MT * 128, NSUB = 8 / MT;
  const int r0 = threadIdx.x % SUB, ln = r0 & 63, j = (r0 >> 6) & 1, m0 = 32 * (r0 >> 7) + (ln & 31), kl = 16 * j + 4 * (ln >> 5);
  const unsigned voff = TRANSPOSED ? (unsigned)(kl * ldw + m0) : (unsigned)(m0 * ldw + kl);
  const unsigned voff2 = TWO ? (unsigned)(m0 * ld2 + kl) : 0u;
#pragma unroll
  for (int u = 0; u < PER_THREAD; ++u) {
    const int sub = (u * WG_THREADS) / SUB;          // (compile time per u: 256 threads never straddle a sub-panel)
    const int dm = 32 * (((u * WG_THREADS) % SUB) >> 7);  // ... and this fragment's rows are dm below those of fragment 0
    int g = p * NSUB + sub;                          // the sub-panel's place in the stream, then in its own matrix
    const float *Wm = Wp;
    int ld = ldw, kv = kvalid;
    unsigned vo = voff;
    if constexpr (TWO) {
      if (g >= n_first) {  // (workgroup-uniform)
        g -= n_first;
        Wm = W2;
        ld = kv = ld2;
        vo = voff2;
      }
    }
    const int ks = 32 * g;
    if (sub < nsub) {  // (workgroup-uniform)
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int kc = ks + feat_base(c);  // k = kc + kl
        const float *base = TRANSPOSED ? Wm + (kc * ld + dm) : Wm + (dm * ld + kc);
        const bool in = kc + kl < kv;
        const float v = base[in ? vo : 0u];
        w[u][c] = in ? v : 0.f;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) w[u][c] = 0.f;
    }
  }
}

// ... split (round to nearest) and written as the three images of the panel: buf[sub][term][tile][j][lane]
template <int MT>
__device__ __forceinline__ void commit_panel(u32x4 *__restrict__ buf, const float (&w)[PER_THREAD][8], int nsub) {
  constexpr int SUB = MT * 128;
#pragma unroll
  for (int u = 0; u < PER_THREAD; ++u) {
    const int sub = (u * WG_THREADS) / SUB;
    if (sub >= nsub) continue;  // (workgroup-uniform)
    const int r = (threadIdx.x + u * WG_THREADS) % SUB;
    unsigned q[3][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) split3_rne(w[u][2 * c], w[u][2 * c + 1], q[0][c], q[1][c], q[2][c]);
#pragma unroll
    for (int term = 0; term < 3; ++term) buf[(sub * 3 + term) * SUB + r] = u32x4{q[term][0], q[term][1], q[term][2], q[term][3]};
  }
}

// the slab's 32 columns of sub-panel s: pieces 4 s .. 4 s + 3 of its ATL(KP) image (xp = the slab's image + lane).  TWO: from
// sub-panel n_first on, pieces 4 (s - n_first) .. of the slab's second image xp2 (load_panel's stream)
template <bool TWO>
__device__ __forceinline__ void load_cols(const f32x4 *__restrict__ xp, const f32x4 *__restrict__ xp2, int n_first, int s,
                                          float (&x)[16]) {
  if constexpr (TWO) {
    if (s >= n_first) {  // (workgroup-uniform)
      s -= n_first;
      xp = xp2;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = xp[(4 * s + q) * WAVE];
    x[4 * q + 0] = v[0];
    x[4 * q + 1] = v[1];
    x[4 * q + 2] = v[2];
    x[4 * q + 3] = v[3];
  }
}

// A kernel argument as the loop body sees it anew in every workgroup iteration.  What depends on it (the bias values, the lane
// addresses of the epilogue's loads and stores) is then formed where it is used instead of once in front of the loop, where it
// would hold registers for the kernel's lifetime -- the difference between 256 registers and a spill at two waves per SIMD.
template <typename T>
__device__ __forceinline__ T *per_iteration(T *p) {
  asm volatile("" : "+s"(p));
  return p;
}

// MODE 0 forward, 1 backward, 2 forward-mode tangent (HATRPO's Fisher-vector product):
//   z_dot = Wp (= W'_dot) x_in + bp (= b'_dot) [+ W2 (= W') x_in2 (= x_in_dot)],  x_out_dot = LNjac(mask . z_dot) with the PRIMAL
//   x_hat / mask / rstd of this layer in xprev / mask_prev / rstd_prev.  The two products are one stream of n_first + ld2 / 32
//   sub-panels (load_panel): the prefetch / commit pipeline below never learns where one operand ends, a panel may straddle the
//   boundary (MT = 2, 64 -> 64: the whole K = 128 reduction is ONE panel), and there is no drain between the operands.  n_first
//   counts the sub-panels that hold a valid column of Wp; the columns of x_in past them would meet zero weights and are skipped.
//
// ACT 0 is ReLU, everything above.  ACT 1..4 (act_funcs.h: leaky_relu, tanh, sigmoid, selu; opt-in HARL_ACT_256=1) changes
// the EPILOGUE only, where every accumulator of the slab already sits in this wave's registers -- the composed 64 / 128 route
// (raw GEMM, harl_act_ln_fwd, harl_act_bwd) sends the pre-activation image through HBM for the same arithmetic:
//   forward  : a = act(acc), x_hat = LayerNorm(a) in the two-pass form below; the record is x_hat, mean(a), rstd (mean_out,
//              rstd_out) and there are no mask words -- the backward rebuilds a = x_hat / rstd + mean from it
//   backward : dz_prev = act'(a) . LNbwd(W'^T dz) with act' taken from the value a (mean_prev, rstd_prev), multiplied into the
//              LayerNorm backward's output in place: at MT = 8 nothing joins acc / x_hat / out, the three 128-register arrays
//              live at the ReLU epilogue's peak.  A zero dz row still gives a zero row (0 times a finite slope).
//   tangent  : (HATRPO on these networks, opt-in HARL_TRPO_ACT_256=1) the K loop is MODE 2's, two operands in one stream; the
//              epilogue rebuilds a from the same record with the backward's own arithmetic -- the slope the Fisher-vector
//              product's forward half multiplies by is bit for bit the one its backward half multiplies by -- and multiplies
//              act'(a) into the ACCUMULATORS in place, where the ReLU tangent pops mask bits; the LayerNorm Jacobian then runs on
//              them as it does there (acc / x_hat / out at MT = 8 again).  No mask words are read.  The composed 64 / 128 route
//              (two raw harl_mlp_linear, harl_act_ln_tangent) is three launches and two pre-activation images through HBM.
template <int MT, int MODE, int ACT = 0>
__global__ __launch_bounds__(WG_THREADS, MT == 8 ? 1 : 2) void k_panel_rect(
    const float *__restrict__ xin, int KP, const float *__restrict__ Wp, int ldw, int kvalid, const float *__restrict__ bp,
    float *__restrict__ xout, uint32_t *__restrict__ mask_out, float *__restrict__ rstd_out, const float *__restrict__ xprev,
    const uint32_t *__restrict__ mask_prev, const float *__restrict__ rstd_prev, long n_slabs,
    const float *__restrict__ xin2 = nullptr, const float *__restrict__ W2 = nullptr, int ld2 = 0, int n_first = 0,
    float *__restrict__ mean_out = nullptr, const float *__restrict__ mean_prev = nullptr) {
  static_assert(ACT >= 0 && ACT <= 4 && MODE >= 0 && MODE <= 2, "relu and the four of act_funcs.h; forward, backward, tangent");
  constexpr bool BWD = MODE == 1, TWO = MODE == 2;
  constexpr int H = 32 * MT, NSUB = 8 / MT, NBUF = MT == 8 ? 2 : 1, SUB = MT * 128, BUF = 3 * PANEL_FRAGS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4 *img = reinterpret_cast<u32x4 *>(lds);
  const int lane = threadIdx.x & 63, wave = wave_id(), i = lane & 31, h = lane >> 5;
  const int n_sub = TWO ? n_first + (xin2 ? ld2 / 32 : 0) : KP / 32, n_panels = (n_sub + NSUB - 1) / NSUB;
  const long n_iter = (n_slabs + WAVES_PER_WG - 1) / WAVES_PER_WG;
  for (long it = blockIdx.x; it < n_iter; it += gridDim.x) {  // uniform trip count: barriers inside
    const long s_raw = it * WAVES_PER_WG + wave;
    const bool live = s_raw < n_slabs;
    const long slab = live ? s_raw : n_slabs - 1;
    const f32x4 *xp = reinterpret_cast<const f32x4 *>(xin + slab * (long)KP * SLAB) + lane;
    const f32x4 *xp2 = TWO ? reinterpret_cast<const f32x4 *>(xin2 + slab * (long)ld2 * SLAB) + lane : nullptr;  // (never read without xin2)
    f32x16 acc[MT];
    // (the bias is read again every iteration: hoisted out of this loop it would hold 16 MT registers for the kernel's lifetime)
    const float *bpi = per_iteration(bp);
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = BWD ? 0.f : bpi[32 * t + (r & 3) + 8 * (r >> 2) + 4 * h];
    float w[PER_THREAD][8];
    int nsub_p = n_sub < NSUB ? n_sub : NSUB;
    load_panel<MT, BWD, TWO>(w, Wp, ldw, kvalid, W2, ld2, n_first, 0, nsub_p);
    __syncthreads();  // the last panel of the iteration before is no longer being read
    commit_panel<MT>(img, w, nsub_p);
    for (int p = 0; p < n_panels; ++p) {
      // this slab's columns of the panel's first sub-panel, then the prefetch; the columns of sub-panel s + 1 are asked for
      // while sub-panel s multiplies (by then the prefetch in front of them has long returned)
      float xa[16];
      load_cols<TWO>(xp, xp2, n_first, p * NSUB, xa);
      const bool more = p + 1 < n_panels;
      const int rest = n_sub - (p + 1) * NSUB, nsub_next = rest < NSUB ? rest : NSUB;
      if (more) load_panel<MT, BWD, TWO>(w, Wp, ldw, kvalid, W2, ld2, n_first, p + 1, nsub_next);
      __syncthreads();  // panel p is complete (and, with two buffers, panel p - 1 is no longer being read)
      const u32x4 *wl = img + (p % NBUF) * BUF + lane;
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
        if (sub < nsub_p) {
          u32x4 x1[2], x2[2], x3[2];
          split_acts<16>(xa, x1, x2, x3);
          float xb[16];
          if (sub + 1 < nsub_p) load_cols<TWO>(xp, xp2, n_first, p * NSUB + sub + 1, xb);
          split_gemm<MT, 2>(wl + sub * 3 * SUB, x1, x2, x3, acc, [](int) {});
          if (sub + 1 < nsub_p) {
#pragma unroll
            for (int c = 0; c < 16; ++c) xa[c] = xb[c];
          }
        }
      if (more) {
        if (NBUF == 1) __syncthreads();  // one buffer: every wave has drained panel p
        commit_panel<MT>(img + ((p + 1) % NBUF) * BUF, w, nsub_next);
      }
      nsub_p = nsub_next;
    }
    if (!live) continue;
    constexpr int NR = H / 2, NW = (NR + 31) / 32;
    float *xo = per_iteration(xout);
    if constexpr (TWO && ACT != 0) {  // the block below with act'(a) from the value record in the place of the mask bits
      float xh[NR], ad[NR];
      atl_load<H>(per_iteration(xprev), slab, lane, xh);
      const float rstd = per_iteration(rstd_prev)[slab * SLAB + i], mean = per_iteration(mean_prev)[slab * SLAB + i];
      {
#pragma clang fp contract(off)
        const float sd = 1.0f / rstd;  // (the backward's rebuild of a, operation for operation)
#pragma unroll
        for (int R = 0; R < NR; ++R) acc[R >> 4][R & 15] *= act_slope_from_value(xh[R] * sd + mean, ACT);
      }
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        const float d = acc[R >> 4][R & 15];
        s1 += d;
        s2 += d * xh[R];
      }
      s1 = wave_sum32(s1) * (1.0f / H);
      s2 = wave_sum32(s2) * (1.0f / H);
#pragma unroll
      for (int R = 0; R < NR; ++R) ad[R] = rstd * (acc[R >> 4][R & 15] - s1 - xh[R] * s2);
      atl_store<H>(xo, slab, lane, ad);
    } else if constexpr (TWO) {  // mlp.hip's ln_jac_store on registers: nothing of it is addressed before the panel loop has ended
      float xh[NR], ad[NR];
      atl_load<H>(per_iteration(xprev), slab, lane, xh);
      const uint32_t *mi = per_iteration(mask_prev);
      uint32_t bits[NW];
#pragma unroll
      for (int wd = 0; wd < NW; ++wd) bits[wd] = mi[(slab * NW + wd) * WAVE + lane];
      const float rstd = per_iteration(rstd_prev)[slab * SLAB + i];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        ad[R] = mask_pop(acc[R >> 4][R & 15], bits[R >> 5]);
        s1 += ad[R];
        s2 += ad[R] * xh[R];
      }
      s1 = wave_sum32(s1) * (1.0f / H);
      s2 = wave_sum32(s2) * (1.0f / H);
#pragma unroll
      for (int R = 0; R < NR; ++R) ad[R] = rstd * (ad[R] - s1 - xh[R] * s2);
      atl_store<H>(xo, slab, lane, ad);
    } else if constexpr (ACT != 0 && !BWD) {  // elementwise.hip's k_act_ln_fwd on the accumulators
#pragma clang fp contract(off)
      float v[NR];
      float sum = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        v[R] = act_value(acc[R >> 4][R & 15], ACT);
        sum += v[R];
      }
      sum = wave_sum32(sum);
      const float mean = sum * (1.0f / H);
      float vs = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        v[R] -= mean;
        vs += v[R] * v[R];
      }
      vs = wave_sum32(vs);
      const float rstd = 1.0f / sqrtf(vs * (1.0f / H) + 1e-5f);
#pragma unroll
      for (int R = 0; R < NR; ++R) v[R] *= rstd;
      atl_store<H>(xo, slab, lane, v);
      if (lane < 32) {
        per_iteration(mean_out)[slab * SLAB + lane] = mean;
        per_iteration(rstd_out)[slab * SLAB + lane] = rstd;
      }
    } else if constexpr (ACT != 0) {  // ln_bwd_relu_mbits without the mask words, then k_act_bwd's slope on its output
      float xh[NR], out[NR];
      atl_load<H>(per_iteration(xprev), slab, lane, xh);
      const float rstd = per_iteration(rstd_prev)[slab * SLAB + i], mean = per_iteration(mean_prev)[slab * SLAB + i];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        const float d = acc[R >> 4][R & 15];
        s1 += d;
        s2 = __builtin_fmaf(d, xh[R], s2);
      }
      s1 = wave_sum32(s1);
      s2 = wave_sum32(s2);
      const float c1 = -(s1 * (1.0f / H)) * rstd, c2 = -(s2 * (1.0f / H)) * rstd;
#pragma unroll
      for (int R = 0; R < NR; ++R) out[R] = __builtin_fmaf(xh[R], c2, __builtin_fmaf(acc[R >> 4][R & 15], rstd, c1));
      {
#pragma clang fp contract(off)
        const float sd = 1.0f / rstd;
#pragma unroll
        for (int R = 0; R < NR; ++R) out[R] *= act_slope_from_value(xh[R] * sd + mean, ACT);
      }
      atl_store<H>(xo, slab, lane, out);
    } else if constexpr (!BWD) {
      uint32_t *mo = per_iteration(mask_out);
      float *ro = per_iteration(rstd_out);
      uint32_t bits[NW];
#pragma unroll
      for (int wd = 0; wd < NW; ++wd) bits[wd] = 0u;
      float v[NR];
      float sum = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        v[R] = relu_push(acc[R >> 4][R & 15], bits[R >> 5]);
        sum += v[R];
      }
      sum = wave_sum32(sum);
      const float mean = sum * (1.0f / H);
      float vs = 0.f;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        v[R] -= mean;
        vs += v[R] * v[R];
      }
      vs = wave_sum32(vs);
      const float rstd = 1.0f / sqrtf(vs * (1.0f / H) + 1e-5f);
#pragma unroll
      for (int R = 0; R < NR; ++R) v[R] *= rstd;
      atl_store<H>(xo, slab, lane, v);
#pragma unroll
      for (int wd = 0; wd < NW; ++wd) mo[(slab * NW + wd) * WAVE + lane] = bits[wd];
      if (lane < 32) ro[slab * SLAB + lane] = rstd;
    } else {
      float dx[NR], xh[NR], out[NR];
#pragma unroll
      for (int R = 0; R < NR; ++R) dx[R] = acc[R >> 4][R & 15];
      atl_load<H>(per_iteration(xprev), slab, lane, xh);
      ln_bwd_relu_regs<H>(dx, xh, per_iteration(mask_prev), per_iteration(rstd_prev)[slab * SLAB + i], lane, slab, out);
      atl_store<H>(xo, slab, lane, out);
    }
  }
}

template <int MT, int MODE>
void launch_rect(const float *xin, int KP, const float *Wp, int ldw, int kvalid, const float *bp, float *xout,
                 uint32_t *mask_out, float *rstd_out, const float *xprev, const uint32_t *mask_prev, const float *rstd_prev,
                 long n_slabs, hipStream_t s, const float *xin2 = nullptr, const float *W2 = nullptr, int ld2 = 0, int n_first = 0) {
  constexpr int NBUF = MT == 8 ? 2 : 1, WG_PER_CU = MT == 8 ? 1 : 2;
  const size_t shm = (size_t)NBUF * 3 * PANEL_FRAGS * sizeof(u32x4);
  allow_big_lds(k_panel_rect<MT, MODE>, shm);
  hipLaunchKernelGGL((k_panel_rect<MT, MODE>), dim3(persistent_grid(n_slabs, WG_PER_CU)), dim3(WG_THREADS), shm, s, xin, KP, Wp,
                     ldw, kvalid, bp, xout, mask_out, rstd_out, xprev, mask_prev, rstd_prev, n_slabs, xin2, W2, ld2, n_first);
}

// the ACT = 1..4 instantiations: the ReLU launch's geometry as it stands, mean in the place of the mask words (MODE 2: the second
// operand of launch_rect)
template <int MT, int MODE, int ACT>
void launch_rect_act(const float *xin, int KP, const float *Wp, int ldw, int kvalid, const float *bp, float *xout, float *mean_out,
                     float *rstd_out, const float *xprev, const float *mean_prev, const float *rstd_prev, long n_slabs, hipStream_t s,
                     const float *xin2 = nullptr, const float *W2 = nullptr, int ld2 = 0, int n_first = 0) {
  constexpr int NBUF = MT == 8 ? 2 : 1, WG_PER_CU = MT == 8 ? 1 : 2;
  const size_t shm = (size_t)NBUF * 3 * PANEL_FRAGS * sizeof(u32x4);
  allow_big_lds(k_panel_rect<MT, MODE, ACT>, shm);
  hipLaunchKernelGGL((k_panel_rect<MT, MODE, ACT>), dim3(persistent_grid(n_slabs, WG_PER_CU)), dim3(WG_THREADS), shm, s, xin, KP, Wp,
                     ldw, kvalid, bp, xout, (uint32_t *)nullptr, rstd_out, xprev, (const uint32_t *)nullptr, rstd_prev, n_slabs,
                     xin2, W2, ld2, n_first, mean_out, mean_prev);
}

// ... by run-time width and activation id (both checked by the caller)
template <int MODE, typename... Args>
void dispatch_rect_act(int H, int act, Args... a) {
#define RECT_ACT(MTv)                                            \
  switch (act) {                                                 \
    case 1: launch_rect_act<MTv, MODE, 1>(a...); break;          \
    case 2: launch_rect_act<MTv, MODE, 2>(a...); break;          \
    case 3: launch_rect_act<MTv, MODE, 3>(a...); break;          \
    default: launch_rect_act<MTv, MODE, 4>(a...); break;         \
  }
  if (H == 64) { RECT_ACT(2) } else if (H == 128) { RECT_ACT(4) } else { RECT_ACT(8) }
#undef RECT_ACT
}

bool width_ok(int h) { return h == 64 || h == 128 || h == 256; }

// ---- grouped heads on these trunks (opt-in HARL_CAT_WIDE_256=1): a Categorical head of 65..512 actions is G <= 4 groups of
// sp_g = 64 / 128 rows, each a folded pack [sp_g][K], a bias and an ATL(sp_g) image (csrc/cathead.hip).  The two kernels below
// walk ALL groups in one launch on the machinery above -- sub-panels, the 48 KiB panel, the register prefetch, one slab per wave.
// The table travels by value in the kernel arguments: every lookup in it is workgroup-uniform and a chain of scalar selects
// over constant indices (pick / the prefix compares), never an indexed read of a private copy.
constexpr int MAX_GROUPS = 4;
struct GroupTab {
  const float *W[MAX_GROUPS];  // folded pack [sp][ld], ld = the head input's width
  const float *b[MAX_GROUPS];  // forward: bias [sp]
  float *img[MAX_GROUPS];      // forward: the ATL(sp) logits image (out); backward: the ATL(sp) dz image (in)
  int sp[MAX_GROUPS];          // 64 / 128
  int first[MAX_GROUPS];       // backward: the group's first sub-panel in the K stream (prefix sum of sp / 32; unused: past the end)
  int n;
};

template <typename T>
__device__ __forceinline__ T pick(const T (&a)[MAX_GROUPS], int g) {
  T v = a[0];
#pragma unroll
  for (int k = 1; k < MAX_GROUPS; ++k)
    if (g == k) v = a[k];
  return v;
}

// forward: panel p (two full sub-panels = 64 columns) of ONE group's pack Wm = [rows][ld], as the 128-row panel of MT = 4.  A
// 64-row group has no rows 64..127: a thread's fragments 1 and 3 are those rows (dm = 64), so they are zeros as a whole and
// the pack is never read past its end.
__device__ __forceinline__ void load_panel_rows(float (&w)[PER_THREAD][8], const float *__restrict__ Wm, int ld, int rows, int p) {
  constexpr int MT = 4, SUB = MT * 128, NSUB = 8 / MT;
  const int r0 = threadIdx.x % SUB, ln = r0 & 63, j = (r0 >> 6) & 1, m0 = 32 * (r0 >> 7) + (ln & 31), kl = 16 * j + 4 * (ln >> 5);
  const unsigned voff = (unsigned)(m0 * ld + kl);  // (m0 < 64 <= rows)
#pragma unroll
  for (int u = 0; u < PER_THREAD; ++u) {
    const int sub = (u * WG_THREADS) / SUB, dm = 32 * (((u * WG_THREADS) % SUB) >> 7);  // (compile time: dm = 0 / 64)
    const bool in = dm < rows;  // (workgroup-uniform; the address stays inside the pack either way)
    const float *base = Wm + ((in ? dm : 0) * ld + 32 * (p * NSUB + sub));
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float v = base[feat_base(c) + voff];
      w[u][c] = in ? v : 0.f;
    }
  }
}

// z_g = W'_g x + b'_g for every group g, raw (no activation, no LayerNorm): the logits of a grouped head from the ATL(KP) head
// input, KP = 64 / 128 / 256.  k_panel_rect's forward at MT = 4 with the weight stream running over (group, K panel): nq =
// G KP / 64 panels through ONE prefetch pipeline, so the first panel of group g + 1 is on its way into registers while the
// last panel of group g multiplies and nothing drains at a group boundary.  There the wave stores its accumulators as they
// are and seeds them again from the next bias; the slab's x columns are read again per group (L2 hits, 32 KiB per wave).
// A 64-row group runs on the same four row tiles with zero weights past row 64 and stores the ATL(64) half (tiles 0 and 1): one
// instantiation, no second accumulator shape in the loop, at the price of idle MFMAs in the one group that can be 64 rows.
__global__ __launch_bounds__(WG_THREADS, 2) void k_rect_linear_groups(const float *__restrict__ xin, int KP, GroupTab tab, long n_slabs) {
  constexpr int MT = 4, NSUB = 8 / MT, SUB = MT * 128;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4 *img = reinterpret_cast<u32x4 *>(lds);
  const int lane = threadIdx.x & 63, wave = wave_id(), h = lane >> 5;
  const int ppg = KP / (32 * NSUB), nq = tab.n * ppg;  // panels per group, panels of the stream
  const long n_iter = (n_slabs + WAVES_PER_WG - 1) / WAVES_PER_WG;
  for (long it = blockIdx.x; it < n_iter; it += gridDim.x) {  // uniform trip count: barriers inside
    const long s_raw = it * WAVES_PER_WG + wave;
    const bool live = s_raw < n_slabs;
    const long slab = live ? s_raw : n_slabs - 1;
    const f32x4 *xp = reinterpret_cast<const f32x4 *>(xin + slab * (long)KP * SLAB) + lane;
    f32x16 acc[MT];
    auto seed = [&](int g) {
      const float *bg = pick(tab.b, g);
      const int sp = pick(tab.sp, g);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const bool in = 32 * t < sp;  // (a 64-row group has no bias past row 64: tiles 2 and 3 start from 0 and stay there)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = bg[(in ? 32 * t : 0) + (r & 3) + 8 * (r >> 2) + 4 * h];
          acc[t][r] = in ? v : 0.f;
        }
      }
    };
    seed(0);
    float w[PER_THREAD][8];
    load_panel_rows(w, tab.W[0], KP, tab.sp[0], 0);
    __syncthreads();  // the last panel of the iteration before is no longer being read
    commit_panel<MT>(img, w, NSUB);
    int g = 0, p = 0;
    for (int q = 0; q < nq; ++q) {
      float xa[16];
      load_cols<false>(xp, nullptr, 0, p * NSUB, xa);
      const bool more = q + 1 < nq, last = p + 1 == ppg;
      const int gn = last ? g + 1 : g, pn = last ? 0 : p + 1;
      if (more) load_panel_rows(w, pick(tab.W, gn), KP, pick(tab.sp, gn), pn);
      __syncthreads();  // panel q is complete
      const u32x4 *wl = img + lane;
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub) {
        u32x4 x1[2], x2[2], x3[2];
        split_acts<16>(xa, x1, x2, x3);
        float xb[16];
        if (sub + 1 < NSUB) load_cols<false>(xp, nullptr, 0, p * NSUB + sub + 1, xb);
        split_gemm<MT, 2>(wl + sub * 3 * SUB, x1, x2, x3, acc, [](int) {});
        if (sub + 1 < NSUB) {
#pragma unroll
          for (int c = 0; c < 16; ++c) xa[c] = xb[c];
        }
      }
      if (more) {
        __syncthreads();  // one buffer: every wave has drained panel q
        commit_panel<MT>(img, w, NSUB);
      }
      if (last) {  // group g is complete: its logits leave raw, the accumulators start over from the next bias
        if (live) {
          float *zg = pick(tab.img, g);
          if (pick(tab.sp, g) == 128) {
            float v[64];
#pragma unroll
            for (int R = 0; R < 64; ++R) v[R] = acc[R >> 4][R & 15];
            atl_store<128>(zg, slab, lane, v);
          } else {
            float v[32];
#pragma unroll
            for (int R = 0; R < 32; ++R) v[R] = acc[R >> 4][R & 15];
            atl_store<64>(zg, slab, lane, v);
          }
        }
        if (more) seed(gn);
      }
      g = gn;
      p = pn;
    }
  }
}

// ---- the tangent of the grouped logits (HATRPO's Fisher-vector product on these heads, opt-in HARL_TRPO_CAT_WIDE_256=1):
//   z_dot_g = W'_g_dot x_hat + b'_g_dot + W'_g x_dot      for every group g, raw, ONE ATL(sp_g) image per group
// k_rect_linear_groups crossed with the two-operand stream of k_panel_rect<MT, 2>.  The table of a group holds both matrices:
// operand 0 is (W'_g_dot, x_hat), operand 1 is (W'_g, x_dot).
struct TangentTab {
  const float *W[MAX_GROUPS];   // folded pack [sp][ld]
  const float *Wd[MAX_GROUPS];  // its tangent [sp][ld]
  const float *bd[MAX_GROUPS];  // the bias' tangent [sp]
  float *zd[MAX_GROUPS];        // the ATL(sp) tangent image (out)
  int sp[MAX_GROUPS];           // 64 / 128
  int n;
};

// The weight stream runs over (group, operand, K panel): nq = 2 G KP / 64 panels of 64 columns through the ONE register
// prefetch and the one 48 KiB buffer of the forward.  Nothing drains between the two operands of a group or between groups:
// while the last panel of (g, W') multiplies, the first panel of (g + 1, W'_dot) is in registers.  Which matrix a panel reads
// and which image the slab's columns come from are functions of the stream position alone, so workgroup-uniform: the matrix is
// a scalar select in front of load_panel_rows, the image a scalar select of the base in front of ONE lane address -- no second
// lane pointer lives across the loop.  Both operands add into the same accumulators, seeded from b'_g_dot; after operand 1 the
// wave stores them raw and seeds them from the next group's bias.  64-row groups and dead waves as in the forward.
__global__ __launch_bounds__(WG_THREADS, 2) void k_rect_tangent_groups(const float *__restrict__ xin, const float *__restrict__ xin_dot,
                                                                      int KP, TangentTab tab, long n_slabs) {
  constexpr int MT = 4, NSUB = 8 / MT, SUB = MT * 128;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4 *img = reinterpret_cast<u32x4 *>(lds);
  const int lane = threadIdx.x & 63, wave = wave_id(), h = lane >> 5;
  const int ppo = KP / (32 * NSUB), nq = tab.n * 2 * ppo;  // panels per operand, panels of the stream
  const long n_iter = (n_slabs + WAVES_PER_WG - 1) / WAVES_PER_WG;
  for (long it = blockIdx.x; it < n_iter; it += gridDim.x) {  // uniform trip count: barriers inside
    const long s_raw = it * WAVES_PER_WG + wave;
    const bool live = s_raw < n_slabs;
    const long slab = live ? s_raw : n_slabs - 1;
    const long xoff = slab * (long)KP * SLAB + 4 * lane;  // this lane's place in either image of the slab
    f32x16 acc[MT];
    auto seed = [&](int g) {
      const float *bg = pick(tab.bd, g);
      const int sp = pick(tab.sp, g);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const bool in = 32 * t < sp;  // (a 64-row group has no bias past row 64: tiles 2 and 3 start from 0 and stay there)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = bg[(in ? 32 * t : 0) + (r & 3) + 8 * (r >> 2) + 4 * h];
          acc[t][r] = in ? v : 0.f;
        }
      }
    };
    seed(0);
    float w[PER_THREAD][8];
    load_panel_rows(w, tab.Wd[0], KP, tab.sp[0], 0);
    __syncthreads();  // the last panel of the iteration before is no longer being read
    commit_panel<MT>(img, w, NSUB);
    int g = 0, o = 0, p = 0;
    for (int q = 0; q < nq; ++q) {
      const f32x4 *xp = reinterpret_cast<const f32x4 *>((o ? xin_dot : xin) + xoff);  // (workgroup-uniform base)
      float xa[16];
      load_cols<false>(xp, nullptr, 0, p * NSUB, xa);
      const bool more = q + 1 < nq, last = p + 1 == ppo, done = last && o == 1;
      const int pn = last ? 0 : p + 1, on = last ? o ^ 1 : o, gn = done ? g + 1 : g;
      if (more) load_panel_rows(w, on ? pick(tab.W, gn) : pick(tab.Wd, gn), KP, pick(tab.sp, gn), pn);
      __syncthreads();  // panel q is complete
      const u32x4 *wl = img + lane;
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub) {
        u32x4 x1[2], x2[2], x3[2];
        split_acts<16>(xa, x1, x2, x3);
        float xb[16];
        if (sub + 1 < NSUB) load_cols<false>(xp, nullptr, 0, p * NSUB + sub + 1, xb);
        split_gemm<MT, 2>(wl + sub * 3 * SUB, x1, x2, x3, acc, [](int) {});
        if (sub + 1 < NSUB) {
#pragma unroll
          for (int c = 0; c < 16; ++c) xa[c] = xb[c];
        }
      }
      if (more) {
        __syncthreads();  // one buffer: every wave has drained panel q
        commit_panel<MT>(img, w, NSUB);
      }
      if (done) {  // both operands of group g are in: its tangent leaves raw, the accumulators start over from the next bias
        if (live) {
          float *zg = pick(tab.zd, g);
          if (pick(tab.sp, g) == 128) {
            float v[64];
#pragma unroll
            for (int R = 0; R < 64; ++R) v[R] = acc[R >> 4][R & 15];
            atl_store<128>(zg, slab, lane, v);
          } else {
            float v[32];
#pragma unroll
            for (int R = 0; R < 32; ++R) v[R] = acc[R >> 4][R & 15];
            atl_store<64>(zg, slab, lane, v);
          }
        }
        if (more) seed(gn);
      }
      g = gn;
      o = on;
      p = pn;
    }
  }
}

// backward: where sub-panel s of the K stream lies -- the group whose prefix of sp / 32 sub-panels contains it (the tangent
// mode's n_first over a table) -- as that group's pack, dz image, image width and the sub-panel's place inside the group
struct GroupSub {
  const float *W, *img;
  int sp, s;
};
__device__ __forceinline__ GroupSub group_sub(const GroupTab &tab, int s) {
  GroupSub r{tab.W[0], tab.img[0], tab.sp[0], s};
#pragma unroll
  for (int k = 1; k < MAX_GROUPS; ++k)
    if (s >= tab.first[k]) r = GroupSub{tab.W[k], tab.img[k], tab.sp[k], s - tab.first[k]};  // (workgroup-uniform)
  return r;
}

// ... the fp32 weights of panel p of that stream, transposed: A[row][k] = W_g[k * ld + row], every k of a group valid
template <int MT>
__device__ __forceinline__ void load_panel_groups(float (&w)[PER_THREAD][8], const GroupTab &tab, int ld, int p, int nsub) {
  constexpr int SUB = MT * 128, NSUB = 8 / MT;
  const int r0 = threadIdx.x % SUB, ln = r0 & 63, j = (r0 >> 6) & 1, m0 = 32 * (r0 >> 7) + (ln & 31), kl = 16 * j + 4 * (ln >> 5);
  const unsigned voff = (unsigned)(kl * ld + m0);
#pragma unroll
  for (int u = 0; u < PER_THREAD; ++u) {
    const int sub = (u * WG_THREADS) / SUB, dm = 32 * (((u * WG_THREADS) % SUB) >> 7);
    if (sub < nsub) {  // (workgroup-uniform)
      const GroupSub gs = group_sub(tab, p * NSUB + sub);
#pragma unroll
      for (int c = 0; c < 8; ++c) w[u][c] = (gs.W + ((32 * gs.s + feat_base(c)) * ld + dm))[voff];
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) w[u][c] = 0.f;
    }
  }
}

__device__ __forceinline__ void load_cols_groups(const GroupTab &tab, long slab, int lane, int s, float (&x)[16]) {
  const GroupSub gs = group_sub(tab, s);
  load_cols<false>(reinterpret_cast<const f32x4 *>(gs.img + slab * (long)gs.sp * SLAB) + lane, nullptr, 0, gs.s, x);
}

// dz_prev = relu' . LNbwd(sum_g W'_g^T dz_g): the backward mode of k_panel_rect with its K stream running over the groups
// (n_sub = sum_g sp_g / 32 sub-panels, at most 16; a panel may hold sub-panels of two groups).  The sum over the groups is the
// GEMM's own K loop and the LayerNorm backward runs once, on the total.
template <int MT>
__global__ __launch_bounds__(WG_THREADS, MT == 8 ? 1 : 2) void k_rect_bwd_groups(
    GroupTab tab, int n_sub, float *__restrict__ xout, const float *__restrict__ xprev, const uint32_t *__restrict__ mask_prev,
    const float *__restrict__ rstd_prev, long n_slabs) {
  constexpr int H = 32 * MT, NSUB = 8 / MT, NBUF = MT == 8 ? 2 : 1, SUB = MT * 128, BUF = 3 * PANEL_FRAGS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  u32x4 *img = reinterpret_cast<u32x4 *>(lds);
  const int lane = threadIdx.x & 63, wave = wave_id(), i = lane & 31;
  const int n_panels = (n_sub + NSUB - 1) / NSUB;
  const long n_iter = (n_slabs + WAVES_PER_WG - 1) / WAVES_PER_WG;
  for (long it = blockIdx.x; it < n_iter; it += gridDim.x) {  // uniform trip count: barriers inside
    const long s_raw = it * WAVES_PER_WG + wave;
    const bool live = s_raw < n_slabs;
    const long slab = live ? s_raw : n_slabs - 1;
    f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float w[PER_THREAD][8];
    int nsub_p = n_sub < NSUB ? n_sub : NSUB;
    load_panel_groups<MT>(w, tab, H, 0, nsub_p);
    __syncthreads();  // the last panel of the iteration before is no longer being read
    commit_panel<MT>(img, w, nsub_p);
    for (int p = 0; p < n_panels; ++p) {
      float xa[16];
      load_cols_groups(tab, slab, lane, p * NSUB, xa);
      const bool more = p + 1 < n_panels;
      const int rest = n_sub - (p + 1) * NSUB, nsub_next = rest < NSUB ? rest : NSUB;
      if (more) load_panel_groups<MT>(w, tab, H, p + 1, nsub_next);
      __syncthreads();  // panel p is complete (and, with two buffers, panel p - 1 is no longer being read)
      const u32x4 *wl = img + (p % NBUF) * BUF + lane;
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
        if (sub < nsub_p) {
          u32x4 x1[2], x2[2], x3[2];
          split_acts<16>(xa, x1, x2, x3);
          float xb[16];
          if (sub + 1 < nsub_p) load_cols_groups(tab, slab, lane, p * NSUB + sub + 1, xb);
          split_gemm<MT, 2>(wl + sub * 3 * SUB, x1, x2, x3, acc, [](int) {});
          if (sub + 1 < nsub_p) {
#pragma unroll
            for (int c = 0; c < 16; ++c) xa[c] = xb[c];
          }
        }
      if (more) {
        if (NBUF == 1) __syncthreads();  // one buffer: every wave has drained panel p
        commit_panel<MT>(img + ((p + 1) % NBUF) * BUF, w, nsub_next);
      }
      nsub_p = nsub_next;
    }
    if (!live) continue;
    constexpr int NR = H / 2;
    float dx[NR], xh[NR], out[NR];
#pragma unroll
    for (int R = 0; R < NR; ++R) dx[R] = acc[R >> 4][R & 15];
    atl_load<H>(per_iteration(xprev), slab, lane, xh);
    ln_bwd_relu_regs<H>(dx, xh, per_iteration(mask_prev), per_iteration(rstd_prev)[slab * SLAB + i], lane, slab, out);
    atl_store<H>(per_iteration(xout), slab, lane, out);
  }
}

template <int MT>
void launch_bwd_groups(const GroupTab &tab, int n_sub, float *xout, const float *xprev, const uint32_t *mask_prev,
                       const float *rstd_prev, long n_slabs, hipStream_t s) {
  constexpr int NBUF = MT == 8 ? 2 : 1, WG_PER_CU = MT == 8 ? 1 : 2;
  const size_t shm = (size_t)NBUF * 3 * PANEL_FRAGS * sizeof(u32x4);
  allow_big_lds(k_rect_bwd_groups<MT>, shm);
  hipLaunchKernelGGL((k_rect_bwd_groups<MT>), dim3(persistent_grid(n_slabs, WG_PER_CU)), dim3(WG_THREADS), shm, s, tab, n_sub, xout,
                     xprev, mask_prev, rstd_prev, n_slabs);
}

// the host arrays of a grouped head as the kernels' table; false: not 1..4 groups of 64 / 128 rows.  Unused entries repeat
// group 0 and start past any stream, so the selects never take them.
bool group_tab(GroupTab &tab, int n_groups, const int *sp, const float *const *Wp, const float *const *bp, float *const *img) {
  if (n_groups < 1 || n_groups > MAX_GROUPS || !sp || !Wp || !img) return false;
  int first = 0;
  for (int g = 0; g < MAX_GROUPS; ++g) {
    const int k = g < n_groups ? g : 0;
    if (sp[k] != 64 && sp[k] != 128) return false;
    tab.W[g] = Wp[k];
    tab.b[g] = bp ? bp[k] : nullptr;
    tab.img[g] = img[k];
    tab.sp[g] = sp[k];
    tab.first[g] = g < n_groups ? first : 1 << 20;
    first += sp[k] / 32;
  }
  tab.n = n_groups;
  return true;
}
}  // namespace

extern "C" int harl_mlp_rect_fwd(const float *xin, long M, int KP, const float *Wp, int D, const float *bp, int HO, float *xout,
                                 uint32_t *relu_mask, float *rstd, void *stream) {
  if (M <= 0) return 0;
  if (!width_ok(HO)) return bad("harl_mlp_rect_fwd: output width must be 64, 128 or 256");
  if (D < 1 || KP % 32 != 0 || KP < D || KP > 512) return bad("harl_mlp_rect_fwd: KP must be a multiple of 32, >= D >= 1 and <= 512");
  const long n_slabs = n_slabs_of(M);
#define RECT(MTv) launch_rect<MTv, 0>(xin, KP, Wp, D, D, bp, xout, relu_mask, rstd, nullptr, nullptr, nullptr, n_slabs, (hipStream_t)stream)
  if (HO == 64) RECT(2); else if (HO == 128) RECT(4); else RECT(8);
#undef RECT
  return check_launch("harl_mlp_rect_fwd");
}

extern "C" int harl_mlp_rect_bwd(const float *dz, const float *xprev, const uint32_t *relu_mask_prev, const float *rstd_prev,
                                 long M, int HO, int HI, const float *Wp, float *dz_prev, void *stream) {
  if (M <= 0) return 0;
  if (!width_ok(HO) || !width_ok(HI)) return bad("harl_mlp_rect_bwd: both widths must be 64, 128 or 256");
  const long n_slabs = n_slabs_of(M);
  // dx_hat[i] = sum_o Wp[o][i] dz[o]: rows = input features, k = output features, Wp = [HO][HI] (row stride HI)
#define RECT(MTv) launch_rect<MTv, 1>(dz, HO, Wp, HI, HO, nullptr, dz_prev, nullptr, nullptr, xprev, relu_mask_prev, rstd_prev, n_slabs, (hipStream_t)stream)
  if (HI == 64) RECT(2); else if (HI == 128) RECT(4); else RECT(8);
#undef RECT
  return check_launch("harl_mlp_rect_bwd");
}

extern "C" int harl_mlp_rect_act_fwd(const float *xin, long M, int KP, const float *Wp, int D, const float *bp, int HO, int act,
                                     float *xout, float *mean, float *rstd, void *stream) {
  if (M <= 0) return 0;
  if (act < 1 || act > 4) return bad("harl_mlp_rect_act_fwd: activation id must be 1 (leaky_relu), 2 (tanh), 3 (sigmoid) or 4 (selu)");
  if (!width_ok(HO)) return bad("harl_mlp_rect_act_fwd: output width must be 64, 128 or 256");
  if (D < 1 || KP % 32 != 0 || KP < D || KP > 512) return bad("harl_mlp_rect_act_fwd: KP must be a multiple of 32, >= D >= 1 and <= 512");
  dispatch_rect_act<0>(HO, act, xin, KP, Wp, D, D, bp, xout, mean, rstd, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, n_slabs_of(M), (hipStream_t)stream);
  return check_launch("harl_mlp_rect_act_fwd");
}

extern "C" int harl_mlp_rect_act_bwd(const float *dz, const float *xprev, const float *mean_prev, const float *rstd_prev, long M,
                                     int HO, int HI, int act, const float *Wp, float *dz_prev, void *stream) {
  if (M <= 0) return 0;
  if (act < 1 || act > 4) return bad("harl_mlp_rect_act_bwd: activation id must be 1 (leaky_relu), 2 (tanh), 3 (sigmoid) or 4 (selu)");
  if (!width_ok(HO) || !width_ok(HI)) return bad("harl_mlp_rect_act_bwd: both widths must be 64, 128 or 256");
  // (rows = input features, k = output features, as in harl_mlp_rect_bwd)
  dispatch_rect_act<1>(HI, act, dz, HO, Wp, HI, HO, (const float *)nullptr, dz_prev, (float *)nullptr, (float *)nullptr, xprev,
                       mean_prev, rstd_prev, n_slabs_of(M), (hipStream_t)stream);
  return check_launch("harl_mlp_rect_act_bwd");
}

extern "C" int harl_mlp_rect_tangent(const float *xin_dot, const float *xin, long M, int KP, int HO, const float *Wp,
                                     const float *Wdp, int D, const float *bdp, const float *xprimal, const uint32_t *mask_in,
                                     const float *rstd_in, float *xout_dot, void *stream) {
  if (M <= 0) return 0;
  if (!width_ok(HO)) return bad("harl_mlp_rect_tangent: output width must be 64, 128 or 256");
  if (xin_dot) {
    if (!Wp || !width_ok(KP) || D != KP) return bad("harl_mlp_rect_tangent: a hidden layer (x_in_dot given) has KP = D = 64, 128 or 256 and needs W'");
  } else if (D < 1 || KP % 32 != 0 || KP < D || KP > 512 || HO == 256) {
    return bad("harl_mlp_rect_tangent: a first layer has KP a multiple of 32, >= D >= 1 and <= 512, and 64 or 128 outputs");
  }
  const long n_slabs = n_slabs_of(M);
  // the stream: (D + 31) / 32 sub-panels of W'_dot x_in, then KP / 32 of W' x_in_dot (both matrices [HO][D])
#define RECT(MTv) launch_rect<MTv, 2>(xin, KP, Wdp, D, D, bdp, xout_dot, nullptr, nullptr, xprimal, mask_in, rstd_in, n_slabs, (hipStream_t)stream, xin_dot, xin_dot ? Wp : nullptr, xin_dot ? KP : 0, (D + 31) / 32)
  if (HO == 64) RECT(2); else if (HO == 128) RECT(4); else RECT(8);
#undef RECT
  return check_launch("harl_mlp_rect_tangent");
}

extern "C" int harl_mlp_rect_act_tangent(const float *xin_dot, const float *xin, long M, int KP, int HO, const float *Wp,
                                         const float *Wdp, int D, const float *bdp, int act, const float *xprimal,
                                         const float *mean_in, const float *rstd_in, float *xout_dot, void *stream) {
  if (M <= 0) return 0;
  if (act < 1 || act > 4) return bad("harl_mlp_rect_act_tangent: activation id must be 1 (leaky_relu), 2 (tanh), 3 (sigmoid) or 4 (selu)");
  if (!width_ok(HO)) return bad("harl_mlp_rect_act_tangent: output width must be 64, 128 or 256");
  if (xin_dot) {
    if (!Wp || !width_ok(KP) || D != KP) return bad("harl_mlp_rect_act_tangent: a hidden layer (x_in_dot given) has KP = D = 64, 128 or 256 and needs W'");
  } else if (D < 1 || KP % 32 != 0 || KP < D || KP > 512) {
    return bad("harl_mlp_rect_act_tangent: a first layer has KP a multiple of 32, >= D >= 1 and <= 512");
  }
  // (harl_mlp_rect_tangent's stream: (D + 31) / 32 sub-panels of W'_dot x_in, then KP / 32 of W' x_in_dot)
  dispatch_rect_act<2>(HO, act, xin, KP, Wdp, D, D, bdp, xout_dot, (float *)nullptr, (float *)nullptr, xprimal, mean_in, rstd_in,
                       n_slabs_of(M), (hipStream_t)stream, xin_dot, xin_dot ? Wp : (const float *)nullptr, xin_dot ? KP : 0, (D + 31) / 32);
  return check_launch("harl_mlp_rect_act_tangent");
}

extern "C" int harl_mlp_rect_linear_groups(const float *xin, long M, int KP, int n_groups, const int *sp, const float *const *Wp,
                                           const float *const *bp, float *const *z, void *stream) {
  if (M <= 0) return 0;
  GroupTab tab;
  if (!width_ok(KP) || !bp || !group_tab(tab, n_groups, sp, Wp, bp, z))
    return bad("harl_mlp_rect_linear_groups: 1..4 groups of 64 / 128 rows on a head input of 64, 128 or 256 columns");
  const long n_slabs = n_slabs_of(M);
  const size_t shm = (size_t)3 * PANEL_FRAGS * sizeof(u32x4);
  allow_big_lds(k_rect_linear_groups, shm);
  hipLaunchKernelGGL(k_rect_linear_groups, dim3(persistent_grid(n_slabs, 2)), dim3(WG_THREADS), shm, (hipStream_t)stream, xin, KP, tab,
                     n_slabs);
  return check_launch("harl_mlp_rect_linear_groups");
}

extern "C" int harl_mlp_rect_tangent_groups(const float *xin_dot, const float *xin, long M, int KP, int n_groups, const int *sp,
                                            const float *const *Wp, const float *const *Wdp, const float *const *bdp,
                                            float *const *zd, void *stream) {
  if (M <= 0) return 0;
  bool ok = xin_dot && xin && width_ok(KP) && n_groups >= 1 && n_groups <= MAX_GROUPS && sp && Wp && Wdp && bdp && zd;
  for (int g = 0; ok && g < n_groups; ++g) ok = (sp[g] == 64 || sp[g] == 128) && Wp[g] && Wdp[g] && bdp[g] && zd[g];
  if (!ok)
    return bad("harl_mlp_rect_tangent_groups: 1..4 groups of 64 / 128 rows on a head input of 64, 128 or 256 columns, every pointer given");
  TangentTab tab;
  for (int g = 0; g < MAX_GROUPS; ++g) {  // (unused entries repeat group 0: the stream never reaches them)
    const int k = g < n_groups ? g : 0;
    tab.W[g] = Wp[k];
    tab.Wd[g] = Wdp[k];
    tab.bd[g] = bdp[k];
    tab.zd[g] = zd[k];
    tab.sp[g] = sp[k];
  }
  tab.n = n_groups;
  const long n_slabs = n_slabs_of(M);
  const size_t shm = (size_t)3 * PANEL_FRAGS * sizeof(u32x4);
  allow_big_lds(k_rect_tangent_groups, shm);
  hipLaunchKernelGGL(k_rect_tangent_groups, dim3(persistent_grid(n_slabs, 2)), dim3(WG_THREADS), shm, (hipStream_t)stream, xin, xin_dot,
                     KP, tab, n_slabs);
  return check_launch("harl_mlp_rect_tangent_groups");
}

extern "C" int harl_mlp_rect_bwd_groups(const float *const *dz, int n_groups, const int *sp, const float *const *Wp,
                                        const float *xprev, const uint32_t *relu_mask_prev, const float *rstd_prev, long M, int HI,
                                        float *dz_prev, void *stream) {
  if (M <= 0) return 0;
  GroupTab tab;
  if (!width_ok(HI) || !group_tab(tab, n_groups, sp, Wp, nullptr, const_cast<float *const *>(dz)))
    return bad("harl_mlp_rect_bwd_groups: 1..4 groups of 64 / 128 rows into a head input of 64, 128 or 256 columns");
  int n_sub = 0;
  for (int g = 0; g < n_groups; ++g) n_sub += sp[g] / 32;
  const long n_slabs = n_slabs_of(M);
#define RECT(MTv) launch_bwd_groups<MTv>(tab, n_sub, dz_prev, xprev, relu_mask_prev, rstd_prev, n_slabs, (hipStream_t)stream)
  if (HI == 64) RECT(2); else if (HI == 128) RECT(4); else RECT(8);
#undef RECT
  return check_launch("harl_mlp_rect_bwd_groups");
}
