// bwd_fused.h -- the fused hidden-layer backward: k_bwd_dx_dw (four waves), k_bwd_dx_dw8 (eight waves, the default) and what the
// two share.  Part of mlp.hip's translation unit, included there below tr_read and the weight-gradient kernels: not stand-alone.
#pragma once

// =============================================================================================
// k_bwd_dx_dw: the WHOLE backward of one hidden Linear(128 -> 128) and the relu + LayerNorm in front of it in ONE persistent
// launch (round 5): dz_prev = LNrelu'(Wp^T dz), dW' += dz^T x_hat_prev, db' += sum dz, and -- first-layer variant, KT = 1 --
// dW_1' += dz_1^T x0n.  It replaces the pair harl_mlp_dw_partials(dz, x_hat_prev) + harl_mlp_bwd_dx(...), which streamed the same
// two operands (dz 512 B + x_hat_prev 512 B per sample) from HBM one after the other: half of the MPE step's time and 17 of its
// 58 GB.  Matches autograd through MLPLayer (harl/models/base/mlp.py:25-38, happo.py:93-100).
//
// One workgroup per CU, four waves, 144 KiB of LDS: the three split images of Wp^T (96 KiB, as k_bwd_dx) and TWO transposition
// buffers for x_hat_prev^T (k_dw_tr's image, 24 KiB each).  A super-round = four slabs, one per wave:
//   O part (the owner's slab, k_bwd_dx's body): dz already split (below) -> 192 MFMAs -> LayerNorm/ReLU backward -> dz_prev
//     (stored, KT = 0) or the first-layer weight gradient on the matrix-pipe transposes (KT = 1, mfma_transpose.h);
//   D part, four rounds, one per slab of the super-round: wave w owns row tile w of dW' (output features 32 w .. 32 w + 31).
//     Its A operand -- that 32-feature block of the slab's dz, transposed -- it makes itself on the matrix pipe (its four float4
//     pieces of the block, split exactly, times the permuted identity: 6 MFMAs, no LDS, and the transposition's row sums are
//     db'); the B operand x_hat_prev^T is shared: every wave splits a quarter of the slab's pieces and stores them into the
//     round's buffer, the fragments come back through ds_read_b64_tr_b16.  Both are fetched a second time microseconds after
//     their owners touched them -- which, measured (rocprofv3 --pmc FETCH_SIZE, profiles/r05_hbm_traffic.md), does NOT stay in the
//     L2: 1.56 GB leave it per launch against 0.96 GB of operands (a super-round's working set per XCD, 32 workgroups x 4 slabs x
//     32 KB, is the L2's 4 MB); the pair of layer kernels fetched 1.83 GB.
// Version 1 of this kernel (one buffer, both operands through LDS, two barriers per round) measured no faster than the pair it
// replaces: with one workgroup per CU nothing overlaps a barrier wait (profiles/r05_bwd_fused_ab.md).  Hence the software
// pipeline: everything round n+1 needs is prepared DURING round n's 48 product MFMAs -- a wave has one MFMA in flight for 32
// cycles but needs ~12 of issue for it, and up to five VALU instructions placed BETWEEN two MFMAs are free
// (profiles/r03_mfma_valu_overlap.md) -- as filler chunks of 5-8 VALU pinned behind each MFMA with sched_barrier (source order
// is honoured exactly): the split of the next A block (16 chunks), its 6 transposing MFMAs, the packing of their results and the
// split of the next B pieces (16 chunks).  The split of the OWNER's slab of dz (64 chunks: the 2.2k cycles k_bwd_dx spends in
// "split dz") rides behind the product MFMAs of its own dX GEMM, one k-step ahead of its use (those 192 shadows were empty).
// The B terms are stored at the END of round n into the buffer round n-1 read, so ONE barrier per round suffices (every wave
// has left round n-1 when any wave stores for n+1), and it finds the stores long complete.  FILL = false runs the same chunks
// as a block in front of the product MFMAs (A/B).
// Per-workgroup partial rows in the layout of harl_reduce_partials_multi: dW' by tiles straight from the accumulators (the
// waves own disjoint row tiles), dW_1' through finish_partials; rows gridDim.x .. n_part_rows-1 of both arenas are cleared.
//
// The two kernels share the gradient rounds (GradRounds), the owner's chunked split, operand requests and LayerNorm backward
// (owner_*), the first-layer gradient (Dw1Acc) and the epilogue.  What differs stays in the kernel bodies: which wave plays which
// part, when the owner requests and holds its dz and operands, where it meets the rounds' barriers, and Sched4 / Sched8.
// =============================================================================================
__device__ __forceinline__ unsigned split_stage1(float f0, float f1, float &r0, float &r1) {
  const unsigned b0 = __float_as_uint(f0), b1 = __float_as_uint(f1);
  r0 = f0 - __uint_as_float(b0 & 0xffff0000u);
  r1 = f1 - __uint_as_float(b1 & 0xffff0000u);
  return __builtin_amdgcn_perm(b1, b0, 0x07060302u);
}
__device__ __forceinline__ void split_stage2(float r0, float r1, unsigned &p2, unsigned &p3) {
  const unsigned c0 = __float_as_uint(r0), c1 = __float_as_uint(r1);
  p2 = __builtin_amdgcn_perm(c1, c0, 0x07060302u);
  const float q0 = r0 - __uint_as_float(c0 & 0xffff0000u), q1 = r1 - __uint_as_float(c1 & 0xffff0000u);
  p3 = __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u);
}

// compile-time loop: f(std::integral_constant<int, I>) for I = I0 .. N-1 -- every index inside is a constant expression, whatever
// the unroller thinks of the body's size (a `#pragma unroll` loop that stays rolled turns register arrays into scratch)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

constexpr int BDW_H = 128, BDW_MT = 4, BDW_NJ = 8, BDW_NR = 64, BDW_KPF = 32;  // the layer, its GEMM tiling, first-layer k (padded)
constexpr int BDW_SQ = (128 / 16) * 128 + 8, BDW_IMG = 8 * BDW_SQ;  // k_dw_tr's image geometry at H = 128
constexpr int BDW_BUF = 3 * BDW_IMG;                                // one transposition buffer: three term images
constexpr size_t bdw_lds_bytes() { return split_image_bytes(128, 128) + (size_t)2 * BDW_BUF; }

// accumulator tiles (and the per-lane bias sums that go with them) cleared
template <int N>
__device__ __forceinline__ void zero_acc(f32x16 (&a)[N], float *db = nullptr) {
#pragma unroll
  for (int t = 0; t < N; ++t) {
    if (db) db[t] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) a[t][r] = 0.f;
  }
}

// The D part of one wave: row tile `wave` of dW' | db' over the slabs of the workgroup's super-rounds.
//   Sched::LOAD_R0 / LOAD_RN: the slot (product MFMA) behind which the round after next's pieces are requested, round 0 / 1, 2;
//   extra(rc, sc): further filler work of the caller's behind slots 32..47 of rounds 1..3 (free of this part's chunks);
//   phase(std::integral_constant<int, n>): the caller's PHASE(n) (the timers live in the kernel body).
// The members are registers: the constructor leaves the arrays uninitialised (a value-initialising G{...} costs 16 v_mov).
struct GradRounds {
  static constexpr int H = BDW_H;
  const float *const dz, *const xprev;
  const long n_slabs;
  unsigned char *const Bb;  // [2][3 terms][BDW_IMG]: x_hat_prev^T staging
  const int lane, wave, i, h;
  const Ident ident;
  f32x16 acc2[4];  // dW' tiles (row tile = wave, column tiles 0..3)
  float db2;       // db' of feature 32 wave + (lane & 31): this lane half's 16 samples of every slab
  // prA: the four float4 pieces 4 wave + u of a slab's dz = registers 16 wave .. 16 wave + 15 of the accumulator layout = the
  // 32-feature block `wave`; prB: pieces 4 wave + u of x_hat_prev (this wave's quarter of the B operand)
  f32x4 prA[4], prB[4];
  u32x2_t spB[4][3];          // split terms of prB: one ds_write_b64 each
  u32x4 ya[3][2];             // split terms of prA by k-step (split_transpose_block's y1 / y2 / y3)
  f32x16 tc[3];               // the three transposed terms (lane = feature, 16 samples)
  u32x4 At[3][2], AtN[3][2];  // A operands [term][k-step] of this round / of the next one
  float rr0, rr1;             // remainders between the two stages of a pair's split
  // Preparing a round that will not be executed (past the last slab) is harmless -- its operands are never multiplied -- except
  // for the bias sums of its A block: `vnext` (1 or 0) multiplies them.  The loads of such a round are clamped to a valid slab.
  float vnext;
  const int frag_lane;  // read_frag's lane offset

  __device__ __forceinline__ GradRounds(const float *dz_, const float *xprev_, long n_slabs_, unsigned char *Bb_, int lane_,
                                        int wave_, const Ident &ident_)
      : dz(dz_), xprev(xprev_), n_slabs(n_slabs_), Bb(Bb_), lane(lane_), wave(wave_), i(lane_ & 31), h(lane_ >> 5),
        ident(ident_), db2(0.f), rr0(0.f), rr1(0.f), vnext(1.f),
        frag_lane(((lane_ >> 4) & 1) * 128 + ((lane_ & 15) >> 2) * 32 + (lane_ & 3) * 8) {}

  __device__ __forceinline__ void d_load(long ds) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      prA[u] = (reinterpret_cast<const f32x4 *>(dz + ds * (long)(H * SLAB)) + lane)[(4 * wave + u) * WAVE];
      prB[u] = (reinterpret_cast<const f32x4 *>(xprev + ds * (long)(H * SLAB)) + lane)[(4 * wave + u) * WAVE];
    }
  }
  __device__ __forceinline__ void d_load_next(long ds, long fallback) { d_load(ds < n_slabs ? ds : fallback); }
  // A chunk k (0..15): pair p = k >> 1 = registers 2p, 2p + 1 of the block -> word p & 3 of k-step p >> 2; stage k & 1
  __device__ __forceinline__ void a_chunk(int k) {
    const int pi = k >> 1, j = pi >> 2, c = pi & 3, u = pi >> 1, e = 2 * (pi & 1);
    if ((k & 1) == 0) {
      ya[0][j][c] = split_stage1(prA[u][e], prA[u][e + 1], rr0, rr1);
    } else {
      unsigned p2, p3;
      split_stage2(rr0, rr1, p2, p3);
      ya[1][j][c] = p2;
      ya[2][j][c] = p3;
    }
  }
  // B chunk k (0..15): piece k >> 2, pair (k >> 1) & 1, stage k & 1
  __device__ __forceinline__ void b_chunk(int k) {
    const int u = k >> 2, c2 = (k >> 1) & 1;
    if ((k & 1) == 0) {
      spB[u][0][c2] = split_stage1(prB[u][2 * c2], prB[u][2 * c2 + 1], rr0, rr1);
    } else {
      unsigned p2, p3;
      split_stage2(rr0, rr1, p2, p3);
      spB[u][1][c2] = p2;
      spB[u][2][c2] = p3;
    }
  }
  // transposing MFMA k (0..5) of the A block: term k % 3, k-step k / 3 (mfma_transpose.h, transpose_block)
  __device__ __forceinline__ void t_mfma(int k) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int t = k % 3;
    if (k < 3) tc[t] = mfma_bf16(ya[t][0], ident.j0, zero);
    else tc[t] = mfma_bf16(ya[t][1], ident.j1, tc[t]);
  }
  // pack chunk k (0..5): k < 3: term k -> the two k-step operands; k >= 3: its row sums into db'
  __device__ __forceinline__ void p_chunk(int k) {
    if (k < 3) {
      pack_transposed(tc[k], AtN[k][0], AtN[k][1]);
    } else {
      f32x2 a = {0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 8; ++r) a += f32x2{tc[k - 3][2 * r], tc[k - 3][2 * r + 1]};
      db2 += vnext * (a[0] + a[1]);
    }
  }
  __device__ __forceinline__ void b_store(int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = 4 * wave + u;
      unsigned char *d = Bb + buf * BDW_BUF + (i >> 2) * BDW_SQ + (2 * (q >> 2) + ((q & 3) >> 1)) * 128 + (i & 3) * 32 +
                         (8 * (q & 1) + 4 * h) * 2;
#pragma unroll
      for (int term = 0; term < 3; ++term) *reinterpret_cast<u32x2_t *>(d + term * BDW_IMG) = spB[u][term];
    }
  }
  // B fragment of column tile `tile`, k-step ks: the eight samples sigma(r, h) = (r & 3) + 8 (r >> 2) + 4 h + 16 ks, r = 0..7 --
  // the order the matrix-pipe transposition leaves the A operand in (mfma_transpose.h): sample quads 4 ks + h and 4 ks + 2 + h
  __device__ __forceinline__ void read_frag(int buf, int ks, int tile, u32x4 (&f)[3]) {
#pragma unroll
    for (int term = 0; term < 3; ++term) {
      const unsigned char *fp = Bb + buf * BDW_BUF + term * BDW_IMG + (4 * ks + h) * BDW_SQ + 2 * tile * 128 + frag_lane;
      const u32x2_t lo = tr_read(fp), hi = tr_read(fp + 2 * BDW_SQ);
      f[term] = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
  }
  // the prepared round's A operands become current
  __device__ __forceinline__ void a_advance() {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      At[t][0] = AtN[t][0];
      At[t][1] = AtN[t][1];
    }
  }

  // the first round of the first super-round, prepared in the open
  __device__ __forceinline__ void prologue(long base0) {
    d_load(base0);
#pragma unroll
    for (int k = 0; k < 16; ++k) a_chunk(k);
#pragma unroll
    for (int k = 0; k < 6; ++k) t_mfma(k);
#pragma unroll
    for (int k = 0; k < 16; ++k) b_chunk(k);
#pragma unroll
    for (int k = 0; k < 6; ++k) p_chunk(k);
    a_advance();
    b_store(0);
  }

  // round r (0..3) of the super-round at `base`: the slab base + r
  template <int r, bool FILL, class Sched, class Extra, class Phase>
  __device__ __forceinline__ void round(long base, long sr_stride, Extra &&extra, Phase &&phase) {
    __syncthreads();  // every wave's B terms of this round are in buffer r & 1; buffer (r + 1) & 1 is free
    phase(std::integral_constant<int, 5>{});
    // the round being prepared (r + 1, or round 0 of the next super-round) and the one whose pieces are requested (r + 2; none
    // from round 3: the next super-round fetches its round 1 itself)
    const long ds1 = r < 3 ? base + r + 1 : base + sr_stride;
    const long ds2 = r < 2 ? base + r + 2 : base + sr_stride;
    vnext = uniform_f(ds1 < n_slabs ? 1.f : 0.f);
    // TSLOT: the product MFMA behind which the six transposing MFMAs are issued
    constexpr int TSLOT = r == 0 ? 31 : 15;
    auto slot = [&](auto sc) {  // filler work behind product MFMA s (0..47)
      constexpr int s_ = decltype(sc)::value;
      if constexpr (r == 0) {  // the pieces of round 1 were requested just before the super-round: nothing in the first 16 slots
        if constexpr (s_ >= 16 && s_ < 32) a_chunk(s_ - 16);
        else if constexpr (s_ >= 32 && s_ < 42) b_chunk(s_ - 32 + 6);
        else if constexpr (s_ >= 42) p_chunk(s_ - 42);
        if constexpr (s_ == Sched::LOAD_R0) d_load_next(ds2, base);
      } else {
        if constexpr (s_ < 16) a_chunk(s_);
        else if constexpr (s_ < 26) b_chunk(s_ - 16 + 6);
        else if constexpr (s_ < 32) p_chunk(s_ - 26);
        else extra(std::integral_constant<int, r>{}, sc);
        if constexpr (s_ == Sched::LOAD_RN && r < 3) d_load_next(ds2, base);
      }
      if constexpr (s_ == TSLOT) {  // the six transposing MFMAs, each with one of the first six B chunks behind it
        static_for<0, 6>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          __builtin_amdgcn_sched_barrier(0);
          t_mfma(k);
          b_chunk(k);
        });
      }
    };
    u32x4 bv[2][3];
    read_frag(r & 1, 0, 0, bv[0]);
    if constexpr (!FILL) static_for<0, 48>(slot);
    // ---- 2 k-steps x 4 column tiles x the six cross products; B fragments one tile-step ahead
    static_for<0, 8>([&](auto nc) {
      constexpr int n = decltype(nc)::value, ks = n >> 2, b = n & 3;
      if constexpr (n + 1 < 8) read_frag(r & 1, (n + 1) >> 2, (n + 1) & 3, bv[(n + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      constexpr int AT[6] = {2, 0, 1, 1, 0, 0}, BT[6] = {0, 2, 1, 0, 1, 0};  // the six cross products, smallest first
      static_for<0, 6>([&](auto kc) {
        constexpr int k6 = decltype(kc)::value;
        acc2[b] = mfma_bf16(At[AT[k6]][ks], bv[n & 1][BT[k6]], acc2[b]);
        if constexpr (FILL) slot(std::integral_constant<int, 6 * n + k6>{});
        __builtin_amdgcn_sched_barrier(0);
      });
    });
    phase(std::integral_constant<int, 6>{});
    // the next round's B terms into the buffer the PREVIOUS round read (every wave has passed this round's barrier, i.e.
    // left the previous round); its A operands become current
    b_store((r + 1) & 1);
    a_advance();
    phase(std::integral_constant<int, 7>{});
  }

  // the super-round at `base` (round 0's operands: from the previous one's last round / the prologue; round 1's pieces: the caller)
  template <bool FILL, class Sched, class Extra, class Phase>
  __device__ __forceinline__ void rounds(long base, long sr_stride, Extra &&extra, Phase &&phase) {
    static_for<0, 4>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      if (base + r < n_slabs) round<r, FILL, Sched>(base, sr_stride, extra, phase);  // workgroup-uniform
    });
  }

  // this workgroup's partial row of dW' | db' straight from the accumulators (the waves own disjoint tiles)
  __device__ __forceinline__ void store_row(float *dw2_part) {
    float *mypart = dw2_part + (long)blockIdx.x * ((long)H * H + H);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
        mypart[(long)o * H + 32 * b + i] = acc2[b][r];
      }
    const float dbt = wave_sum32(db2);
    if (h == 0) mypart[(long)H * H + 32 * wave + i] = dbt;
  }
};

// rows gridDim.x .. n_part_rows-1 of the dW' | db' arena cleared, by the whole workgroup of NTH threads
template <int NTH>
__device__ __forceinline__ void clear_dw2_rows(float *dw2_part, int n_part_rows) {
  constexpr long ROW2 = (long)BDW_H * BDW_H + BDW_H;
  for (int row = blockIdx.x + gridDim.x; row < n_part_rows; row += gridDim.x) {
    float *z = dw2_part + (long)row * ROW2;
    for (int e = threadIdx.x; e < ROW2; e += NTH) z[e] = 0.f;
  }
}

// The O part's pieces.  Each kernel decides WHEN it requests the operands and how it holds the slab's raw dz.
// O chunk k (0..63) of a slab's split into the B operands of the dX GEMM: pair k>>1 (registers 2p, 2p+1 -> word p&3 of k-step
// p>>2), stage k&1; q0 / q1 carry the remainders from a pair's first stage to its second
__device__ __forceinline__ void owner_split_chunk(int k, const float (&raw)[BDW_NR], u32x4 (&g1)[BDW_NJ], u32x4 (&g2)[BDW_NJ],
                                                  u32x4 (&g3)[BDW_NJ], float &q0, float &q1) {
  const int pi = k >> 1, j = pi >> 2, c = pi & 3;
  if ((k & 1) == 0) {
    g1[j][c] = split_stage1(raw[2 * pi], raw[2 * pi + 1], q0, q1);
  } else {
    unsigned p2, p3;
    split_stage2(q0, q1, p2, p3);
    g2[j][c] = p2;
    g3[j][c] = p3;
  }
}
// requests: the LayerNorm / ReLU backward's operands of `slab`; its x0n block (KT = 1)
__device__ __forceinline__ void owner_ln_operands(const float *xprev, const float *rstd_prev, const uint32_t *mask_prev, long slab,
                                                  int lane, float (&xh)[BDW_NR], float &rstd, uint32_t (&mbits)[2]) {
  atl_load<BDW_H>(xprev, slab, lane, xh);
  rstd = rstd_prev[slab * SLAB + (lane & 31)];
#pragma unroll
  for (int w = 0; w < 2; ++w) mbits[w] = mask_prev[(slab * 2 + w) * WAVE + lane];
}
__device__ __forceinline__ void owner_x0_operands(const float *x0n, long slab, int lane, f32x4 (&x0r)[BDW_KPF / 8]) {
  const f32x4 *bp = reinterpret_cast<const f32x4 *>(x0n + slab * (long)(BDW_KPF * SLAB)) + lane;
#pragma unroll
  for (int q = 0; q < BDW_KPF / 8; ++q) x0r[q] = bp[q * WAVE];
}
// the dX GEMM's accumulators -> LayerNorm / ReLU backward -> out = the slab's dz_prev, stored if wanted
__device__ __forceinline__ void owner_ln_bwd(const f32x16 (&acc)[BDW_MT], const float (&xh)[BDW_NR], const uint32_t (&mbits)[2],
                                             float rstd, float *dz_prev, long slab, int lane, float (&out)[BDW_NR]) {
  float dx[BDW_NR];
#pragma unroll
  for (int R = 0; R < BDW_NR; ++R) dx[R] = acc[R >> 4][R & 15];
  ln_bwd_relu_mbits<BDW_H>(dx, xh, mbits, rstd, out);
  if (dz_prev) atl_store<BDW_H>(dz_prev, slab, lane, out);
}
// the first-layer gradient of an owner wave (KT = 1): dW_1' tiles and db_1' (per-lane sums over the lane's samples)
struct Dw1Acc {
  f32x16 acc1[4];
  float dbs[4];
  __device__ __forceinline__ void zero() { zero_acc(acc1, dbs); }
  // one slab: dW_1' += out^T x0n, db_1' += sum out, both transposed on the matrix pipe
  __device__ __forceinline__ void add(const f32x4 (&x0r)[BDW_KPF / 8], const float (&out)[BDW_NR], const Ident &ident) {
    float xr0[BDW_KPF / 2];
#pragma unroll
    for (int q = 0; q < BDW_KPF / 8; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) xr0[4 * q + e] = x0r[q][e];
    u32x4 a1[BDW_KPF / 16], a2[BDW_KPF / 16], a3[BDW_KPF / 16];
    split_acts<BDW_KPF / 2>(xr0, a1, a2, a3);
    u32x4 Bt[3][2];
    transpose_block<false>(a1[0], a1[1], a2[0], a2[1], a3[0], a3[1], ident, Bt);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      u32x4 A1[3][2];
      dbs[a] += split_transpose_block<true>(&out[16 * a], ident, A1);
      dw_tile(acc1[a], A1, Bt);
    }
  }
  // the workgroup's partial row of dW_1' | db_1' (and the arena's unused rows cleared) through the LDS at `buf`
  template <int NTH>
  __device__ __forceinline__ void finish(float *buf, float *dw1_part, int n_part_rows) {
    f32x16 a1x[4][1];
#pragma unroll
    for (int a = 0; a < 4; ++a) a1x[a][0] = acc1[a];
    finish_partials<4, 1, NTH>(a1x, dbs, buf, dw1_part, n_part_rows);
  }
};

// k_bwd_dx_dw: four waves, each the owner of slab base + wave AND the gradient wave of row tile `wave` (-DHARL_BWD_SPLIT_WAVES=0;
// the bit-exact oracle of tests/test_gpu_bwd_split_waves.py).  The owner's operands are requested before its GEMM, the next
// slab's raw dz before the rounds; k-step 0 of that slab's split rides in the last round's free slots.
struct Sched4 { static constexpr int LOAD_R0 = 41, LOAD_RN = 25; };  // beside the packing
template <int KT, bool FILL>
__global__ __launch_bounds__(WG_THREADS, 1) void k_bwd_dx_dw(
    const float *__restrict__ dz, const float *__restrict__ xprev, const uint32_t *__restrict__ mask_prev,
    const float *__restrict__ rstd_prev, const float *__restrict__ Wp, float *__restrict__ dz_prev, long n_slabs,
    const float *__restrict__ x0n, float *__restrict__ dw1_part, float *__restrict__ dw2_part, int n_part_rows) {
  constexpr int H = BDW_H, MT = BDW_MT, NJ = BDW_NJ, NR = BDW_NR, KPF = BDW_KPF;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  PHASE_BEGIN();
  auto ph = [&](auto pc) { PHASE(decltype(pc)::value); };
  u32x4 *img = reinterpret_cast<u32x4 *>(lds);
  stage_split_matrix<H, H, true, WG_THREADS>(img, Wp);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = wave_id();
  const u32x4 *wl = img + lane;
  const long sr_stride = (long)gridDim.x * WAVES_PER_WG;
  const long base0 = (long)blockIdx.x * WAVES_PER_WG;
  const Ident ident = make_ident(lane);

  // ---- persistent accumulators: dW' | db' in G; dW_1' tiles and db_1' (per-lane sums over the lane's samples), KT = 1
  GradRounds G(dz, xprev, n_slabs, reinterpret_cast<unsigned char *>(img + 3 * MT * NJ * 64), lane, wave, ident);
  Dw1Acc A1;
  zero_acc(G.acc2);
  if constexpr (KT > 0) A1.zero();

  // ---- owner state: the current slab's dz split into the B operands of the GEMM, the next slab's raw dz
  float raw[NR];
  u32x4 g1[NJ], g2[NJ], g3[NJ];
  float ro0 = 0.f, ro1 = 0.f;
  auto o_chunk = [&](int k) { owner_split_chunk(k, raw, g1, g2, g3, ro0, ro1); };
  atl_load<H>(dz, base0 + wave < n_slabs ? base0 + wave : 0, lane, raw);
  // k-step 0 of the first slab (later slabs: the last weight-gradient round's slots 32..39)
#pragma unroll
  for (int k = 0; k < 8; ++k) o_chunk(k);
  if (base0 < n_slabs) G.prologue(base0);
  PHASE(10);

  for (long base = base0; base < n_slabs; base += sr_stride) {
    const long slab = base + wave;
    const bool own = slab < n_slabs;
    const long nxt = slab + sr_stride < n_slabs ? slab + sr_stride : (own ? slab : 0);
    // =========================== O part: this wave's own slab ===========================
    if (own) {
      float xh[NR], rstd;
      uint32_t mbits[2];
      owner_ln_operands(xprev, rstd_prev, mask_prev, slab, lane, xh, rstd, mbits);
      f32x4 x0r[KT > 0 ? KPF / 8 : 1];
      if constexpr (KT > 0) owner_x0_operands(x0n, slab, lane, x0r);
      f32x16 acc[MT];
      zero_acc(acc);
      PHASE(0);
      // the split of k-step j + 1 of THIS slab's dz (raw) behind the 24 product MFMAs of k-step j: one chunk (one stage of
      // a pair: ~5.5 VALU) behind every third MFMA
      split_gemm_fill<MT, NJ>(wl, g1, g2, g3, acc, [&](int s_, int k6) {
        const int j1 = s_ / MT + 1, q = (s_ % MT) * 6 + k6;  // q = 0..23: the MFMA's position inside k-step j
        if (j1 < NJ && q % 3 == 0) o_chunk(8 * j1 + q / 3);
      });
      PHASE(1);
      float out[NR];
      owner_ln_bwd(acc, xh, mbits, rstd, dz_prev, slab, lane, out);
      PHASE(2);
      if constexpr (KT > 0) {
        A1.add(x0r, out, ident);
        PHASE(3);
      }
    }
    // =========================== D part: the four slabs of this super-round ===========================
    // the owner's NEXT slab of dz (g1..g3 are dead since the GEMM; first needed by the fillers of round 3) and this wave's
    // pieces of round 1 -- not earlier: the first-layer gradient above is the register peak of this kernel
    atl_load<H>(dz, nxt, lane, raw);
    G.d_load_next(base + 1, base);
    PHASE(4);
    G.rounds<FILL, Sched4>(base, sr_stride, [&](auto rc, auto sc) {
      constexpr int r = decltype(rc)::value, s_ = decltype(sc)::value;
      if constexpr (r == 3 && s_ < 40) o_chunk(s_ - 32);  // k-step 0 of the owner's next slab; the other seven ride inside its dX GEMM
    }, ph);
  }

  G.store_row(dw2_part);
  clear_dw2_rows<WG_THREADS>(dw2_part, n_part_rows);
  if constexpr (KT > 0) A1.finish<WG_THREADS>(reinterpret_cast<float *>(img), dw1_part, n_part_rows);
  PHASE(11);
  PHASE_END(3);
}

// k_bwd_dx_dw8 (HARL_BWD_SPLIT_WAVES = 1, the default): k_bwd_dx_dw with the two parts on waves of their own -- eight waves,
// two per SIMD, the same 144 KiB of LDS.  Waves 0..3 are the owners (the O part of slab base + w, nothing else), waves 4..7
// the gradient waves (the D part, row tile w - 4 of dW').  The D part never reads what the O part computes and the two use
// disjoint LDS (the weight image / the staging buffers), so each SIMD gets a second wave to issue while the other stalls on a
// load, a barrier or the LayerNorm chain -- what the single wave per SIMD of k_bwd_dx_dw did in 44 % of its phase table.
// Every wave has half the registers (<= 256: occupancy 2): the owner streams its dz by k-step and requests the LayerNorm /
// x0n operands late, the gradient waves request the next pieces after the packing instead of beside it.  The slab-to-wave
// assignment and every MFMA / reduction order are k_bwd_dx_dw's: the same bits (tests/test_gpu_bwd_split_waves.py).
// s_barrier is workgroup-wide: an owner meets the barrier of each of the four rounds of its super-round once (obar), spread
// over its slab so that owner segment k runs beside round k; the gradient waves run the rounds of the owners' super-round, so
// their second read of dz / x_hat_prev follows the owners' first by a few microseconds.
#ifndef HARL_BWD_SPLIT_WAVES
#define HARL_BWD_SPLIT_WAVES 1
#endif
struct Sched8 { static constexpr int LOAD_R0 = 47, LOAD_RN = 31; };  // after the packing: not beside tc
template <int KT, bool FILL>
__global__ __launch_bounds__(2 * WG_THREADS, 1) void k_bwd_dx_dw8(
    const float *__restrict__ dz, const float *__restrict__ xprev, const uint32_t *__restrict__ mask_prev,
    const float *__restrict__ rstd_prev, const float *__restrict__ Wp, float *__restrict__ dz_prev, long n_slabs,
    const float *__restrict__ x0n, float *__restrict__ dw1_part, float *__restrict__ dw2_part, int n_part_rows) {
  constexpr int H = BDW_H, MT = BDW_MT, NJ = BDW_NJ, NR = BDW_NR, KPF = BDW_KPF, NTH = 2 * WG_THREADS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  PHASE_BEGIN();
  auto ph = [&](auto pc) { PHASE(decltype(pc)::value); };
  u32x4 *img = reinterpret_cast<u32x4 *>(lds);
  stage_split_matrix<H, H, true, NTH>(img, Wp);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave_ = wave_id();
  const int wave = wave_ & 3;  // owner of slab base + wave / gradient wave of row tile `wave` of dW'
  const bool owner = wave_ < WAVES_PER_WG;
  const u32x4 *wl = img + lane;
  const long sr_stride = (long)gridDim.x * WAVES_PER_WG;
  const long base0 = (long)blockIdx.x * WAVES_PER_WG;
  const Ident ident = make_ident(lane);

  // ---- persistent accumulators: dW' | db' in G; dW_1' tiles and db_1' (per-lane sums over the lane's samples), KT = 1
  // (each role clears its accumulators in its own branch, and the other role's after its loop: nothing of the other role is
  // live across a role's loop)
  GradRounds G(dz, xprev, n_slabs, reinterpret_cast<unsigned char *>(img + 3 * MT * NJ * 64), lane, wave, ident);
  Dw1Acc A1;

  // ---- owner state: the slab's raw dz (streamed by k-step) and its split into the B operands of the GEMM
  float raw[NR];
  u32x4 g1[NJ], g2[NJ], g3[NJ];
  float ro0 = 0.f, ro1 = 0.f;
  auto o_chunk = [&](int k) { owner_split_chunk(k, raw, g1, g2, g3, ro0, ro1); };
  if (!owner && base0 < n_slabs) G.prologue(base0);
  PHASE(10);

  auto o_part = [&](long base) {
    const long slab = base + wave;
    const bool own = slab < n_slabs;
    // owner barrier k: meets the barrier of weight-gradient round k of this super-round (workgroup-uniform condition:
    // the rounds run for the slabs that exist).  Placement, by k-step of the dX GEMM (OB1 / OB2: after k-step OBk - 1; NJ: after
    // the GEMM; NJ + 1: after the LayerNorm backward) -- four owner segments of about one round each.
    constexpr int OB1 = KT > 0 ? 4 : 3, OB2 = KT > 0 ? NJ : 6, OB3 = KT > 0 ? NJ + 1 : NJ;
    auto obar = [&](int k) { if (base + k < n_slabs) __builtin_amdgcn_s_barrier(); };
    // =========================== O part: this wave's own slab ===========================
    if (own) {
      // dz streamed by k-step (pieces 2j, 2j + 1 of atl_load's layout = raw[8j .. 8j + 7]), RAW_LEAD k-steps ahead of
      // the split -- a third of the registers a whole slab held; no prefetch across the slabs: the gradient wave on this SIMD
      // issues while this one waits
      constexpr int RAW_LEAD = 3;
      auto raw_ks = [&](int j) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(dz + slab * (long)(H * SLAB)) + lane;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const f32x4 v = p[(2 * j + c) * WAVE];
#pragma unroll
          for (int e = 0; e < 4; ++e) raw[8 * j + 4 * c + e] = v[e];
        }
      };
#pragma unroll
      for (int j = 0; j < RAW_LEAD; ++j) raw_ks(j);
      obar(0);
#pragma unroll
      for (int k = 0; k < 8; ++k) o_chunk(k);  // k-step 0 (the other seven ride inside the GEMM)
      float xh[NR], rstd;
      uint32_t mbits[2];
      f32x4 x0r[KT > 0 ? KPF / 8 : 1];
      // the LayerNorm operands are requested at the end of the GEMM, x0n after the LayerNorm backward: across the GEMM, acc,
      // dW_1', the split terms and the weight fragments hold the registers (the four-wave kernel issued both before it; one
      // k-step earlier, or x0n with the others, spills)
      constexpr int LN_STEP = NJ;
      f32x16 acc[MT];
      zero_acc(acc);
      PHASE(0);
      // the split of k-step j + 1 of the slab's dz (raw) behind the 24 product MFMAs of k-step j, one chunk behind every third
      // MFMA (as the four-wave kernel), the request of k-step j + RAW_LEAD's dz at its start, the barriers at k-step ends
      split_gemm_fill<MT, NJ>(wl, g1, g2, g3, acc, [&](int s_, int k6) {
        const int j1 = s_ / MT + 1, q = (s_ % MT) * 6 + k6;  // q = 0..23: the MFMA's position inside k-step j
        if (j1 < NJ && q % 3 == 0) o_chunk(8 * j1 + q / 3);
        if (s_ % MT == 0 && k6 == 0 && j1 - 1 + RAW_LEAD < NJ) raw_ks(j1 - 1 + RAW_LEAD);
        if (s_ % MT == MT - 1 && k6 == 5) {  // end of k-step j1 - 1
          if (j1 == LN_STEP) owner_ln_operands(xprev, rstd_prev, mask_prev, slab, lane, xh, rstd, mbits);
          if (j1 == OB1) obar(1);
          if (j1 == OB2) obar(2);
          if (j1 == OB3) obar(3);
        }
      });
      PHASE(1);
      float out[NR];
      owner_ln_bwd(acc, xh, mbits, rstd, dz_prev, slab, lane, out);
      if constexpr (KT > 0) owner_x0_operands(x0n, slab, lane, x0r);
      if constexpr (OB3 == NJ + 1) obar(3);
      PHASE(2);
      if constexpr (KT > 0) {
        A1.add(x0r, out, ident);
        PHASE(3);
      }
    }
    else {  // no slab for this owner in the last super-round; it still meets the rounds' barriers
#pragma unroll
      for (int k = 0; k < 4; ++k) obar(k);
    }
  };
  if (owner) {
    if constexpr (KT > 0) A1.zero();
    for (long base = base0; base < n_slabs; base += sr_stride) o_part(base);
    zero_acc(G.acc2);
  } else {
    zero_acc(G.acc2);
    // =========================== D part: the four slabs of each super-round ===========================
    for (long base = base0; base < n_slabs; base += sr_stride) {
      G.d_load_next(base + 1, base);  // this wave's pieces of round 1
      PHASE(4);
      G.rounds<FILL, Sched8>(base, sr_stride, [](auto, auto) {}, ph);
    }
    if constexpr (KT > 0) A1.zero();
  }

  if (!owner) G.store_row(dw2_part);
  clear_dw2_rows<NTH>(dw2_part, n_part_rows);
  if constexpr (KT > 0) {  // A1.finish's body, here: behind the call this kernel (KT = 1: exactly 256 VGPRs) spills 12 bytes
    f32x16 a1x[4][1];
#pragma unroll
    for (int a = 0; a < 4; ++a) a1x[a][0] = A1.acc1[a];
    finish_partials<4, 1, NTH>(a1x, A1.dbs, reinterpret_cast<float *>(img), dw1_part, n_part_rows);
  }
  PHASE(11);
  PHASE_END_BY(4, 0);                     // wave 0: the owner's phases
  PHASE_END_BY(5, 64 * WAVES_PER_WG);     // wave 4: the gradient waves' phases
}
