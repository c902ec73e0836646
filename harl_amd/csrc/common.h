// common.h -- shared device helpers for the gfx950 kernels (wave64, MFMA 32x32x2 f32 layouts).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// Phase timing (debug builds only: -DHARL_PHASE_TIMING, `python -m harl_amd._build` variant "phase", tools/phase_cycles.py).
// s_memtime at phase boundaries of the persistent kernels' slab loops, summed per phase over the slabs of wave 0 of
// workgroup 0 and left in a per-translation-unit device array that harl_phase_read_<tu>() copies out.  Compiled out otherwise.
// ---------------------------------------------------------------------------------------------
#ifdef HARL_PHASE_TIMING
#define HARL_NPHASE 12
static __device__ long long harl_phase_cyc[8][HARL_NPHASE];
// per workgroup (wave 0): {shader cycles PHASE_BEGIN..PHASE_END, s_memrealtime (100 MHz) at PHASE_BEGIN, at PHASE_END} -- the
// spread of the workgroups' loop times, their start skew and the shader clock under load (tools/phase_cycles.py --wg)
static __device__ long long harl_phase_wg[8][256][3];
#define PHASE_BEGIN()                                    \
  long long _pt_acc[HARL_NPHASE];                        \
  for (int _k = 0; _k < HARL_NPHASE; ++_k) _pt_acc[_k] = 0; \
  const long long _pt_rt0 = __builtin_amdgcn_s_memrealtime(); \
  const long long _pt_c0 = __builtin_readcyclecounter(); \
  long long _pt_last = _pt_c0;
#define PHASE(i)                                         \
  do {                                                   \
    __builtin_amdgcn_sched_barrier(0);                   \
    const long long _t = __builtin_readcyclecounter();   \
    _pt_acc[i] += _t - _pt_last;                         \
    _pt_last = _t;                                       \
    __builtin_amdgcn_sched_barrier(0);                   \
  } while (0)
#define PHASE_END(slot) PHASE_END_BY(slot, 0)
// ... recorded by thread `tid` (its wave's sums: kernels whose waves take different roles)
#define PHASE_END_BY(slot, tid)                          \
  do {                                                   \
    if (blockIdx.x == 0 && threadIdx.x == (tid))         \
      for (int _k = 0; _k < HARL_NPHASE; ++_k) harl_phase_cyc[slot][_k] = _pt_acc[_k]; \
    if (threadIdx.x == (tid) && blockIdx.x < 256) {      \
      harl_phase_wg[slot][blockIdx.x][0] = __builtin_readcyclecounter() - _pt_c0; \
      harl_phase_wg[slot][blockIdx.x][1] = _pt_rt0;      \
      harl_phase_wg[slot][blockIdx.x][2] = __builtin_amdgcn_s_memrealtime(); \
    }                                                    \
  } while (0)
#define HARL_PHASE_ACCESSOR(tu)                                                                    \
  extern "C" int harl_phase_read_##tu(long long *out) {                                            \
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(harl_phase_cyc), sizeof(long long) * 8 * HARL_NPHASE); \
  }                                                                                                \
  extern "C" int harl_phase_read_wg_##tu(long long *out) {                                         \
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(harl_phase_wg), sizeof(long long) * 8 * 256 * 3); \
  }
#else
#define PHASE_BEGIN()
#define PHASE(i)
#define PHASE_END(slot)
#define PHASE_END_BY(slot, tid)
#define HARL_PHASE_ACCESSOR(tu)
#endif

namespace harl {

constexpr int WAVE = 64;
constexpr int SLAB = 32;          // samples per wave-slab (N dimension of v_mfma_f32_32x32x2_f32)
constexpr int WG_THREADS = 256;   // 4 waves
constexpr int WAVES_PER_WG = 4;
constexpr int PS_STRIDE = 48;     // floats per partial-scalar row: [0..8) scalars, [8..40) per-dim sums
constexpr int DHEAD_LD = 32;      // row stride of the head-gradient matrix (head width padded to 32)

void set_error(const char *msg);
int check_launch(const char *what);

// ---------------------------------------------------------------------------------------------
// Register <-> feature map of the "C layout" of v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md §3):
// a 32x32 tile D[row][col]: lane l holds col = l & 31 and, in register r (0..15),
// row = (r & 3) + 8*(r >> 2) + 4*(l >> 5).
// We compute Y^T = W * X^T, i.e. tile rows = output features, tile cols = samples, so lane
// (s = l&31, h = l>>5) holds sample s and, for register index R = 16*t + r of a width-H
// activation, feature  f(R, h) = 32*t + (r&3) + 8*(r>>2) + 4*h.   Each lane holds H/2 features.
// Because a GEMM's k order is free, the same register file is directly the B operand of the
// next layer's MFMA (k-step R: half h supplies feature f(R,h)) -- no transpose between layers.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ constexpr int feat_base(int R) {  // f(R, 0)
  return 32 * (R >> 4) + (R & 3) + 8 * ((R & 15) >> 2);
}

// The wave's index in its workgroup.  It is uniform across the wave, which the compiler cannot see through threadIdx.x >> 6:
// readfirstlane tells it, and the slab counters, loop bounds and every address derived from them move to scalar registers
// and the scalar ALU (fewer vector registers, fewer VALU slots in the slab loops).
#ifdef HARL_NO_WAVE_ID  // A/B switch (tools): the plain vector-register wave index
__device__ __forceinline__ int wave_id() { return (int)(threadIdx.x >> 6); }
#else
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
#endif
// a value that is the same in every lane of the wave, moved to a scalar register
__device__ __forceinline__ float uniform_f(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
__device__ __forceinline__ float wave_xor32(float v) {  // exchange with the partner half (lane ^ 32)
  return __shfl_xor(v, 32, 64);
}
// v + (the partner half's v), in every lane.  v_permlane32_swap exchanges lanes 32-63 of its first operand with lanes 0-31 of
// its second; with both operands = v the two results are {own, partner} in one half and {partner, own} in the other, so
// their sum is the same commutative fp32 addition everywhere.  9 + 5 cycles; __shfl_xor(v, 32) is a ds_bpermute_b32 whose LDS
// round trip (~60 cycles, tools/valu_cost.hip) sits on the critical path of every LayerNorm statistic.
__device__ __forceinline__ float wave_sum32(float v) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// sum over the 32 lanes of each half (lanes 0-31 and 32-63 separately); result in every lane of the half
__device__ __forceinline__ float half_reduce_sum(float v) {
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_reduce_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ATL (activation tile layout): slab g of a width-H activation = [H/8][64 lanes][4] floats.
template <int H>
__device__ __forceinline__ void atl_load(const float *__restrict__ base, long slab, int lane, float (&x)[H / 2]) {
  const f32x4 *p = reinterpret_cast<const f32x4 *>(base + slab * (long)(H * SLAB)) + lane;
#pragma unroll
  for (int q = 0; q < H / 8; ++q) {
    f32x4 v = p[q * WAVE];
    x[4 * q + 0] = v[0];
    x[4 * q + 1] = v[1];
    x[4 * q + 2] = v[2];
    x[4 * q + 3] = v[3];
  }
}
template <int H>
__device__ __forceinline__ void atl_store(float *__restrict__ base, long slab, int lane, const float (&x)[H / 2]) {
  f32x4 *p = reinterpret_cast<f32x4 *>(base + slab * (long)(H * SLAB)) + lane;
#pragma unroll
  for (int q = 0; q < H / 8; ++q) {
    f32x4 v;
    v[0] = x[4 * q + 0];
    v[1] = x[4 * q + 1];
    v[2] = x[4 * q + 2];
    v[3] = x[4 * q + 3];
    p[q * WAVE] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// ReLU masks.  One bit per (sample, feature): lane (s, h) keeps H/2 bits in (H/2+31)/32 words, feature register R in
// word R>>5, pushed MSB-first (R = 0 ends up in bit 31) and consumed in the same order by shifting the top bit out
// into VCC.  On gfx950 VALU instructions are NOT overlapped with another wave's MFMAs on the same SIMD (measured:
// tools/mfma_lds.hip, time = 64 cycles x MFMAs + 4 cycles x VALU ops), so the epilogues of the MFMA kernels are written
// for instruction count: 3 ops per element for relu + mask here (compare, select, add-with-carry), 2 to apply a mask.
// ---------------------------------------------------------------------------------------------
#ifndef HARL_NO_PK
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
#ifdef HARL_PK_SPLIT_OFF
constexpr bool PK_DEFAULT = false;  // A/B: only the operand splits unpacked
#else
constexpr bool PK_DEFAULT = true;
#endif
#else
// A/B build (tools/build_variants.py nopk=-DHARL_NO_PK): the same arithmetic on register pairs as two scalar instructions
// instead of one v_pk_*_f32 (MI355X guide: packed fp32 VALU beside MFMAs costs more than the two scalar instructions it replaces)
struct f32x2 {
  float x, y;
  __device__ __forceinline__ float operator[](int i) const { return i ? y : x; }
  __device__ __forceinline__ f32x2 &operator+=(const f32x2 &o) { x += o.x; y += o.y; return *this; }
};
__device__ __forceinline__ f32x2 operator+(f32x2 a, f32x2 b) { return f32x2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ f32x2 operator-(f32x2 a, f32x2 b) { return f32x2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ f32x2 operator*(f32x2 a, f32x2 b) { return f32x2{a.x * b.x, a.y * b.y}; }
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return f32x2{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)}; }
constexpr bool PK_DEFAULT = false;
#endif

__device__ __forceinline__ float relu_push(float a, uint32_t &bits) {  // returns a > 0 ? a : 0 ; bits = bits<<1 | (a>0)
  float v;
  asm volatile("v_cmp_lt_f32 vcc, 0, %2\n\tv_cndmask_b32 %0, 0, %2, vcc\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc"
               : "=&v"(v), "+v"(bits)
               : "v"(a)
               : "vcc");
  return v;
}
// max(a, 0) as ONE instruction: fmaxf() costs a second v_max_f32 (x, x) in front -- the canonicalisation IEEE maxNum asks for
// when the compiler cannot prove its input is not a signalling NaN (256 instead of 128 VALU per slab in the log-prob passes),
// and it folds v_med3_f32(a, 0, +inf) back into the same pair.  The INTEGER maximum of the bit pattern with 0 is the same
// function (negative floats, -0 included, are negative integers; positive floats keep their bits) and a plain v_max_i32.
// Not inline asm: these values come straight out of MFMAs, and the wait states between a matrix instruction's write and a
// VALU read are software's job on gfx9 -- the hazard recogniser inserts them for instructions it knows, not for the operands
// of an asm statement (measured in round 4: `v_max_f32` in an asm statement read stale accumulators).
__device__ __forceinline__ float relu_plain(float a) {
  const int b = __float_as_int(a);
  return __int_as_float(b > 0 ? b : 0);
}
__device__ __forceinline__ float mask_pop(float x, uint32_t &bits) {  // returns top bit ? x : 0 ; bits <<= 1
  float o;
  asm volatile("v_add_co_u32 %1, vcc, %1, %1\n\tv_cndmask_b32 %0, 0, %2, vcc" : "=&v"(o), "+v"(bits) : "v"(x) : "vcc");
  return o;
}

// backward of  x_hat = norm(relu(z))  for one sample per lane-pair:
//   da = rstd (dx_hat - mean_f(dx_hat) - x_hat mean_f(dx_hat x_hat)) ;  dz = relu_mask ? da : 0 ; store ATL
// evaluated as  da = fma(x_hat, -s2 rstd, fma(dx_hat, rstd, -s1 rstd))  on register pairs (v_pk_fma_f32).
template <int H>
__device__ __forceinline__ void ln_bwd_relu_mbits(const float (&dx)[H / 2], const float (&xh)[H / 2],
                                                 const uint32_t (&bits_in)[(H / 2 + 31) / 32], float rstd, float (&out)[H / 2]) {
  // the ReLU-mask words come in registers: the callers load them BEFORE their GEMM (behind its sched_barriers a load at the
  // point of use is issued after the last MFMA and its whole latency is exposed once per slab)
  constexpr int NR = H / 2;
  constexpr int NW = (NR + 31) / 32;
  f32x2 a1 = {0.f, 0.f}, a2 = {0.f, 0.f};
#pragma unroll
  for (int P = 0; P < NR / 2; ++P) {
    const f32x2 d = {dx[2 * P], dx[2 * P + 1]}, x = {xh[2 * P], xh[2 * P + 1]};
    a1 += d;
    a2 += d * x;
  }
  float s1 = a1[0] + a1[1], s2 = a2[0] + a2[1];
  s1 = wave_sum32(s1);
  s2 = wave_sum32(s2);
  const float c1 = -(s1 * (1.0f / H)) * rstd, c2 = -(s2 * (1.0f / H)) * rstd;
  const f32x2 c1v = {c1, c1}, c2v = {c2, c2}, rv = {rstd, rstd};
  uint32_t bits[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) bits[w] = bits_in[w];
#pragma unroll
  for (int P = 0; P < NR / 2; ++P) {
    const f32x2 d = {dx[2 * P], dx[2 * P + 1]}, x = {xh[2 * P], xh[2 * P + 1]};
    const f32x2 da = fma2(x, c2v, fma2(d, rv, c1v));
    out[2 * P] = mask_pop(da[0], bits[(2 * P) >> 5]);
    out[2 * P + 1] = mask_pop(da[1], bits[(2 * P + 1) >> 5]);
  }
}

template <int H>
__device__ __forceinline__ void ln_bwd_relu_regs(const float (&dx)[H / 2], const float (&xh)[H / 2],
                                                 const uint32_t *__restrict__ mask_in, float rstd, int lane, long slab,
                                                 float (&out)[H / 2]) {
  constexpr int NW = (H / 2 + 31) / 32;
  uint32_t bits[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) bits[w] = mask_in[(slab * NW + w) * WAVE + lane];
  ln_bwd_relu_mbits<H>(dx, xh, bits, rstd, out);
}

template <int H>
__device__ __forceinline__ void ln_bwd_relu_store(const float (&dx)[H / 2], const float (&xh)[H / 2],
                                                  const uint32_t *__restrict__ mask_in, float rstd, int lane, long slab,
                                                  float *__restrict__ dz_out) {
  float out[H / 2];
  ln_bwd_relu_regs<H>(dx, xh, mask_in, rstd, lane, slab, out);
  atl_store<H>(dz_out, slab, lane, out);
}

// Workgroup-cooperative copy of a row-major [ROWS][COLS] fp32 matrix from global memory into LDS with row stride LD.
// All of a thread's float4 loads are issued before the first LDS write: the prologue of the persistent MFMA kernels
// costs one L2 latency instead of ROWS*COLS/NTHR dependent-looking scalar round trips (it was ~20 us of a ~250 us
// kernel, see tools/mfma_lds.hip).  Falls back to scalar loads when src is not 16-byte aligned.
template <int ROWS, int COLS, int LD, int NTHR>
__device__ __forceinline__ void stage_matrix(float *__restrict__ dst, const float *__restrict__ src) {
  static_assert(COLS % 4 == 0, "rows are copied in float4 pieces");
  constexpr int NV = ROWS * COLS / 4, PER = (NV + NTHR - 1) / NTHR;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    f32x4 v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e4 = threadIdx.x + u * NTHR;
      v[u] = e4 < NV ? reinterpret_cast<const f32x4 *>(src)[e4] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e4 = threadIdx.x + u * NTHR;
      if (e4 < NV) {
        const int e = 4 * e4, o = e / COLS, k = e - o * COLS;
        float *d = dst + o * LD + k;
        if constexpr (LD % 4 == 0) {
          *reinterpret_cast<f32x4 *>(d) = v[u];
        } else {
          d[0] = v[u][0];
          d[1] = v[u][1];
          d[2] = v[u][2];
          d[3] = v[u][3];
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < ROWS * COLS; e += NTHR) {
      const int o = e / COLS, k = e - o * COLS;
      dst[o * LD + k] = src[e];
    }
  }
}

// dynamic LDS above 64 KiB needs an explicit opt-in per kernel; done once per (kernel, size): the call is not a stream
// operation and must not run while a stream is being captured into a hipGraph (the first, eager call of a sequence has
// raised the limit by then)
bool lds_opt_in_needed(const void *kernel, size_t bytes);  // elementwise.hip
template <typename F>
inline void allow_big_lds(F kernel, size_t bytes) {
  if (bytes > 48 * 1024 && lds_opt_in_needed(reinterpret_cast<const void *>(kernel), bytes))
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

inline long n_slabs_of(long M) { return (M + SLAB - 1) / SLAB; }
inline int persistent_grid(long n_slabs, int wg_per_cu) {
  long wgs = (n_slabs + WAVES_PER_WG - 1) / WAVES_PER_WG;
  long cap = 256L * wg_per_cu;
  return (int)(wgs < cap ? (wgs < 1 ? 1 : wgs) : cap);
}

}  // namespace harl
