// cathead.hip -- Categorical action heads of 65..512 actions (harl/models/base/act.py:24-43,45-86,104-157 with
// harl/models/base/distributions.py:7-25,37-55: Categorical(hidden, n) for a Discrete(n) space, availability mask), gfx950.
//
// Built like the MultiDiscrete heads (multihead.hip): the head is an ordinary Linear whose n rows are cut into GROUPS of 128
// (rows [128 g, min(128 (g + 1), n)); the last group is an ATL(64) image when it holds <= 64 rows).  The logits of every group
// come from harl_mlp_linear, the gradient into the trunk from harl_mlp_bwd_dx and the weight gradient from
// harl_mlp_dw_partials over the d(loss)/d(logits) images written here.  This file is the per-sample arithmetic in between:
// ONE softmax that spans the groups.  HBM-bound, no MFMA; one wave per 32-sample slab, lane (s, h) holds SP/2 logits of sample
// s of one group at a time, so the register budget is that of one group whatever n is.
//   pass 1  over the groups: running maximum m, sum-exp se = sum e^(z - m) and T = sum e^(z - m) (z - m), rescaled whenever a
//           group raises the maximum (online softmax); then lse = m + log se, entropy = log se - T / se, log pi(a) = z_a - lse
//   pass 2  reloads each group: d(unscaled loss)/d(logits) in place (loss), or the normalised logits to head_out (log-prob)
// Three things a group must get right: rows >= n of the last group are padding of the folded weight block (logit 0): they are
// absent from maximum, sum and entropy and their gradient is written as 0; an unavailable action's logit is the fp32 value
// -1e10 (act.py / distributions.py:52-55, not -inf), set BEFORE the maximum; samples past M (and the padding sequences of a
// recurrent batch) add nothing to part_scalars and their gradient rows are 0.
// HATRPO (harl/algorithms/actors/hatrpo.py:77-177, harl/utils/trpo_util.py:47-51,132-158) adds the surrogate in its form (mode 1
// of the loss), the head part of the Fisher-vector product (k_cat_head_fvp) and the KL sum over rows this wide (k_cat_kl).
#include "common.h"
#include "../../include/harl_hip.h"

using namespace harl;

namespace {
int bad(const char *m) {
  set_error(m);
  return -2;
}

constexpr int MAXG = HARL_MD_MAX_GROUPS;
constexpr int GROUP = 128;
constexpr float PAD = -3.0e38f;  // logit of a padding row (masked logits are -1e10: still far above it)

struct CatArgs {
  float *z[MAXG];  // logits images, ATL(sp[g]); the loss kernel overwrites them with d(loss)/d(logits)
  int sp[MAXG];
  int n_groups, n;
  long M, m_valid, m_pad;
  const int64_t *idx;
  const float *actions;  // [rows] (or [rows, 1]) indices stored as fp32
  const float *avail;    // [rows, n], 0 = unavailable; NULL = every action available
  const float *old_logp;  // [rows] (loss: by row; log-prob pass: by batch position)
  const float *adv;
  const double *adv_moments;
  const float *factor_in, *active;
  float clip_lo, clip_hi, entropy_coef;
  int mode;
  float *logp_out, *ent_out, *factor_out, *head_out, *part_scalars;
  long n_slabs;
};

// this lane's SP/2 logits of one group; logits of unavailable actions become -1e10.  av = the sample's availability row at
// the group's first action (NULL: none); cnt = real logits of the group: rows >= cnt are padding of the folded weight block
// and become PAD, a finite value below every logit (e^(PAD - m) = 0 exactly: absent from maximum, sum and entropy, probability
// 0 and therefore gradient 0, without a per-element test in the passes).
// The mask loads are unconditional (index clamped into the row) and selected afterwards: a load under a per-lane condition
// keeps one lane mask alive per element.  VEC (n a multiple of 4, 16-byte aligned rows): the four consecutive actions of a
// register quad in one 16-byte load -- a lane pair then reads 32 contiguous bytes of its row per instruction.
template <int SP, bool VEC>
__device__ __forceinline__ void group_load(const float *img, long slab, int lane, int h, int cnt, const float *av,
                                           float (&v)[64]) {
  float t[SP / 2];
  atl_load<SP>(img, slab, lane, t);
  if (av) {  // wave-uniform
    float m[SP / 2];
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < SP / 8; ++q) {
        const int f0 = feat_base(4 * q) + 4 * h;  // registers 4q .. 4q + 3 = actions f0 .. f0 + 3
        const f32x4 a4 = *reinterpret_cast<const f32x4 *>(av + min(f0, cnt - 4));
        m[4 * q + 0] = a4[0];
        m[4 * q + 1] = a4[1];
        m[4 * q + 2] = a4[2];
        m[4 * q + 3] = a4[3];
      }
    } else {
#pragma unroll
      for (int R = 0; R < SP / 2; ++R) m[R] = av[min(feat_base(R) + 4 * h, cnt - 1)];
    }
#pragma unroll
    for (int R = 0; R < SP / 2; ++R)
      if (m[R] == 0.f) t[R] = -1e10f;
  }
  if (cnt < SP) {  // wave-uniform: the last group only
#pragma unroll
    for (int R = 0; R < SP / 2; ++R)
      if (feat_base(R) + 4 * h >= cnt) t[R] = PAD;
  }
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) v[R] = t[R];
}

// pass 1 over one group: fold its logits into the running (m, se, T) of the sample and pick up the action's logit.
// m is the same in both lanes of a sample; se, T and za are per-lane partial sums (combined after the last group)
template <int SP>
__device__ __forceinline__ void group_stats(const float (&v)[64], int h, int a_local, float &m, float &se, float &T, float &za) {
  float gm = PAD;
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) gm = fmaxf(gm, v[R]);
  gm = fmaxf(gm, wave_xor32(gm));
  const float mn = fmaxf(m, gm);
  // sum e^(z - mn) (z - mn) = c (T + (m - mn) se) with c = e^(m - mn); first group: c = 0, se = T = 0
  const float c = expf(m - mn);
  T = c * (T + (m - mn) * se);
  se *= c;
  m = mn;
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) {
    const float d = v[R] - mn;
    const float e = expf(d);  // padding rows: exactly 0 (and 0 x d = -0)
    se += e;
    T += e * d;
    if (feat_base(R) + 4 * h == a_local) za = v[R];
  }
}

// pass 2 over one group: the gradient image (TRAIN) or the normalised logits of a valid sample to its head_out row
template <int SP, bool TRAIN>
__device__ __forceinline__ void group_emit(const float (&v)[64], float (&out)[64], int h, int cnt, int a_local, float lse,
                                           float ent, float dlp, float ecoef, float *ho) {
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) {
    const int f = feat_base(R) + 4 * h;
    const float lp = v[R] - lse;
    if constexpr (TRAIN) {
      const float p = expf(lp);
      const float onehot = (f == a_local && f < cnt) ? 1.f : 0.f;
      // d logp_a / dz_c = onehot - p_c ;  d ent / dz_c = -p_c (log p_c + ent); masked logits and padding rows (p = 0) receive
      // no gradient; dlp = ecoef = 0 for invalid samples
      out[R] = p == 0.f ? dlp * onehot : dlp * (onehot - p) + ecoef * (-p * (lp + ent));
    } else if (ho && f < cnt) {
      ho[f] = lp;
    }
  }
}

// TRPO (harl_cat_head_loss mode 1, hatrpo.py:77-90): the surrogate +imp * adv * factor * active itself, no clip and no entropy
// term in the gradient.  A template parameter, so that the code of modes 0 / 2 is the code it was.
template <bool TRAIN, bool VEC, bool TRPO = false>
__global__ __launch_bounds__(WG_THREADS) void k_cat_head(CatArgs A) {
  __shared__ float red[WAVES_PER_WG * PS_STRIDE];
  const int lane = threadIdx.x & 63, wave = wave_id(), i = lane & 31, h = lane >> 5;
  float adv_mean = 0.f, adv_den = 1.f;
  if (TRAIN && A.adv_moments) {  // happo.py:122-127
    const double cnt = A.adv_moments[2];
    const double mu = A.adv_moments[0] / cnt;
    const double var = A.adv_moments[1] / cnt - mu * mu;
    adv_mean = (float)mu;
    adv_den = 1.0f / ((float)sqrt(var > 0 ? var : 0.0) + 1e-5f);
  }
  float sc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) sc[k] = 0.f;

  for (long slab = (long)blockIdx.x * WAVES_PER_WG + wave; slab < A.n_slabs; slab += (long)gridDim.x * WAVES_PER_WG) {
    const long j = slab * SLAB + i;
    const bool valid = j < A.M && (A.m_pad == 0 || (j % A.m_pad) < A.m_valid);
    const long jc = j < A.M ? j : A.M - 1;
    const long row = A.idx ? A.idx[jc] : jc;
    const long orow = TRAIN ? row : jc;  // log-prob passes address old_logp / factor by batch position
    const int a = A.actions ? (int)A.actions[row] : 0;
    const float *av_row = A.avail ? A.avail + row * (long)A.n : nullptr;

    float v[64];
    float m = PAD, se = 0.f, T = 0.f, za = 0.f;
    for (int g = 0; g < A.n_groups; ++g) {
      const int cnt = min(GROUP, A.n - GROUP * g);
      const float *av = av_row ? av_row + GROUP * g : nullptr;
      if (A.sp[g] == 128) {
        group_load<128, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        group_stats<128>(v, h, a - GROUP * g, m, se, T, za);
      } else {
        group_load<64, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        group_stats<64>(v, h, a - GROUP * g, m, se, T, za);
      }
    }
    se = wave_sum32(se);
    T = wave_sum32(T);
    za = wave_sum32(za);  // one lane of the pair holds the action's logit, the other 0
    const float lgse = logf(se);
    const float lse = m + lgse;
    const float lpa = za - lse;
    const float ent = lgse - T / se;  // -sum p log p with log p = (z - m) - log se (distributions.py:7-25)

    float imp = 1.f;
    if (TRAIN || A.old_logp) imp = expf(lpa - A.old_logp[orow]);  // happo.py:66-70 (one column: prod = mean)

    float dlp = 0.f, ecoef = 0.f;
    if constexpr (!TRAIN) {
      if (valid && h == 0) {
        if (A.logp_out) A.logp_out[j] = lpa;
        if (A.ent_out) A.ent_out[j] = ent;
        if (A.factor_out) A.factor_out[j] = A.factor_out[j] * imp;  // on_policy_ha_runner.py:116-124
      }
      if (!A.head_out) continue;
    } else {
      if (A.logp_out && valid && h == 0) A.logp_out[j] = lpa;  // log pi(a|o) under the CURRENT parameters, by batch position
      const float actv = A.active ? A.active[row] : 1.f;
      const float advn = (A.adv[row] - adv_mean) * adv_den;
      const float fct = A.factor_in ? A.factor_in[row] : 1.f;
      const float surr1 = imp * advn;
      const float impc = fminf(fmaxf(imp, A.clip_lo), A.clip_hi);
      const float surr2 = impc * advn;
      const float mn = fminf(surr1, surr2);
      const float inrange = (imp >= A.clip_lo && imp <= A.clip_hi) ? 1.f : 0.f;
      float gsel = surr1 < surr2 ? 1.f : (surr1 > surr2 ? inrange : 0.5f + 0.5f * inrange);  // torch.min ties split evenly
      if (A.mode != 0) gsel = 1.f;  // HAA2C: no clip (haa2c.py:70-80)
      if constexpr (TRPO) {
        dlp = valid ? fct * actv * advn * imp : 0.f;
      } else {
        dlp = valid ? -fct * actv * advn * gsel * imp : 0.f;
        ecoef = valid ? -A.entropy_coef * actv : 0.f;  // the entropy bonus is active-mask weighted (act.py:143-150)
      }
      if (valid && h == 0) {
        if constexpr (TRPO) sc[0] += surr1 * fct * actv;
        else sc[0] += -fct * (A.mode == 2 ? surr1 : mn) * actv;
        sc[1] += actv;
        sc[2] += ent * actv;
        sc[3] += imp;
        sc[4] += 1.f;
      }
    }

    // second pass over the logits
    float *ho_row = (!TRAIN && valid) ? A.head_out + j * (long)A.n : nullptr;
    for (int g = 0; g < A.n_groups; ++g) {
      const int cnt = min(GROUP, A.n - GROUP * g);
      const float *av = av_row ? av_row + GROUP * g : nullptr;
      float *ho = ho_row ? ho_row + GROUP * g : nullptr;
      float out[64];
      if (A.sp[g] == 128) {
        group_load<128, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        group_emit<128, TRAIN>(v, out, h, cnt, a - GROUP * g, lse, ent, dlp, ecoef, ho);
        if constexpr (TRAIN) {
          float t[64];
#pragma unroll
          for (int R = 0; R < 64; ++R) t[R] = out[R];
          atl_store<128>(A.z[g], slab, lane, t);
        }
      } else {
        group_load<64, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        group_emit<64, TRAIN>(v, out, h, cnt, a - GROUP * g, lse, ent, dlp, ecoef, ho);
        if constexpr (TRAIN) {
          float t[32];
#pragma unroll
          for (int R = 0; R < 32; ++R) t[R] = out[R];
          atl_store<64>(A.z[g], slab, lane, t);
        }
      }
    }
  }

  if constexpr (TRAIN) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float t = wave_reduce_sum(sc[k]);
      if (lane == 0) red[wave * PS_STRIDE + k] = t;
    }
    __syncthreads();
    if (threadIdx.x < PS_STRIDE) {
      float t = 0.f;
      if (threadIdx.x < 8)
        t = (red[0 * PS_STRIDE + threadIdx.x] + red[1 * PS_STRIDE + threadIdx.x]) +
            (red[2 * PS_STRIDE + threadIdx.x] + red[3 * PS_STRIDE + threadIdx.x]);
      A.part_scalars[(long)blockIdx.x * PS_STRIDE + threadIdx.x] = t;
    }
  }
}

// =============================================================================================
// HATRPO Fisher-vector product, head part (harl/utils/trpo_util.py:132-158): the grouped counterpart of k_actor_head_fvp
// (heads.hip), whose arithmetic this is.  z_dot = zd_a + zd_b is the tangent of the logits (two harl_mlp_linear products per
// group), M = identity on the normalised logits q = z - logsumexp(z) over ALL n entries -- a masked entry's q = -1e10 - lse
// still moves with lse -- and the log-softmax backward of dq = q_dot goes IN PLACE into the logits images:
//   S = sum_un p_c z_dot_c,  q_dot_c = [un_c] z_dot_c - S,  sum_dq = sum_un z_dot_c - n S,
//   out_c = un_c ? (z_dot_c - S) - p_c sum_dq : 0          (un_c: available and c < n)
// pass 1 is online over the groups like group_stats: running maximum m, se = sum e^(z - m) and U = sum_un e^(z - m) z_dot,
// rescaled together; S = U / se.  pass 2 reloads logits and tangents and writes.  group_load leaves exactly -1e10 in a masked
// entry and PAD in a padding row, so un_c is `logit > -1e10`: no second walk over the availability row.
// =============================================================================================
struct CatFvpArgs {
  float *z[MAXG];  // logits images, overwritten with the result
  const float *zd_a[MAXG], *zd_b[MAXG];  // tangent images in the layout of z (zd_b: NULL = none)
  int sp[MAXG];
  int n_groups, n;
  long M, m_valid, m_pad;
  const float *avail;  // [M, n] by batch position; NULL = every action available
  long n_slabs;
};

constexpr float MASKED = -1e10f;

template <int SP>
__device__ __forceinline__ void tangent_load(const float *a, const float *b, long slab, int lane, float (&d)[64]) {
  float t[SP / 2];
  atl_load<SP>(a, slab, lane, t);
  if (b) {  // wave-uniform
    float u[SP / 2];
    atl_load<SP>(b, slab, lane, u);
#pragma unroll
    for (int R = 0; R < SP / 2; ++R) t[R] += u[R];
  }
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) d[R] = t[R];
}

// pass 1 over one group: m is the same in both lanes of a sample; se, U and sz are per-lane partial sums
template <int SP>
__device__ __forceinline__ void fvp_stats(const float (&v)[64], const float (&d)[64], float &m, float &se, float &U, float &sz) {
  float gm = PAD;
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) gm = fmaxf(gm, v[R]);
  gm = fmaxf(gm, wave_xor32(gm));
  const float mn = fmaxf(m, gm);
  const float c = expf(m - mn);  // first group: 0, and se = U = 0
  se *= c;
  U *= c;
  m = mn;
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) {
    const float e = expf(v[R] - mn);
    se += e;
    const bool un = v[R] > MASKED;  // (selects, not products: the tangent of a padding row is whatever the GEMM left there)
    U += un ? e * d[R] : 0.f;
    sz += un ? d[R] : 0.f;
  }
}

// pass 2 over one group: the result takes the tangent's place in d
template <int SP>
__device__ __forceinline__ void fvp_emit(const float (&v)[64], float (&d)[64], bool valid, float lse, float S, float sum_dq) {
#pragma unroll
  for (int R = 0; R < SP / 2; ++R) {
    const float z = valid ? v[R] : MASKED;  // (an invalid sample as a row of masked entries: one select, no branch per entry)
    const float p = expf(z - lse);
    d[R] = z > MASKED ? (d[R] - S) - p * sum_dq : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(WG_THREADS, 2) void k_cat_head_fvp(CatFvpArgs A) {
  const int lane = threadIdx.x & 63, wave = wave_id(), i = lane & 31, h = lane >> 5;
  for (long slab = (long)blockIdx.x * WAVES_PER_WG + wave; slab < A.n_slabs; slab += (long)gridDim.x * WAVES_PER_WG) {
    const long j = slab * SLAB + i;
    const bool valid = j < A.M && (A.m_pad == 0 || (j % A.m_pad) < A.m_valid);
    const long jc = j < A.M ? j : A.M - 1;
    const float *av_row = A.avail ? A.avail + jc * (long)A.n : nullptr;

    float v[64], d[64];
    float m = PAD, se = 0.f, U = 0.f, sz = 0.f;
    for (int g = 0; g < A.n_groups; ++g) {
      const int cnt = min(GROUP, A.n - GROUP * g);
      const float *av = av_row ? av_row + GROUP * g : nullptr;
      if (A.sp[g] == 128) {
        group_load<128, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        tangent_load<128>(A.zd_a[g], A.zd_b[g], slab, lane, d);
        fvp_stats<128>(v, d, m, se, U, sz);
      } else {
        group_load<64, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        tangent_load<64>(A.zd_a[g], A.zd_b[g], slab, lane, d);
        fvp_stats<64>(v, d, m, se, U, sz);
      }
    }
    se = wave_sum32(se);
    U = wave_sum32(U);
    sz = wave_sum32(sz);
    const float lse = m + logf(se);
    const float S = U / se;
    const float sum_dq = sz - (float)A.n * S;  // sum over ALL n entries of q_dot_c = [un_c] z_dot_c - S

    for (int g = 0; g < A.n_groups; ++g) {
      const int cnt = min(GROUP, A.n - GROUP * g);
      const float *av = av_row ? av_row + GROUP * g : nullptr;
      if (A.sp[g] == 128) {
        group_load<128, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        tangent_load<128>(A.zd_a[g], A.zd_b[g], slab, lane, d);
        fvp_emit<128>(v, d, valid, lse, S, sum_dq);
        atl_store<128>(A.z[g], slab, lane, d);
      } else {
        group_load<64, VEC>(A.z[g], slab, lane, h, cnt, av, v);
        tangent_load<64>(A.zd_a[g], A.zd_b[g], slab, lane, d);
        fvp_emit<64>(v, d, valid, lse, S, sum_dq);
        float t[32];
#pragma unroll
        for (int R = 0; R < 32; ++R) t[R] = d[R];
        atl_store<64>(A.z[g], slab, lane, t);
      }
    }
  }
}

// sum over rows of kl_approx(old || new) on normalised logits (trpo_util.py:47-51), rows of 65..512 entries: one wave per row,
// the lanes walk it (k_trpo_kl, heads.hip: one THREAD per row).  The reference's fp32 term order per entry -- with it a masked
// entry (both values exactly -1e10) contributes exactly 0 -- lane-partial fp32 sums, one wave reduction per row, fp64 across rows.
template <bool VEC>
__global__ __launch_bounds__(WG_THREADS) void k_cat_kl(const float *__restrict__ ho, const float *__restrict__ hn, long M, int n,
                                                       double *__restrict__ out) {
  __shared__ double sh[WAVES_PER_WG];
  const int lane = threadIdx.x & 63, wave = wave_id();
  double acc = 0;
  for (long r = (long)blockIdx.x * WAVES_PER_WG + wave; r < M; r += (long)gridDim.x * WAVES_PER_WG) {
    float k = 0.f;
    if constexpr (VEC) {  // n a multiple of 4, 16-byte aligned rows
      const f32x4 *po = reinterpret_cast<const f32x4 *>(ho + r * (long)n), *pn = reinterpret_cast<const f32x4 *>(hn + r * (long)n);
      for (int c = lane; c < n / 4; c += WAVE) {
        const f32x4 pp = po[c], q = pn[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) k += (expf(q[e] - pp[e]) - 1.f - q[e]) + pp[e];
      }
    } else {
      const float *po = ho + r * (long)n, *pn = hn + r * (long)n;
      for (int c = lane; c < n; c += WAVE) {
        const float pp = po[c], q = pn[c];
        k += (expf(q - pp) - 1.f - q) + pp;
      }
    }
    acc += (double)wave_reduce_sum(k);  // (the same value in every lane)
  }
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (sh[0] + sh[1]) + (sh[2] + sh[3]));
}

// groups of a Discrete(n) head: rows [128 g, min(128 (g + 1), n)), full groups ATL(128), the last one ATL(64 | 128)
template <class Args>
int fill_layout(Args &A, float *const *z, int n_groups, const int *sp, int n) {
  if (n < 1 || n > GROUP * MAXG || n_groups != (n + GROUP - 1) / GROUP || !z || !sp)
    return bad("Categorical head: 1..512 actions in ceil(n / 128) groups");
  for (int g = 0; g < n_groups; ++g) {
    const int cnt = n - GROUP * g < GROUP ? n - GROUP * g : GROUP;
    if ((sp[g] != 64 && sp[g] != 128) || sp[g] < cnt || !z[g])
      return bad("Categorical head: a group image is ATL(64) or ATL(128) and holds the group's logits");
    A.z[g] = z[g];
    A.sp[g] = sp[g];
  }
  A.n_groups = n_groups;
  A.n = n;
  return 0;
}

// 16-byte mask loads: every availability row starts on a 16-byte boundary and every group holds a multiple of 4 actions
template <class Args>
bool vec_mask(const Args &A) { return A.avail && (A.n & 3) == 0 && (reinterpret_cast<uintptr_t>(A.avail) & 15) == 0; }
}  // namespace

extern "C" int harl_cat_head_fvp(float *const *z, const float *const *zd_a, const float *const *zd_b, int n_groups,
                                 const int *sp, int n, long M, const float *avail, long m_valid, long m_pad, void *stream) {
  if (M <= 0) return 0;
  CatFvpArgs A{};
  if (int rc = fill_layout(A, z, n_groups, sp, n)) return rc;
  if (!zd_a) return bad("harl_cat_head_fvp: the tangent images zd_a are required");
  for (int g = 0; g < n_groups; ++g) {
    if (!zd_a[g] || (zd_b && !zd_b[g])) return bad("harl_cat_head_fvp: one tangent image per group");
    A.zd_a[g] = zd_a[g];
    A.zd_b[g] = zd_b ? zd_b[g] : nullptr;
  }
  A.M = M; A.m_valid = m_valid; A.m_pad = m_pad; A.avail = avail;
  A.n_slabs = n_slabs_of(M);
  const int grid = persistent_grid(A.n_slabs, 4);
  if (vec_mask(A)) hipLaunchKernelGGL((k_cat_head_fvp<true>), dim3(grid), dim3(WG_THREADS), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL((k_cat_head_fvp<false>), dim3(grid), dim3(WG_THREADS), 0, (hipStream_t)stream, A);
  return check_launch("harl_cat_head_fvp");
}

extern "C" int harl_cat_kl_sum(const float *head_old, const float *head_new, long M, int n, double *out_sum, void *stream) {
  if (M <= 0) return 0;
  if (!head_old || !head_new || !out_sum || n < 1) return bad("harl_cat_kl_sum: head_old, head_new, out_sum and n >= 1 are required");
  const long wgs = (M + WAVES_PER_WG - 1) / WAVES_PER_WG;
  const int grid = (int)(wgs < 2048 ? wgs : 2048);  // up to eight workgroups per CU: nothing but loads in flight
  const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(head_old) | reinterpret_cast<uintptr_t>(head_new)) & 15) == 0;
  if (vec) hipLaunchKernelGGL((k_cat_kl<true>), dim3(grid), dim3(WG_THREADS), 0, (hipStream_t)stream, head_old, head_new, M, n, out_sum);
  else hipLaunchKernelGGL((k_cat_kl<false>), dim3(grid), dim3(WG_THREADS), 0, (hipStream_t)stream, head_old, head_new, M, n, out_sum);
  return check_launch("harl_cat_kl_sum");
}

extern "C" int harl_cat_head_logp(const float *const *z, int n_groups, const int *sp, int n, long M, const int64_t *idx,
                                  const float *actions, const float *avail, float *logp_out, float *ent_out,
                                  const float *old_logp, float *factor, float *head_out, long m_valid, long m_pad,
                                  void *stream) {
  if (M <= 0) return 0;
  CatArgs A{};
  if (int rc = fill_layout(A, const_cast<float *const *>(reinterpret_cast<const float *const *>(z)), n_groups, sp, n)) return rc;
  if (factor && !old_logp) return bad("harl_cat_head_logp: the factor product needs old_logp");
  A.M = M; A.m_valid = m_valid; A.m_pad = m_pad; A.idx = idx;
  A.actions = actions; A.avail = avail; A.logp_out = logp_out; A.ent_out = ent_out; A.old_logp = old_logp;
  A.factor_out = factor; A.head_out = head_out;
  A.n_slabs = n_slabs_of(M);
  const int grid = persistent_grid(A.n_slabs, 4);
  if (vec_mask(A)) hipLaunchKernelGGL((k_cat_head<false, true>), dim3(grid), dim3(WG_THREADS), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL((k_cat_head<false, false>), dim3(grid), dim3(WG_THREADS), 0, (hipStream_t)stream, A);
  return check_launch("harl_cat_head_logp");
}

extern "C" int harl_cat_head_loss(float *const *z, int n_groups, const int *sp, int n, long M, const int64_t *idx,
                                  const float *actions, const float *avail, const float *old_logp, const float *adv,
                                  const double *adv_moments, const float *factor, const float *active, double clip_param,
                                  float entropy_coef, int mode, long m_valid, long m_pad, float *logp_out,
                                  float *part_scalars, int n_blocks, void *stream) {
  if (M <= 0) return 0;
  CatArgs A{};
  if (int rc = fill_layout(A, z, n_groups, sp, n)) return rc;
  if (mode < 0 || mode > 2) return bad("harl_cat_head_loss: mode 0 (HAPPO / MAPPO), 1 (HATRPO) or 2 (HAA2C)");
  if (n_blocks < 1) return bad("harl_cat_head_loss: n_blocks must be positive");
  if (!actions || !old_logp || !adv || !part_scalars) return bad("harl_cat_head_loss: actions, old_logp, adv and part_scalars are required");
  A.M = M; A.m_valid = m_valid; A.m_pad = m_pad; A.idx = idx;
  A.actions = actions; A.avail = avail; A.old_logp = old_logp; A.adv = adv; A.adv_moments = adv_moments;
  A.factor_in = factor; A.active = active;
  A.clip_lo = (float)(1.0 - clip_param); A.clip_hi = (float)(1.0 + clip_param);
  A.entropy_coef = entropy_coef; A.mode = mode;
  A.logp_out = logp_out; A.part_scalars = part_scalars;
  A.n_slabs = n_slabs_of(M);
  const dim3 grid(n_blocks), wg(WG_THREADS);
  if (mode == 1) {
    if (vec_mask(A)) hipLaunchKernelGGL((k_cat_head<true, true, true>), grid, wg, 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL((k_cat_head<true, false, true>), grid, wg, 0, (hipStream_t)stream, A);
  } else if (vec_mask(A)) hipLaunchKernelGGL((k_cat_head<true, true>), grid, wg, 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL((k_cat_head<true, false>), grid, wg, 0, (hipStream_t)stream, A);
  return check_launch("harl_cat_head_loss");
}
