// Generalised Jensen-Shannon divergence JSD(beta) between a student row and the mean of K teacher
// rows, on bf16 logits at an inverse temperature (on-policy distillation, GKD; Agarwal et al.).
//
//   i = inv_temp,  q = softmax(i s),  p = (1/K) sum_k softmax(i t_k)
//   beta = 0      L = sum_v p (log p - log q)                    forward KL
//   beta = 1      L = A,  A = sum_v q (log q - log p)            reverse KL
//   0 < beta < 1  m = beta p + (1 - beta) q,  P = sum_v p (log p - log m),
//                 A = sum_v q (log q - log m),  L = beta P + (1 - beta) A
//   dL/ds_v = i (q_v - p_v)                         beta = 0
//   dL/ds_v = i c q_v (log q_v - log m_v - A)       beta > 0;  c = 1 - beta (beta = 1: c = 1, m = p)
//
// Everything stays in the log domain (fp32 exp underflows below -104): log q_v and log p_kv are a
// scaled difference to the row's RAW max minus the log of the row sum; log p is the logsumexp over
// the K teachers minus log K (K = 1: the teacher's own value); log m is
// logaddexp(log beta + log p, log(1 - beta) + log q) as max + log(1 + exp(-|a - b|)). log beta and
// log(1 - beta) arrive as fp32 arguments formed in double by the host.
// q_v = 0 (student logit -inf) adds exactly 0 to A and gets gradient exactly 0; p_v = 0 adds exactly
// 0 to the p sums; the mathematically infinite cases (beta = 0 with q_v = 0 < p_v, beta = 1 with
// p_v = 0 < q_v) give +inf.
//
// Forward: one 256-thread block per row, one launch. Sweep 1 runs the online (max, sum-exp) of the
// student row and of every teacher row together, K + 1 independent 16 B load streams per lane;
// sweep 2 re-reads the same rows (the block's own working set) and accumulates P and / or A per
// lane; the block sums go through wave_sum and a 4-entry LDS array in fixed order: no atomics, the
// same bits every run. Backward: one block per row, one sweep, dL/ds written as bf16 into a buffer
// of its own; the inputs are only read.
// A row whose row_mask entry is 0 leaves before its logits are loaded: loss, aux, lse and gradient 0.
#include "common.h"
#include "gjsd_params.h"

namespace dla {

namespace {

enum { GJSD_FWD_KL = 0, GJSD_MIXED = 1, GJSD_REV_KL = 2 };

__device__ __forceinline__ bool row_live(const GjsdParams& p, int64_t r) {
  if (!p.mask) return true;
  return p.mask_u8 ? static_cast<const uint8_t*>(p.mask)[r] != 0 : static_cast<const float*>(p.mask)[r] != 0.f;
}

// W logits of one row at vector index i (VEC: 8 from one 16 B load; else 1)
template <bool VEC>
__device__ __forceinline__ void load_w(const bf16_t* row, int i, float (&x)[VEC ? 8 : 1]) {
  if constexpr (VEC) {
    const bf16x8 a = load_bf16x8(row + static_cast<int64_t>(i) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = bf2f(a[j]);
  } else {
    x[0] = bf2f(row[i]);
  }
}

// online (raw max, sum of exp of scaled differences): row_lse<.., TEMP>'s per-lane update
template <int W>
__device__ __forceinline__ void online_update(const float (&x)[W], float& m, float& s, float it) {
#pragma clang fp contract(off)
  float lm = x[0];
#pragma unroll
  for (int j = 1; j < W; ++j) lm = fmaxf(lm, x[j]);
  if (lm == -INFINITY) return;  // W logits of -inf add 0 (with m still -inf, x - m would be NaN)
  if (lm > m) {
    s *= __expf((m - lm) * it);
    m = lm;
  }
#pragma unroll
  for (int j = 0; j < W; ++j) s += __expf((x[j] - m) * it);
}

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2, float it) {
#pragma clang fp contract(off)
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf((m - mn) * it) + s2 * __expf((m2 - mn) * it);
  m = mn;
}

// log of the mean over K <= KT teachers of exp(lpk[k]); -inf when every teacher has p = 0 there.
// The entries k >= K hold -inf: they leave the max alone and add exp(-inf) = 0 to the sum.
template <int KT>
__device__ __forceinline__ float log_mean_exp(const float (&lpk)[KT], float logK) {
#pragma clang fp contract(off)
  if constexpr (KT == 1) return lpk[0];
  float mk = lpk[0];
#pragma unroll
  for (int k = 1; k < KT; ++k) mk = fmaxf(mk, lpk[k]);
  if (mk == -INFINITY) return -INFINITY;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) sum += __expf(lpk[k] - mk);
  return mk + __logf(sum) - logK;
}

// log(beta p + (1 - beta) q) from log p and log q; -inf when both are
__device__ __forceinline__ float log_mix(float lp, float lq, float lb, float l1b) {
#pragma clang fp contract(off)
  const float a = lb + lp, b = l1b + lq;
  const float mx = fmaxf(a, b);
  if (mx == -INFINITY) return -INFINITY;
  return mx + __logf(1.f + __expf(-fabsf(a - b)));  // one side -inf: |a - b| = inf, exp = 0
}

// one vocabulary entry's terms of P = sum p (log p - log m') and A = sum q (log q - log m'), m' = q
// (beta = 0, P only), p (beta = 1, A only) or the mixture
template <int MODE>
__device__ __forceinline__ void accumulate(float lq, float lp, float lb, float l1b, float& P, float& A) {
#pragma clang fp contract(off)
  if constexpr (MODE == GJSD_FWD_KL) {
    if (lp != -INFINITY) P = lq == -INFINITY ? INFINITY : __builtin_fmaf(__expf(lp), lp - lq, P);
  } else if constexpr (MODE == GJSD_REV_KL) {
    if (lq != -INFINITY) A = lp == -INFINITY ? INFINITY : __builtin_fmaf(__expf(lq), lq - lp, A);
  } else {
    const float lm = log_mix(lp, lq, lb, l1b);
    if (lp != -INFINITY) P = __builtin_fmaf(__expf(lp), lp - lm, P);
    if (lq != -INFINITY) A = __builtin_fmaf(__expf(lq), lq - lm, A);
  }
}

}  // namespace

// One row of the forward for K <= KM teachers; KM is the unroll bound of every per-teacher loop (the
// kernel picks the smallest of 1, 2, 4, 8 that holds K, so K = 1 and K = 2 run no predicated spare).
template <bool VEC, int MODE, int KM>
__device__ __forceinline__ void gjsd_fwd_row(const GjsdParams& p, float (*sm)[4], float (*ss)[4], float* redP,
                                             float* redA) {
  constexpr int W = VEC ? 8 : 1;
  const int64_t r = blockIdx.x;
  const int K = KM <= 2 ? KM : p.K;
  if (!row_live(p, r)) {  // row-uniform: the whole block leaves, before any barrier
    if (threadIdx.x == 0) {
      p.loss[r] = 0.f;
      p.aux[r] = 0.f;
      p.s_lse[r] = 0.f;
      for (int k = 0; k < K; ++k) p.t_lse[k * p.N + r] = 0.f;
    }
    return;
  }
  const bf16_t* srow = p.s + r * p.s_ld;
  const bf16_t* trow = p.t + r * p.t_ld;
  const float it = p.it;
  const int n = VEC ? p.V >> 3 : p.V;

  // ---- sweep 1: stream 0 = student, stream 1 + k = teacher k
  float m[KM + 1], s[KM + 1];
#pragma unroll
  for (int j = 0; j <= KM; ++j) {
    m[j] = -INFINITY;
    s[j] = 0.f;
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    float x[KM + 1][W];
    load_w<VEC>(srow, i, x[0]);
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) load_w<VEC>(trow + k * p.t_sk, i, x[1 + k]);
    online_update<W>(x[0], m[0], s[0], it);
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) online_update<W>(x[1 + k], m[1 + k], s[1 + k], it);
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j <= KM; ++j) {
    if (j <= K) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m[j], o, 64), s2 = __shfl_xor(s[j], o, 64);
        online_merge(m[j], s[j], m2, s2, it);
      }
      if (lane == 0) {
        sm[j][w] = m[j];
        ss[j][w] = s[j];
      }
    }
  }
  __syncthreads();
  float ls[KM + 1];  // log of the row sum: log softmax(i z)_v = (z_v - m) i - ls
#pragma unroll
  for (int j = 0; j <= KM; ++j) {
    ls[j] = 0.f;
    if (j <= K) {
      m[j] = sm[j][0];
      s[j] = ss[j][0];
#pragma unroll
      for (int q = 1; q < 4; ++q) online_merge(m[j], s[j], sm[j][q], ss[j][q], it);
      ls[j] = logf(s[j]);
    }
  }
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    p.s_lse[r] = m[0] * it + ls[0];
    for (int k = 0; k < K; ++k) p.t_lse[k * p.N + r] = m[1 + k] * it + ls[1 + k];
  }

  // ---- sweep 2
  float P = 0.f, A = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    float x[KM + 1][W];
    load_w<VEC>(srow, i, x[0]);
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) load_w<VEC>(trow + k * p.t_sk, i, x[1 + k]);
#pragma unroll
    for (int j = 0; j < W; ++j) {
#pragma clang fp contract(off)
      const float lq = (x[0][j] - m[0]) * it - ls[0];
      float lpk[KM];
#pragma unroll
      for (int k = 0; k < KM; ++k) lpk[k] = k < K ? (x[1 + k][j] - m[1 + k]) * it - ls[1 + k] : -INFINITY;
      const float lp = log_mean_exp<KM>(lpk, p.logK);
      accumulate<MODE>(lq, lp, p.lb, p.l1b, P, A);
    }
  }
  if constexpr (MODE != GJSD_REV_KL) P = wave_sum(P);
  if constexpr (MODE != GJSD_FWD_KL) A = wave_sum(A);
  if (lane == 0) {
    redP[w] = P;
    redA[w] = A;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    P = ((redP[0] + redP[1]) + redP[2]) + redP[3];
    A = ((redA[0] + redA[1]) + redA[2]) + redA[3];
    if constexpr (MODE == GJSD_FWD_KL) {
      p.loss[r] = P;
      p.aux[r] = 0.f;
    } else if constexpr (MODE == GJSD_REV_KL) {
      p.loss[r] = A;
      p.aux[r] = A;
    } else {
      p.loss[r] = p.beta * P + p.c * A;
      p.aux[r] = A;
    }
  }
}

// ds[r, v] = g[r] i (q - p)  (beta = 0)  or  g[r] i c q (log q - log m - A[r]); q = 0 -> 0.
template <bool VEC, int MODE, int KM>
__device__ __forceinline__ void gjsd_bwd_row(const GjsdParams& p) {
  constexpr int W = VEC ? 8 : 1;
  const int64_t r = blockIdx.x;
  const int K = KM <= 2 ? KM : p.K;
  const int n = VEC ? p.V >> 3 : p.V;
  bf16_t* drow = p.ds + r * static_cast<int64_t>(p.V);
  if (!row_live(p, r)) {
    for (int i = threadIdx.x; i < n; i += 256) {
      if constexpr (VEC) store_bf16x8(drow + static_cast<int64_t>(i) * 8, bf16x8{0, 0, 0, 0, 0, 0, 0, 0});
      else drow[i] = 0;
    }
    return;
  }
  const bf16_t* srow = p.s + r * p.s_ld;
  const bf16_t* trow = p.t + r * p.t_ld;
  const float it = p.it;
  const float sl = p.s_lse[r], A = p.aux[r];
  float tl[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) tl[k] = k < K ? p.t_lse[k * p.N + r] : 0.f;
  float gi, gic;
  {
#pragma clang fp contract(off)  // each product rounded on its own
    gi = p.g[r] * it;
    gic = gi * p.c;
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    float x[KM + 1][W], o[W];
    load_w<VEC>(srow, i, x[0]);
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) load_w<VEC>(trow + k * p.t_sk, i, x[1 + k]);
#pragma unroll
    for (int j = 0; j < W; ++j) {
#pragma clang fp contract(off)
      const float lq = x[0][j] * it - sl;
      const float q = __expf(lq);
      if constexpr (MODE == GJSD_FWD_KL) {
        float pb = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k)
          if (k < K) pb += __expf(x[1 + k][j] * it - tl[k]);
        o[j] = gi * (q - pb * p.invK);
      } else {
        float lpk[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) lpk[k] = k < K ? x[1 + k][j] * it - tl[k] : -INFINITY;
        const float lp = log_mean_exp<KM>(lpk, p.logK);
        const float lm = MODE == GJSD_REV_KL ? lp : log_mix(lp, lq, p.lb, p.l1b);
        o[j] = lq == -INFINITY ? 0.f : (gic * q) * ((lq - lm) - A);
      }
    }
    if constexpr (VEC) store_bf16x8(drow + static_cast<int64_t>(i) * 8, pack_bf16x8(o));
    else drow[i] = f2bf(o[0]);
  }
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void gjsd_fwd_kernel(const GjsdParams p) {
  __shared__ float sm[kGjsdMaxTeachers + 1][4], ss[kGjsdMaxTeachers + 1][4], redP[4], redA[4];
  if (p.K == 1) gjsd_fwd_row<VEC, MODE, 1>(p, sm, ss, redP, redA);  // block-uniform
  else if (p.K == 2) gjsd_fwd_row<VEC, MODE, 2>(p, sm, ss, redP, redA);
  else if (p.K <= 4) gjsd_fwd_row<VEC, MODE, 4>(p, sm, ss, redP, redA);
  else gjsd_fwd_row<VEC, MODE, kGjsdMaxTeachers>(p, sm, ss, redP, redA);
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void gjsd_bwd_kernel(const GjsdParams p) {
  if (p.K == 1) gjsd_bwd_row<VEC, MODE, 1>(p);
  else if (p.K == 2) gjsd_bwd_row<VEC, MODE, 2>(p);
  else if (p.K <= 4) gjsd_bwd_row<VEC, MODE, 4>(p);
  else gjsd_bwd_row<VEC, MODE, kGjsdMaxTeachers>(p);
}

// ----------------------------------------------------------------------------------------------
static bool gjsd_vec(const GjsdParams& p) {
  auto al = [](const void* q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; };
  return p.V % 8 == 0 && p.s_ld % 8 == 0 && p.t_ld % 8 == 0 && p.t_sk % 8 == 0 && al(p.s) && al(p.t) &&
         (p.ds == nullptr || al(p.ds));
}

static int gjsd_mode(const GjsdParams& p) {
  return p.beta == 0.f ? GJSD_FWD_KL : p.beta == 1.f ? GJSD_REV_KL : GJSD_MIXED;
}

template <bool VEC>
static void gjsd_launch(const GjsdParams& p, bool bwd, hipStream_t st) {
  const unsigned grid = static_cast<unsigned>(p.N);
  switch (gjsd_mode(p)) {
    case GJSD_FWD_KL:
      if (bwd) gjsd_bwd_kernel<VEC, GJSD_FWD_KL><<<grid, 256, 0, st>>>(p);
      else gjsd_fwd_kernel<VEC, GJSD_FWD_KL><<<grid, 256, 0, st>>>(p);
      break;
    case GJSD_REV_KL:
      if (bwd) gjsd_bwd_kernel<VEC, GJSD_REV_KL><<<grid, 256, 0, st>>>(p);
      else gjsd_fwd_kernel<VEC, GJSD_REV_KL><<<grid, 256, 0, st>>>(p);
      break;
    default:
      if (bwd) gjsd_bwd_kernel<VEC, GJSD_MIXED><<<grid, 256, 0, st>>>(p);
      else gjsd_fwd_kernel<VEC, GJSD_MIXED><<<grid, 256, 0, st>>>(p);
  }
}

void launch_gjsd(const GjsdParams& p, bool bwd, hipStream_t st) {
  if (p.N == 0) return;
  if (gjsd_vec(p)) gjsd_launch<true>(p, bwd, st);
  else gjsd_launch<false>(p, bwd, st);
}

}  // namespace dla
