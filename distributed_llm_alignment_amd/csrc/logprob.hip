// Vocabulary-row reductions on bf16 logits.
//
// Reference semantics:
//   * `compute_logprobs` (src/training/train_dpo.py:31-39) and `sequence_logprob`
//     (src/training/train_rlhf.py:50-58): log_softmax -> gather(target) per token.
//   * HF ForCausalLMLoss (train_sft.py:145-146): token NLL with ignore_index=-100.
//   * Ensemble KL distillation (train_distill.py:127-144): sum_v p_bar (log p_bar - log q).
// The eager reference materialises fp32 log_softmax over [B,T,V] (1+ GB per micro-batch at
// V=128256). Here one 256-thread block streams a bf16 logits row once (16 B per lane,
// online max/sum in fp32), emitting only per-row scalars; the backward rewrites the SAME
// buffer in place as bf16 dlogits, which feeds the dH / dW GEMMs directly.
#include "common.h"

namespace dla {

// online (max, sum-exp) pair merge
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// The entropy twin carries u = sum_v exp(z_v - m) (z_v - m) next to (m, s): H = log s - u / s.
// Moving the reference point of (s, u) from m to mn >= m: s' = e s, u' = e (u + (m - mn) s) with
// e = exp(m - mn); an empty side (m = -inf, s = u = 0) stays 0 (the product would be 0 * inf).
__device__ __forceinline__ float ent_shift(float u, float s, float m, float mn, float e) {
  return m == -INFINITY ? 0.f : e * (u + (m - mn) * s);
}

// exp(d) is exactly 0 in fp32 below d = -104, so clamping the FACTOR d of a term exp(d) * d here
// changes no term and turns the 0 * inf of a -inf logit into 0.
#define ENT_DMIN (-128.f)

// (max, sum-exp, u) triple merge. logprob_entropy_fwd promises logprob_fwd's lse bit for bit, and
// lse_merge's `s * e1 + s2 * e2` leaves the rounding to the compiler's contraction: in
// logprob_fwd_kernel it is fma(s2, e2, round(s * e1)) at every merge but the last wave level
// (o == 1, sunk into the lane-0 branch as a packed multiply and an add: both products rounded).
// Next to the u arithmetic the same expression contracts differently, so here it is spelled out
// with contraction off (`fused` = every merge but o == 1); tests/test_entropy_gpu.py holds the
// two kernels' lse equal.
__device__ __forceinline__ void lse_merge_u(float& m, float& s, float& u, float m2, float s2, float u2,
                                            bool fused) {
#pragma clang fp contract(off)
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  const float e1 = __expf(m - mn), e2 = __expf(m2 - mn);
  u = ent_shift(u, s, m, mn, e1) + ent_shift(u2, s2, m2, mn, e2);
  const float a = s * e1;
  s = fused ? __builtin_fmaf(s2, e2, a) : a + s2 * e2;
  m = mn;
}

// x * i in the TEMP instantiations, x itself in the others.
template <bool TEMP>
__device__ __forceinline__ float scaled(float x, float i) {
#pragma clang fp contract(off)  // a product rounded on its own, never fused into the caller's sum
  if constexpr (TEMP) return x * i;
  return x;
}

// The (max, sum-exp) merge of the tempered kernels: the sums are of exp(i (z_v - m)) with m the max
// of the RAW logits, so moving the reference point scales the difference, exp((m - mn) * i). Spelled
// out with contraction off in the rounding logprob_fwd_kernel's lse_merge compiles to (see
// lse_merge_u), so that at i = 1 (a multiply by 1.0f is exact) the tempered kernels give the plain
// kernels' bits; tests/test_logprob_temperature_gpu.py holds them equal.
__device__ __forceinline__ void lse_merge_t(float& m, float& s, float m2, float s2, bool fused, float i) {
#pragma clang fp contract(off)
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  const float e1 = __expf((m - mn) * i), e2 = __expf((m2 - mn) * i);
  const float a = s * e1;
  s = fused ? __builtin_fmaf(s2, e2, a) : a + s2 * e2;
  m = mn;
}

// ent_shift at inverse temperature i: u is a sum of exp(d) d with d = i (z_v - m). The scaled
// difference is rounded on its own; the rest is ent_shift's expression, contraction as there.
__device__ __forceinline__ float ent_shift_t(float u, float s, float m, float mn, float e, float i) {
  return m == -INFINITY ? 0.f : e * (u + scaled<true>(m - mn, i) * s);
}

__device__ __forceinline__ void lse_merge_ut(float& m, float& s, float& u, float m2, float s2, float u2,
                                             bool fused, float i) {
#pragma clang fp contract(off)
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  const float e1 = __expf((m - mn) * i), e2 = __expf((m2 - mn) * i);
  u = ent_shift_t(u, s, m, mn, e1, i) + ent_shift_t(u2, s2, m2, mn, e2, i);
  const float a = s * e1;
  s = fused ? __builtin_fmaf(s2, e2, a) : a + s2 * e2;
  m = mn;
}

// ENT: also accumulate u (u_out). The (m, s) arithmetic rounds as with the flag off (contraction
// is switched off wherever s is updated next to u). With the flag on or off a -inf logit (a masked
// vocabulary entry) adds exactly 0, also while the lane's running max is still -inf; only a row
// of nothing but -inf has no lse.
// TEMP: the sums of softmax(it * z), it = 1 / temperature: m stays the max of the RAW logits, every
// exponent argument is a scaled DIFFERENCE, d = (z_v - m) * it, so s = sum_v exp(d) and
// u = sum_v exp(d) d. Contraction is off throughout and the merges are lse_merge_t / lse_merge_ut:
// at it = 1 this is the flag-off arithmetic bit for bit.
// MASK (TEMP && VEC && !ENT only): the row's packed keep mask km, one byte per 8-logit vector, bit j
// (LSB first) for lane value j; a cleared bit turns the fp32 value into -inf right after the
// conversion and nothing else changes, so the sums are those of the row with its dropped entries
// written as -inf, bit for bit. km == nullptr (a row without a mask) is the flag-off loop.
template <bool VEC, bool ENT = false, bool TEMP = false, bool MASK = false>
__device__ __forceinline__ void row_lse(const bf16_t* __restrict__ row, int V, float& m_out,
                                        float& s_out, float* u_out = nullptr, float it = 1.f,
                                        const uint8_t* __restrict__ km = nullptr) {
  static_assert(!MASK || (TEMP && VEC && !ENT), "the keep mask exists for the vectorised tempered kernels only");
  __shared__ float sm[4], ss[4], su[ENT ? 4 : 1];
  float m = -INFINITY, s = 0.f, u = 0.f;
  if constexpr (TEMP && VEC) {
#pragma clang fp contract(off)
    const int nv = V >> 3;
    for (int i = threadIdx.x; i < nv; i += 256) {
      bf16x8 a = load_bf16x8(row + i * 8);
      [[maybe_unused]] unsigned kb = 0xffu;
      if constexpr (MASK) {
        if (km) kb = km[i];
      }
      float x[8];
      float lm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x[j] = bf2f(a[j]);
        if constexpr (MASK) x[j] = (kb >> j) & 1u ? x[j] : -INFINITY;
        lm = fmaxf(lm, x[j]);
      }
      if (lm == -INFINITY) continue;
      if (lm > m) {
        const float e = __expf((m - lm) * it);
        if constexpr (ENT) u = ent_shift_t(u, s, m, lm, e, it);
        s *= e;
        m = lm;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = (x[j] - m) * it;
        const float e = __expf(d);
        s += e;
        if constexpr (ENT) u = __builtin_fmaf(e, fmaxf(d, ENT_DMIN), u);
      }
    }
  } else if constexpr (TEMP) {
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < V; i += 256) {
      const float x = bf2f(row[i]);
      if (x > m) {
        const float e = __expf((m - x) * it);
        if constexpr (ENT) u = ent_shift_t(u, s, m, x, e, it);
        s *= e;
        m = x;
      }
      const float d = (x - m) * it;
      const float e = x == -INFINITY ? 0.f : __expf(d);  // (d is NaN while m is still -inf)
      s += e;
      if constexpr (ENT) u = __builtin_fmaf(e, fmaxf(d, ENT_DMIN), u);
    }
  } else if constexpr (VEC) {
    const int nv = V >> 3;
    for (int i = threadIdx.x; i < nv; i += 256) {
      bf16x8 a = load_bf16x8(row + i * 8);
      float x[8];
      float lm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x[j] = bf2f(a[j]);
        lm = fmaxf(lm, x[j]);
      }
      // eight -inf logits add 0 (with m still -inf, x - m below would be NaN); m is finite below
      if (lm == -INFINITY) continue;
      if (lm > m) {
        if constexpr (ENT) {
#pragma clang fp contract(off)
          const float e = __expf(m - lm);
          u = ent_shift(u, s, m, lm, e);
          s *= e;
        } else {
          s *= __expf(m - lm);
        }
        m = lm;
      }
      if constexpr (ENT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma clang fp contract(off)
          const float d = x[j] - m;
          const float e = __expf(d);
          s += e;
          u = __builtin_fmaf(e, fmaxf(d, ENT_DMIN), u);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += __expf(x[j] - m);
      }
    }
  } else {
    for (int i = threadIdx.x; i < V; i += 256) {
      const float x = bf2f(row[i]);
      if constexpr (ENT) {
#pragma clang fp contract(off)
        if (x > m) {
          const float e = __expf(m - x);
          u = ent_shift(u, s, m, x, e);
          s *= e;
          m = x;
        }
        const float d = x - m;
        const float e = x == -INFINITY ? 0.f : __expf(d);  // (d is NaN while m is still -inf)
        s += e;
        u = __builtin_fmaf(e, fmaxf(d, ENT_DMIN), u);
      } else {
        if (x > m) {
          s *= __expf(m - x);
          m = x;
        }
        s += x == -INFINITY ? 0.f : __expf(x - m);  // (x - m is NaN while m is still -inf)
      }
    }
  }
  // wave merge
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    if constexpr (TEMP && ENT) {
      const float u2 = __shfl_xor(u, o, 64);
      lse_merge_ut(m, s, u, m2, s2, u2, o != 1, it);
    } else if constexpr (TEMP) {
      lse_merge_t(m, s, m2, s2, o != 1, it);
    } else if constexpr (ENT) {
      const float u2 = __shfl_xor(u, o, 64);
      lse_merge_u(m, s, u, m2, s2, u2, o != 1);
    } else {
      lse_merge(m, s, m2, s2);
    }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[w] = m;
    ss[w] = s;
    if constexpr (ENT) su[w] = u;
  }
  __syncthreads();
  m = sm[0];
  s = ss[0];
  if constexpr (ENT) u = su[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    if constexpr (TEMP && ENT) lse_merge_ut(m, s, u, sm[i], ss[i], su[i], true, it);
    else if constexpr (TEMP) lse_merge_t(m, s, sm[i], ss[i], true, it);
    else if constexpr (ENT) lse_merge_u(m, s, u, sm[i], ss[i], su[i], true);
    else lse_merge(m, s, sm[i], ss[i]);
  }
  m_out = m;
  s_out = s;
  if constexpr (ENT) *u_out = u;
}

// logp[r] = logits[r, tgt[r] - off] - lse[r] when this vocab shard [off, off+V) owns the
// target; rows with tgt < 0 (ignored) or a target owned by another shard -> logp 0. lse (of the
// local shard) is always written. off = 0, V = full vocab for the unsharded LM head.
// ENT: ent_out[r] = entropy of the local shard's softmax, from the same read of the row, for
// every row whatever its target.
// TEMP: the same of softmax(inv_temp * logits): lse = inv_temp m + log s, logp = inv_temp z_t - lse,
// ent = log s - u / s with s, u at the scaled differences (row_lse).
// MASK: row r reads row keep_rows[r] of keep [M, V / 8] (keep_rows[r] < 0: no mask, the flag-off
// arithmetic); lse and logp are over the kept set, logp = -inf for a target outside it.
template <bool VEC, bool ENT = false, bool TEMP = false, bool MASK = false>
__global__ __launch_bounds__(256) void logprob_fwd_kernel(const bf16_t* __restrict__ logits,
                                                           int64_t ld, int V, int64_t off,
                                                           const int64_t* __restrict__ tgt,
                                                           float* __restrict__ logp,
                                                           float* __restrict__ lse_out,
                                                           float* __restrict__ ent_out = nullptr,
                                                           float inv_temp = 1.f,
                                                           const uint8_t* __restrict__ keep = nullptr,
                                                           const int64_t* __restrict__ keep_rows = nullptr) {
  const int64_t r = blockIdx.x;
  const bf16_t* row = logits + r * ld;
  float m, s, u = 0.f;
  [[maybe_unused]] const uint8_t* km = nullptr;
  if constexpr (MASK) {
    const int64_t kr = keep_rows[r];  // row-uniform: one row per block
    if (kr >= 0) km = keep + kr * (V >> 3);
  }
  row_lse<VEC, ENT, TEMP, MASK>(row, V, m, s, &u, inv_temp, km);
  if (threadIdx.x == 0) {
    const float lse = scaled<TEMP>(m, inv_temp) + __logf(s);
    lse_out[r] = lse;
    if constexpr (ENT) ent_out[r] = __logf(s) - u / s;
    const int64_t t = tgt[r] - off;
    if constexpr (MASK) {
      float zt = 0.f;
      const bool own = tgt[r] >= 0 && t >= 0 && t < V;
      if (own) zt = (!km || ((km[t >> 3] >> (t & 7)) & 1u)) ? bf2f(row[t]) : -INFINITY;
      logp[r] = own ? scaled<TEMP>(zt, inv_temp) - lse : 0.f;
    } else {
      logp[r] = (tgt[r] >= 0 && t >= 0 && t < V) ? scaled<TEMP>(bf2f(row[t]), inv_temp) - lse : 0.f;
    }
  }
}

// In place: logits[r, v] <- g[r] * (1[v == tgt - off] - exp(logits - lse)), g = dL/dlogp[r];
// lse is the GLOBAL (all-shard) log-sum-exp. Ignored rows (tgt < 0) -> 0; z = -inf -> 0.
// ENT adds the entropy gradient, e = dL/dent[r] and H = the GLOBAL entropy ent_in[r]:
//   logits[r, v] <- g (1[v == t] - p) - e p (z - lse + H),  p = exp(z - lse);  z = -inf -> 0.
// TEMP (softmax(i z), i = inv_temp, y = i z): dz_v = i [ g (1[v == t] - p) - e p (y - lse + H) ],
// p = exp(y - lse), lse and H those of the tempered distribution. The callers fold i into the
// per-row scalars (g i, e i) and pass y = z i as `z`; the expressions below are then the same, and
// at i = 1 so are the bits.
template <bool ENT>
__device__ __forceinline__ float dlogit(float z, bool hit, float gr, float lse, float er, float H) {
#pragma clang fp contract(off)  // one rounding per operation in every kernel that inlines this
  const float p = __expf(z - lse);
  const float d = gr * ((hit ? 1.f : 0.f) - p);
  if constexpr (!ENT) return z == -INFINITY ? 0.f : d;  // (also when the target is the -inf logit)
  return z == -INFINITY ? 0.f : d - er * p * (z - lse + H);
}

// MASK (VEC && TEMP && !ENT): as in the forward; a dropped entry is a -inf logit, so it gets exactly 0.
template <bool VEC, bool ENT = false, bool TEMP = false, bool MASK = false>
__global__ __launch_bounds__(256) void logprob_bwd_kernel(bf16_t* __restrict__ logits, int64_t ld,
                                                           int V, int64_t off,
                                                           const int64_t* __restrict__ tgt,
                                                           const float* __restrict__ lse_in,
                                                           const float* __restrict__ g,
                                                           const float* __restrict__ ent_in = nullptr,
                                                           const float* __restrict__ ge = nullptr,
                                                           float inv_temp = 1.f,
                                                           const uint8_t* __restrict__ keep = nullptr,
                                                           const int64_t* __restrict__ keep_rows = nullptr) {
  static_assert(!MASK || (TEMP && VEC && !ENT), "the keep mask exists for the vectorised tempered kernels only");
  const int64_t r = blockIdx.x;
  bf16_t* row = logits + r * ld;
  [[maybe_unused]] const uint8_t* km = nullptr;
  if constexpr (MASK) {
    const int64_t kr = keep_rows[r];  // row-uniform: one row per block
    if (kr >= 0) km = keep + kr * (V >> 3);
  }
  const int64_t t = tgt[r] - off;
  const float gr = scaled<TEMP>(tgt[r] >= 0 ? g[r] : 0.f, inv_temp);
  const float lse = lse_in[r];
  float er = 0.f, H = 0.f;
  if constexpr (ENT) {
    er = scaled<TEMP>(tgt[r] >= 0 ? ge[r] : 0.f, inv_temp);
    H = ent_in[r];
  }
  if constexpr (VEC) {
    const int nv = V >> 3;
    for (int i = threadIdx.x; i < nv; i += 256) {
      bf16x8 a = load_bf16x8(row + i * 8), o;
      [[maybe_unused]] unsigned kb = 0xffu;
      if constexpr (MASK) {
        if (km) kb = km[i];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = i * 8 + j;
        float x = bf2f(a[j]);
        if constexpr (MASK) x = (kb >> j) & 1u ? x : -INFINITY;
        o[j] = f2bf(dlogit<ENT>(scaled<TEMP>(x, inv_temp), v == t, gr, lse, er, H));
      }
      store_bf16x8(row + i * 8, o);
    }
  } else {
    for (int v = threadIdx.x; v < V; v += 256)
      row[v] = f2bf(dlogit<ENT>(scaled<TEMP>(bf2f(row[v]), inv_temp), v == t, gr, lse, er, H));
  }
}

// The same gradient with a transposed second output (the LM head's TN weight-gradient operand):
// dlogits written in place AND dlogitsT [V, rows] (ld = rows), from one read of the logits, in
// place of the in-place kernel + a separate transpose pass (which reads and writes the [rows, V]
// gradient once more: 815 us per Llama-3-8B DPO micro-batch, profiles/r6_*). Each lane owns an
// 8 x 8 block (8 rows x 8 vocab columns) and transposes it in registers (tr8_bf16); a wave covers
// 64 rows x 64 columns; grid (ceil(V / 256), rows / 64); rows % 8 == 0, V % 8 == 0, ld % 8 == 0.
// ENT: the entropy gradient too (dlogit<true>); two more per-row scalars live inside the unrolled
// row loop, the 16 bf16x8 vectors per lane are unchanged.
// MASK: the lane loads one mask byte for each of its 8 rows (byte c / 8 of row keep_rows[r + i]).
template <bool ENT = false, bool TEMP = false, bool MASK = false>
__global__ __launch_bounds__(256) void logprob_bwd_t_kernel(bf16_t* __restrict__ logits, int64_t ld, int V,
                                                             int64_t off, const int64_t* __restrict__ tgt,
                                                             const float* __restrict__ lse_in,
                                                             const float* __restrict__ g,
                                                             bf16_t* __restrict__ outT, int64_t rows,
                                                             const float* __restrict__ ent_in = nullptr,
                                                             const float* __restrict__ ge = nullptr,
                                                             float inv_temp = 1.f,
                                                             const uint8_t* __restrict__ keep = nullptr,
                                                             const int64_t* __restrict__ keep_rows = nullptr) {
  static_assert(!MASK || (TEMP && !ENT), "the keep mask exists for the tempered kernels only");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = static_cast<int64_t>(blockIdx.y) * 64 + (lane >> 3) * 8;
  const int c = blockIdx.x * 256 + w * 64 + (lane & 7) * 8;
  if (r >= rows || c >= V) return;
  bf16x8 a[8], o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = load_bf16x8(logits + (r + i) * ld + c);
  [[maybe_unused]] unsigned kb[8];
  if constexpr (MASK) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t kr = keep_rows[r + i];
      kb[i] = kr >= 0 ? keep[kr * (V >> 3) + (c >> 3)] : 0xffu;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t t = tgt[r + i] - off;
    const float gr = scaled<TEMP>(tgt[r + i] >= 0 ? g[r + i] : 0.f, inv_temp);
    const float lse = lse_in[r + i];
    float er = 0.f, H = 0.f;
    if constexpr (ENT) {
      er = scaled<TEMP>(tgt[r + i] >= 0 ? ge[r + i] : 0.f, inv_temp);
      H = ent_in[r + i];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = bf2f(a[i][j]);
      if constexpr (MASK) x = (kb[i] >> j) & 1u ? x : -INFINITY;
      o[i][j] = f2bf(dlogit<ENT>(scaled<TEMP>(x, inv_temp), c + j == t, gr, lse, er, H));
    }
    store_bf16x8(logits + (r + i) * ld + c, o[i]);
  }
  bf16x8 tt[8];
  tr8_bf16(o, tt);
#pragma unroll
  for (int j = 0; j < 8; ++j) store_bf16x8(outT + static_cast<int64_t>(c + j) * rows + r, tt[j]);
}

// Ensemble forward-KL distillation, one row per block:
//   p_bar = mean_k softmax(teacher_k), q = softmax(student)
//   kl[r] = sum_v p_bar (log p_bar - log q)
//   (optionally, in place) student_logits[r,:] <- g[r] * (q - p_bar)   (d kl / d z_student)
// Teacher rows are read with their own precomputed lse (t_lse[k, r]).
template <bool WRITE_GRAD>
__global__ __launch_bounds__(256) void ensemble_kl_kernel(bf16_t* __restrict__ s_logits,
                                                           const bf16_t* __restrict__ t_logits,
                                                           int64_t ld, int64_t t_stride, int K,
                                                           int V, const float* __restrict__ s_lse,
                                                           const float* __restrict__ t_lse,
                                                           int64_t rows, const float* __restrict__ g,
                                                           float* __restrict__ kl_out) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  bf16_t* srow = s_logits + r * ld;
  const float sl = s_lse[r];
  const float gr = WRITE_GRAD ? g[r] : 0.f;
  float acc = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) {
    float pbar = 0.f;
    for (int k = 0; k < K; ++k)
      pbar += __expf(bf2f(t_logits[k * t_stride + r * ld + v]) - t_lse[k * rows + r]);
    pbar /= K;
    const float lq = bf2f(srow[v]) - sl;
    if (pbar > 0.f) acc += pbar * (__logf(pbar) - lq);
    if constexpr (WRITE_GRAD) srow[v] = f2bf(gr * (__expf(lq) - pbar));
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) kl_out[r] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void row_lse_kernel(const bf16_t* __restrict__ logits, int64_t ld,
                                                       int V, float* __restrict__ lse_out) {
  const int64_t r = blockIdx.x;
  float m, s;
  row_lse<false>(logits + r * ld, V, m, s);
  if (threadIdx.x == 0) lse_out[r] = m + __logf(s);
}

// ----------------------------------------------------------------------------------------------
void launch_logprob_fwd(const bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                        const int64_t* tgt, float* logp, float* lse, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec) logprob_fwd_kernel<true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse);
  else logprob_fwd_kernel<false><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse);
}

void launch_logprob_bwd(bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                        const int64_t* tgt, const float* lse, const float* g, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec) logprob_bwd_kernel<true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g);
  else logprob_bwd_kernel<false><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g);
}

void launch_logprob_entropy_fwd(const bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                                const int64_t* tgt, float* logp, float* lse, float* ent, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec) logprob_fwd_kernel<true, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse, ent);
  else logprob_fwd_kernel<false, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse, ent);
}

void launch_logprob_entropy_bwd(bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                                const int64_t* tgt, const float* lse, const float* ent, const float* g,
                                const float* ge, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec) logprob_bwd_kernel<true, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, ent, ge);
  else logprob_bwd_kernel<false, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, ent, ge);
}

bool launch_logprob_entropy_bwd_t(bf16_t* logits, int64_t ld, int V, int64_t rows, int64_t off,
                                  const int64_t* tgt, const float* lse, const float* ent, const float* g,
                                  const float* ge, bf16_t* outT, hipStream_t st) {
  if (rows % 8 != 0 || V % 8 != 0 || ld % 8 != 0) return false;
  if (rows == 0) return true;
  const dim3 grid((V + 255) / 256, static_cast<unsigned>((rows + 63) / 64));
  logprob_bwd_t_kernel<true><<<grid, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, outT, rows, ent, ge);
  return true;
}

bool launch_logprob_bwd_t(bf16_t* logits, int64_t ld, int V, int64_t rows, int64_t off, const int64_t* tgt,
                          const float* lse, const float* g, bf16_t* outT, hipStream_t st) {
  if (rows % 8 != 0 || V % 8 != 0 || ld % 8 != 0) return false;
  if (rows == 0) return true;
  const dim3 grid((V + 255) / 256, static_cast<unsigned>((rows + 63) / 64));
  logprob_bwd_t_kernel<false><<<grid, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, outT, rows);
  return true;
}

// The tempered twins (TEMP instantiations): the same launches with inv_temp = 1 / temperature.
void launch_logprob_fwd_temp(const bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                             const int64_t* tgt, float* logp, float* lse, float inv_temp, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec)
    logprob_fwd_kernel<true, false, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse, nullptr,
                                                                inv_temp);
  else
    logprob_fwd_kernel<false, false, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse, nullptr,
                                                                 inv_temp);
}

void launch_logprob_bwd_temp(bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows, const int64_t* tgt,
                             const float* lse, const float* g, float inv_temp, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec)
    logprob_bwd_kernel<true, false, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, nullptr,
                                                                nullptr, inv_temp);
  else
    logprob_bwd_kernel<false, false, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, nullptr,
                                                                 nullptr, inv_temp);
}

void launch_logprob_entropy_fwd_temp(const bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                                     const int64_t* tgt, float* logp, float* lse, float* ent, float inv_temp,
                                     hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec)
    logprob_fwd_kernel<true, true, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse, ent,
                                                               inv_temp);
  else
    logprob_fwd_kernel<false, true, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, logp, lse, ent,
                                                                inv_temp);
}

void launch_logprob_entropy_bwd_temp(bf16_t* logits, int64_t ld, int V, int64_t off, int64_t rows,
                                     const int64_t* tgt, const float* lse, const float* ent, const float* g,
                                     const float* ge, float inv_temp, hipStream_t st) {
  if (rows == 0) return;
  const bool vec = (V % 8 == 0) && (ld % 8 == 0);
  if (vec)
    logprob_bwd_kernel<true, true, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, ent, ge,
                                                               inv_temp);
  else
    logprob_bwd_kernel<false, true, true><<<rows, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, ent, ge,
                                                                inv_temp);
}

bool launch_logprob_entropy_bwd_t_temp(bf16_t* logits, int64_t ld, int V, int64_t rows, int64_t off,
                                       const int64_t* tgt, const float* lse, const float* ent, const float* g,
                                       const float* ge, bf16_t* outT, float inv_temp, hipStream_t st) {
  if (rows % 8 != 0 || V % 8 != 0 || ld % 8 != 0) return false;
  if (rows == 0) return true;
  const dim3 grid((V + 255) / 256, static_cast<unsigned>((rows + 63) / 64));
  logprob_bwd_t_kernel<true, true><<<grid, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, outT, rows, ent, ge,
                                                         inv_temp);
  return true;
}

bool launch_logprob_bwd_t_temp(bf16_t* logits, int64_t ld, int V, int64_t rows, int64_t off, const int64_t* tgt,
                               const float* lse, const float* g, bf16_t* outT, float inv_temp, hipStream_t st) {
  if (rows % 8 != 0 || V % 8 != 0 || ld % 8 != 0) return false;
  if (rows == 0) return true;
  const dim3 grid((V + 255) / 256, static_cast<unsigned>((rows + 63) / 64));
  logprob_bwd_t_kernel<false, true><<<grid, 256, 0, st>>>(logits, ld, V, off, tgt, lse, g, outT, rows, nullptr,
                                                          nullptr, inv_temp);
  return true;
}

// The kept-set twins (MASK instantiations) of the tempered launches: keep uint8 [M, V / 8], keep_rows
// int64 [rows] (< 0: no mask). V % 8 == 0 and ld % 8 == 0 are the caller's to check; no vocab shard.
void launch_logprob_fwd_keep(const bf16_t* logits, int64_t ld, int V, int64_t rows, const int64_t* tgt,
                             float* logp, float* lse, const uint8_t* keep, const int64_t* keep_rows,
                             float inv_temp, hipStream_t st) {
  if (rows == 0) return;
  logprob_fwd_kernel<true, false, true, true><<<rows, 256, 0, st>>>(logits, ld, V, 0, tgt, logp, lse, nullptr,
                                                                    inv_temp, keep, keep_rows);
}

void launch_logprob_bwd_keep(bf16_t* logits, int64_t ld, int V, int64_t rows, const int64_t* tgt,
                             const float* lse, const float* g, const uint8_t* keep, const int64_t* keep_rows,
                             float inv_temp, hipStream_t st) {
  if (rows == 0) return;
  logprob_bwd_kernel<true, false, true, true><<<rows, 256, 0, st>>>(logits, ld, V, 0, tgt, lse, g, nullptr,
                                                                    nullptr, inv_temp, keep, keep_rows);
}

bool launch_logprob_bwd_t_keep(bf16_t* logits, int64_t ld, int V, int64_t rows, const int64_t* tgt,
                               const float* lse, const float* g, bf16_t* outT, const uint8_t* keep,
                               const int64_t* keep_rows, float inv_temp, hipStream_t st) {
  if (rows % 8 != 0 || V % 8 != 0 || ld % 8 != 0) return false;
  if (rows == 0) return true;
  const dim3 grid((V + 255) / 256, static_cast<unsigned>((rows + 63) / 64));
  logprob_bwd_t_kernel<false, true, true><<<grid, 256, 0, st>>>(logits, ld, V, 0, tgt, lse, g, outT, rows,
                                                                nullptr, nullptr, inv_temp, keep, keep_rows);
  return true;
}

void launch_row_lse(const bf16_t* logits, int64_t ld, int V, int64_t rows, float* lse,
                    hipStream_t st) {
  if (rows == 0) return;
  row_lse_kernel<<<rows, 256, 0, st>>>(logits, ld, V, lse);
}

void launch_ensemble_kl(bf16_t* s_logits, const bf16_t* t_logits, int64_t ld, int64_t t_stride,
                        int K, int V, const float* s_lse, const float* t_lse, int64_t rows,
                        const float* g, float* kl, bool write_grad, hipStream_t st) {
  if (rows == 0) return;
  if (write_grad)
    ensemble_kl_kernel<true><<<rows, 256, 0, st>>>(s_logits, t_logits, ld, t_stride, K, V, s_lse,
                                                   t_lse, rows, g, kl);
  else
    ensemble_kl_kernel<false><<<rows, 256, 0, st>>>(s_logits, t_logits, ld, t_stride, K, V, s_lse,
                                                    t_lse, rows, g, kl);
}

}  // namespace dla
