// Sequence-level objective kernels (SURVEY K11 reduction, K12, K14, K15).
//
//   seq_reduce      : masked per-sequence sum / count of token log-probs
//                     (the `(gathered * mask).sum(1) / mask.sum(1).clamp(min=1)` tail of
//                      src/training/train_dpo.py:38 and train_rlhf.py:57)
//   dpo_loss        : -logsigmoid(beta*((pc-pr)-(rc-rr))).mean()   train_dpo.py:42-44
//                     + fused backward coefficients, rewards, margin and accuracy outputs
//   pairwise_loss   : -logsigmoid(sc - sr).mean()                   src/models/reward_model.py:67-68
//   kl_penalty_pg   : kl = lp - lr; r' = r - c*kl; A = r' - mean(r'); loss = -mean(A*lp)
//                                                                   train_rlhf.py:149-153
//   gae / ppo_policy_loss / ppo_value_loss : token-level actor-critic PPO (below)
//   group_advantages / grpo_loss : critic-free group-relative policy optimisation (below)
//   rollout_is_weights / grpo_loss_w / ppo_policy_loss_w : truncated importance weights for the
//                     rollout engine / trainer mismatch and the surrogates that take them (below)
//   grpo_loss_seq   : GSPO, the GRPO loss with the length-normalised sequence-level ratio (below)
// Batch dimensions here are small (pairs per micro-batch), so each loss is a single
// 256-thread block; the point is fusing fwd+bwd+metrics into one launch with no host sync.
#include "common.h"

namespace dla {

// one block per sequence: out_sum[s] = sum_t lp[s,t]*m[s,t]; out_cnt[s] = sum_t m[s,t]
__global__ __launch_bounds__(256) void seq_reduce_kernel(const float* __restrict__ lp,
                                                          const float* __restrict__ mask, int T,
                                                          float* __restrict__ out_sum,
                                                          float* __restrict__ out_cnt) {
  __shared__ float scratch[4];
  const int64_t s = blockIdx.x;
  float a = 0.f, c = 0.f;
  for (int t = threadIdx.x; t < T; t += 256) {
    const float m = mask[s * T + t];
    a += lp[s * T + t] * m;
    c += m;
  }
  a = block_sum<256>(a, scratch);
  c = block_sum<256>(c, scratch);
  if (threadIdx.x == 0) {
    out_sum[s] = a;
    out_cnt[s] = c;
  }
}

// g_tok[s,t] = coef[s] * mask[s,t] / (mean ? max(cnt[s],1) : 1)
__global__ __launch_bounds__(256) void seq_expand_grad_kernel(const float* __restrict__ coef,
                                                               const float* __restrict__ mask,
                                                               const float* __restrict__ cnt,
                                                               int T, int S, bool mean,
                                                               float* __restrict__ g) {
  const int64_t n = static_cast<int64_t>(S) * T;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t s = i / T;
    const float d = mean ? fmaxf(cnt[s], 1.f) : 1.f;
    g[i] = coef[s] * mask[i] / d;
  }
}

// pol/ref: [2B] seq log-probs, chosen = [0,B), rejected = [B,2B).
// outputs: loss[0]; metrics[0..3] = (mean chosen reward, mean rejected reward, accuracy, margin)
// dpol[2B] = dloss/dpol (already includes 1/B), rewards_out[2B] = beta*(pol-ref).
__global__ __launch_bounds__(256) void dpo_loss_kernel(const float* __restrict__ pol,
                                                        const float* __restrict__ ref, int B,
                                                        float beta, float label_smoothing,
                                                        float* __restrict__ loss,
                                                        float* __restrict__ dpol,
                                                        float* __restrict__ rewards_out,
                                                        float* __restrict__ metrics) {
  __shared__ float scratch[4];
  float l = 0.f, rc = 0.f, rr = 0.f, acc = 0.f, mg = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float c_r = beta * (pol[i] - ref[i]);
    const float r_r = beta * (pol[B + i] - ref[B + i]);
    const float z = c_r - r_r;  // beta * ((pc - pr) - (rc - rr))
    // loss = -(1-ls)*logsig(z) - ls*logsig(-z)
    l += -(1.f - label_smoothing) * log_sigmoid(z) - label_smoothing * log_sigmoid(-z);
    // dloss/dz = -(1-ls)*sig(-z) + ls*sig(z)
    const float dz = (-(1.f - label_smoothing) * sigmoidf_(-z) + label_smoothing * sigmoidf_(z)) / B;
    dpol[i] = dz * beta;
    dpol[B + i] = -dz * beta;
    rewards_out[i] = c_r;
    rewards_out[B + i] = r_r;
    rc += c_r;
    rr += r_r;
    acc += (c_r > r_r) ? 1.f : 0.f;
    mg += z;
  }
  l = block_sum<256>(l, scratch);
  rc = block_sum<256>(rc, scratch);
  rr = block_sum<256>(rr, scratch);
  acc = block_sum<256>(acc, scratch);
  mg = block_sum<256>(mg, scratch);
  if (threadIdx.x == 0) {
    loss[0] = l / B;
    metrics[0] = rc / B;
    metrics[1] = rr / B;
    metrics[2] = acc / B;
    metrics[3] = mg / B;
  }
}

// scores: [2B] (chosen, rejected). loss = -mean logsig(sc - sr); dscores; metrics = accuracy.
__global__ __launch_bounds__(256) void pairwise_loss_kernel(const float* __restrict__ sc,
                                                             const float* __restrict__ sr, int B,
                                                             float* __restrict__ loss,
                                                             float* __restrict__ dsc,
                                                             float* __restrict__ dsr,
                                                             float* __restrict__ acc_out) {
  __shared__ float scratch[4];
  float l = 0.f, acc = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float z = sc[i] - sr[i];
    l += -log_sigmoid(z);
    const float dz = -sigmoidf_(-z) / B;
    dsc[i] = dz;
    dsr[i] = -dz;
    acc += z > 0.f ? 1.f : 0.f;
  }
  l = block_sum<256>(l, scratch);
  acc = block_sum<256>(acc, scratch);
  if (threadIdx.x == 0) {
    loss[0] = l / B;
    acc_out[0] = acc / B;
  }
}

// REINFORCE with KL-shaped reward and mean baseline (train_rlhf.py:149-153).
// out: loss[0], kl_mean[0]; dlp[n] = dloss/dlp = -A[i]/n (A is stop-gradient).
__global__ __launch_bounds__(256) void kl_penalty_pg_kernel(const float* __restrict__ lp,
                                                             const float* __restrict__ lr,
                                                             const float* __restrict__ reward,
                                                             int n, float kl_coef,
                                                             float* __restrict__ loss,
                                                             float* __restrict__ kl_mean,
                                                             float* __restrict__ dlp,
                                                             float* __restrict__ adv_out) {
  __shared__ float scratch[4];
  float rsum = 0.f, ksum = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float kl = lp[i] - lr[i];
    rsum += reward[i] - kl_coef * kl;
    ksum += kl;
  }
  rsum = block_sum<256>(rsum, scratch);
  ksum = block_sum<256>(ksum, scratch);
  const float rmean = rsum / n;
  float l = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float kl = lp[i] - lr[i];
    const float a = reward[i] - kl_coef * kl - rmean;
    adv_out[i] = a;
    dlp[i] = -a / n;
    l += -a * lp[i];
  }
  l = block_sum<256>(l, scratch);
  if (threadIdx.x == 0) {
    loss[0] = l / n;
    kl_mean[0] = ksum / n;
  }
}

// ==============================================================================================
// PPO (actor-critic) token objectives: the north-star "PPO RLHF (actor + critic + reward)"
// configuration. The reference's train_rlhf.py:149-153 is the sequence-level REINFORCE special
// case above (kl_penalty_pg); these run over [S, T] token grids.
// ==============================================================================================

// Generalised advantage estimation, one wave per sequence:
//   A_t = m_t * (delta_t + gamma*lam*m_{t+1} * A_{t+1}),  delta_t = r_t + gamma*m_{t+1}*V_{t+1} - V_t
// is the affine reverse recurrence x_t = a_t + c_t x_{t+1}. Lane l owns the contiguous segment
// [l*L, (l+1)*L) (L = ceil(T/64)): pass 1 composes the segment's map x_{t0} = A + C x_{t1}, a
// log2(64)-step shuffle scan composes the maps of lanes l..63 (so every lane learns the x
// entering its segment from the right), pass 2 re-walks the segment writing A_t and the
// returns R_t = A_t + V_t. No serial 1-thread-per-sequence loop over T.
__global__ __launch_bounds__(64) void gae_kernel(const float* __restrict__ r, const float* __restrict__ v,
                                                 const float* __restrict__ m, int T, float gamma,
                                                 float lam, float* __restrict__ adv,
                                                 float* __restrict__ ret) {
  const int lane = threadIdx.x;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * T;
  const int L = (T + 63) / 64;
  const int t0 = min(T, lane * L), t1 = min(T, t0 + L);
  auto coef = [&](int t, float& a, float& c) {
    const float mt = m[base + t];
    const float mn = t + 1 < T ? m[base + t + 1] : 0.f;
    const float vn = t + 1 < T ? v[base + t + 1] : 0.f;
    a = mt * (r[base + t] + gamma * mn * vn - v[base + t]);
    c = mt * gamma * lam * mn;
  };
  float A = 0.f, C = 1.f;  // identity map for an empty segment
  for (int t = t1 - 1; t >= t0; --t) {
    float a, c;
    coef(t, a, c);
    A = a + c * A;
    C = c * C;
  }
  // (SA, SC): composition of the maps of lanes l .. min(63, l + 2^k - 1)
  float SA = A, SC = C;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float na = __shfl_down(SA, off, 64), nc = __shfl_down(SC, off, 64);
    if (lane + off < 64) {
      SA = SA + SC * na;
      SC = SC * nc;
    }
  }
  float x = __shfl_down(SA, 1, 64);  // x entering this segment from the right (x_T = 0)
  if (lane == 63) x = 0.f;
  for (int t = t1 - 1; t >= t0; --t) {
    float a, c;
    coef(t, a, c);
    x = a + c * x;
    adv[base + t] = x;
    ret[base + t] = x + v[base + t];
  }
}

// The product of a detached importance weight with a policy-gradient term, rounded on its own: it
// is never contracted into a neighbouring add, so w = 1 (1.0f * x is exact) leaves every weighted
// kernel below bitwise equal to its unweighted instantiation.
__device__ __forceinline__ float is_mul(float w, float x) {
#pragma clang fp contract(off)
  return w * x;
}

// Clipped surrogate over masked tokens (fwd + bwd in one launch):
//   rho = exp(lp - lp_old); loss = sum m * max(-A rho, -A clip(rho, 1-eps, 1+eps)) / sum m
//   dlp = m * (-A rho if the unclipped branch is the max else 0) / sum m
//   metrics: [0] clip fraction, [1] approx KL  mean((rho - 1) - log rho), [2] token count
// W (ppo_policy_loss_w): a detached per-token weight w multiplies the surrogate and its gradient
// (truncated importance sampling); the divisor stays sum m and the metrics stay unweighted.
template <bool W>
__global__ __launch_bounds__(1024) void ppo_policy_loss_kernel(
    const float* __restrict__ lp, const float* __restrict__ old, const float* __restrict__ adv,
    const float* __restrict__ m, int64_t n, float eps, float* __restrict__ loss,
    float* __restrict__ dlp, float* __restrict__ metrics, const float* __restrict__ w) {
  __shared__ float scratch[16];
  float cnt = 0.f, l = 0.f, cf = 0.f, kl = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float mi = m[i];
    const float d = lp[i] - old[i];
    const float rho = __expf(d), a = adv[i];
    const float l1 = -a * rho, l2 = -a * fminf(fmaxf(rho, 1.f - eps), 1.f + eps);
    if constexpr (W) {
      l += mi * is_mul(w[i], fmaxf(l1, l2));
    } else {
      l += mi * fmaxf(l1, l2);
    }
    cnt += mi;
    cf += mi * (fabsf(rho - 1.f) > eps ? 1.f : 0.f);
    kl += mi * ((rho - 1.f) - d);
  }
  cnt = block_sum<1024>(cnt, scratch);
  l = block_sum<1024>(l, scratch);
  cf = block_sum<1024>(cf, scratch);
  kl = block_sum<1024>(kl, scratch);
  const float inv = 1.f / fmaxf(cnt, 1.f);
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float d = lp[i] - old[i];
    const float rho = __expf(d), a = adv[i];
    const float l1 = -a * rho, l2 = -a * fminf(fmaxf(rho, 1.f - eps), 1.f + eps);
    if constexpr (W) {
      dlp[i] = l1 >= l2 ? m[i] * w[i] * l1 * inv : 0.f;
    } else {
      dlp[i] = l1 >= l2 ? m[i] * l1 * inv : 0.f;
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = l * inv;
    metrics[0] = cf * inv;
    metrics[1] = kl * inv;
    metrics[2] = cnt;
  }
}

// Clipped value loss: 0.5 * sum m * max((V - R)^2, (Vc - R)^2) / sum m,
// Vc = V_old + clamp(V - V_old, -c, c); dV through whichever branch is the max.
__global__ __launch_bounds__(1024) void ppo_value_loss_kernel(
    const float* __restrict__ val, const float* __restrict__ old, const float* __restrict__ ret,
    const float* __restrict__ m, int64_t n, float clip, float* __restrict__ loss,
    float* __restrict__ dval) {
  __shared__ float scratch[16];
  float cnt = 0.f, l = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float mi = m[i], v = val[i], o = old[i], R = ret[i];
    const float vc = o + fminf(fmaxf(v - o, -clip), clip);
    l += mi * 0.5f * fmaxf((v - R) * (v - R), (vc - R) * (vc - R));
    cnt += mi;
  }
  cnt = block_sum<1024>(cnt, scratch);
  l = block_sum<1024>(l, scratch);
  const float inv = 1.f / fmaxf(cnt, 1.f);
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float mi = m[i], v = val[i], o = old[i], R = ret[i];
    const float dv = v - o;
    const float vc = o + fminf(fmaxf(dv, -clip), clip);
    const float u1 = (v - R) * (v - R), u2 = (vc - R) * (vc - R);
    const float g = u1 >= u2 ? (v - R) : (fabsf(dv) <= clip ? (vc - R) : 0.f);
    dval[i] = mi * g * inv;
  }
  if (threadIdx.x == 0) loss[0] = l * inv;
}

// ==============================================================================================
// GRPO (critic-free, group-relative): group advantages + token-level clipped surrogate with a k3
// reference-KL term and the GRPO / DAPO / Dr. GRPO normalisations.
// ==============================================================================================

// Advantage of a rollout = its reward standardised inside its group of G samples of one prompt.
// One wave per group (G <= 64 lives in the wave, larger groups loop); a constant-reward group
// gives exactly 0 (and sd = 0), never NaN.
//   mu = mean, sd = population std;  adv = (r - mu) / (sd + eps)  or  r - mu  (scale_std = 0)
__global__ __launch_bounds__(64) void group_advantages_kernel(const float* __restrict__ r, int G,
                                                              int scale_std, float eps,
                                                              float* __restrict__ adv,
                                                              float* __restrict__ sd_out) {
  const int lane = threadIdx.x;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * G;
  float s = 0.f, hi = -INFINITY, lo = INFINITY;
  for (int g = lane; g < G; g += 64) {
    const float x = r[base + g];
    s += x;
    hi = fmaxf(hi, x);
    lo = fminf(lo, x);
  }
  s = wave_sum(s);
  hi = wave_max(hi);
  lo = -wave_max(-lo);
  const float mu = s / G;
  float q = 0.f;
  for (int g = lane; g < G; g += 64) {
    const float c = r[base + g] - mu;
    q += c * c;
  }
  q = wave_sum(q);
  const bool constant = hi == lo;
  const float sd = constant ? 0.f : sqrtf(q / G);
  const float inv = scale_std ? 1.f / (sd + eps) : 1.f;
  for (int g = lane; g < G; g += 64)
    adv[base + g] = constant ? 0.f : (r[base + g] - mu) * inv;
  if (lane == 0) sd_out[blockIdx.x] = sd;
}

// GRPO loss, launch 1 of 2: one workgroup per sequence reduces its row of the [S, T] grids to
// five partials part[k * S + s]: token count, sum m*per, sum m*[rho outside the clip range],
// sum m*((rho - 1) - d), sum m*k3.
//   d = lp - old; rho = exp(d); pg = max(-A rho, -A clamp(rho, lo, hi)), lo = 1 - clip_low, hi = 1 + clip_high
//   dr = ref - lp; k3 = exp(dr) - dr - 1; per = pg + beta * k3          (A = adv[s], per rollout)
// W (grpo_loss_w): a detached per-token weight w [S, T] multiplies pg and its gradient only
// (truncated importance sampling): per = w pg + beta k3. Divisors and metrics stay unweighted.
struct GrpoTok {
  float per, l1, l2, rho, d, edr, k3;
};
template <bool W>
__device__ __forceinline__ GrpoTok grpo_token(float lp, float old, float ref, float a, float lo,
                                              float hi, float beta, float w) {
  GrpoTok t;
  t.d = lp - old;
  t.rho = expf(t.d);
  t.l1 = -a * t.rho;
  t.l2 = -a * fminf(fmaxf(t.rho, lo), hi);
  const float dr = ref - lp;
  t.edr = expf(dr);
  t.k3 = t.edr - dr - 1.f;
  if constexpr (W) {
    // the unweighted instantiation compiles its sum to fma(beta, k3, pg): the same fma here
    t.per = fmaf(beta, t.k3, is_mul(w, fmaxf(t.l1, t.l2)));
  } else {
    t.per = fmaxf(t.l1, t.l2) + beta * t.k3;
  }
  return t;
}

constexpr int kGrpoThreads = 256;

// SEQ (grpo_loss_seq, GSPO): the ratio is the row's length-normalised one and every action token of
// the row carries the row's surrogate; the k3 term stays per token.
//   l_s = sum_{t: m != 0} d / max(c_s, 1); sr_s = exp(l_s)  (c_s = 0: l_s = 0, sr_s = 1)
//   pg_s = max(-A sr_s, -A clamp(sr_s, lo, hi)); per = w pg_s + beta * k3
// The partials keep their meaning with rho -> sr_s (the two metric sums are c_s times the row's
// value) and two more rows follow them: part[5 S + s] = l_s, which launch 2 reads back so that
// both launches decide the clip on the same bits, and with W part[6 S + s] = sum m w. Entries
// outside the mask are never read into a sum: NaN or junk there reaches no output.
template <bool W, bool SEQ = false>
__global__ __launch_bounds__(kGrpoThreads) void grpo_partials_kernel(
    const float* __restrict__ lp, const float* __restrict__ old, const float* __restrict__ ref,
    const float* __restrict__ adv, const float* __restrict__ m, int S, int T, float lo, float hi,
    float beta, float* __restrict__ part, const float* __restrict__ w) {
  __shared__ float scratch[kGrpoThreads / 64];
  const int s = blockIdx.x;
  const int64_t base = static_cast<int64_t>(s) * T;
  const float a = adv[s];
  if constexpr (SEQ) {
    float dsum = 0.f, c = 0.f;
    for (int t = threadIdx.x; t < T; t += kGrpoThreads) {
      const float mi = m[base + t];
      if (mi != 0.f) {
        dsum += lp[base + t] - old[base + t];
        c += mi;
      }
    }
    dsum = block_sum<kGrpoThreads>(dsum, scratch);
    c = block_sum<kGrpoThreads>(c, scratch);
    const float ls = dsum / fmaxf(c, 1.f);
    const float sr = expf(ls);
    // A = 0 with sr = inf: l1 is NaN and fmaxf returns l2, as in grpo_token
    const float pg = fmaxf(-a * sr, -a * fminf(fmaxf(sr, lo), hi));
    float l = 0.f, klr = 0.f, sw = 0.f;
    for (int t = threadIdx.x; t < T; t += kGrpoThreads) {
      const float mi = m[base + t];
      if (mi != 0.f) {
        const float dr = ref[base + t] - lp[base + t];
        const float k3 = expf(dr) - dr - 1.f;
        float pgw = pg;
        if constexpr (W) {
          pgw = is_mul(w[base + t], pg);
          sw += mi * w[base + t];
        }
        l += mi * fmaf(beta, k3, pgw);
        klr += mi * k3;
      }
    }
    l = block_sum<kGrpoThreads>(l, scratch);
    klr = block_sum<kGrpoThreads>(klr, scratch);
    if constexpr (W) sw = block_sum<kGrpoThreads>(sw, scratch);
    if (threadIdx.x == 0) {
      part[s] = c;
      part[S + s] = l;
      part[2 * S + s] = c * ((sr < lo || sr > hi) ? 1.f : 0.f);
      part[3 * S + s] = c * ((sr - 1.f) - ls);
      part[4 * S + s] = klr;
      part[5 * S + s] = ls;
      if constexpr (W) part[6 * S + s] = sw;
    }
    return;
  }
  float cnt = 0.f, l = 0.f, cf = 0.f, akl = 0.f, klr = 0.f;
  for (int t = threadIdx.x; t < T; t += kGrpoThreads) {
    const float mi = m[base + t];
    const GrpoTok k = grpo_token<W>(lp[base + t], old[base + t], ref[base + t], a, lo, hi, beta,
                                    W ? w[base + t] : 1.f);
    cnt += mi;
    l += mi * k.per;
    cf += mi * ((k.rho < lo || k.rho > hi) ? 1.f : 0.f);
    akl += mi * ((k.rho - 1.f) - k.d);
    klr += mi * k.k3;
  }
  cnt = block_sum<kGrpoThreads>(cnt, scratch);
  l = block_sum<kGrpoThreads>(l, scratch);
  cf = block_sum<kGrpoThreads>(cf, scratch);
  akl = block_sum<kGrpoThreads>(akl, scratch);
  klr = block_sum<kGrpoThreads>(klr, scratch);
  if (threadIdx.x == 0) {
    part[s] = cnt;
    part[S + s] = l;
    part[2 * S + s] = cf;
    part[3 * S + s] = akl;
    part[4 * S + s] = klr;
  }
}

// Launch 2 of 2: every workgroup sums the S token counts in the same fixed order (the divisor of
// the `token` mode), then writes its sequence's gradient row; workgroup 0 also finalises the loss
// and the metrics from the partials. No float atomics: two runs are bitwise equal.
//   mode 0 sequence (GRPO):  sum_s [l_s / max(c_s, 1)] / S
//   mode 1 token (DAPO):     sum_s l_s / max(sum_s c_s, 1)
//   mode 2 constant (Dr. GRPO): sum_s l_s / (S * max_len)
//   denom (optional, device [1]) replaces the final divisor (micro-batches of one rollout batch)
//   dlp = m * w_s * [(l1 >= l2 ? l1 : 0) - beta * (exp(dr) - 1)] / divisor, w_s = 1/max(c_s,1) in mode 0
//         (W: the importance weight multiplies the (l1 >= l2 ? l1 : 0) term)
//   metrics: [0] clipfrac, [1] approx KL, [2] k3 KL to the reference (token means), [3] tokens
// SEQ: d sr_s / d lp_u = sr_s m_u / c_s, so with l1, l2 of the row (from part's l_s, not re-reduced)
//   dlp = m * w_s * [g_s (l1 >= l2 ? l1 : 0) - beta * (exp(dr) - 1)] / divisor
//   g_s = sum_t m w / max(c_s, 1) with W; without W it is the constant 1 and is not formed
template <bool W, bool SEQ = false>
__global__ __launch_bounds__(kGrpoThreads) void grpo_grad_kernel(
    const float* __restrict__ lp, const float* __restrict__ old, const float* __restrict__ ref,
    const float* __restrict__ adv, const float* __restrict__ m, const float* __restrict__ part,
    const float* __restrict__ denom, int S, int T, float lo, float hi, float beta, int mode,
    float max_len, float* __restrict__ loss, float* __restrict__ dlp, float* __restrict__ metrics,
    const float* __restrict__ w) {
  __shared__ float scratch[kGrpoThreads / 64];
  const int s = blockIdx.x;
  float cnt = 0.f;
  for (int i = threadIdx.x; i < S; i += kGrpoThreads) cnt += part[i];
  cnt = block_sum<kGrpoThreads>(cnt, scratch);
  const float div = denom != nullptr ? denom[0]
                    : mode == 0      ? static_cast<float>(S)
                    : mode == 1      ? fmaxf(cnt, 1.f)
                                     : static_cast<float>(S) * max_len;
  if (s == 0) {
    float l = 0.f, cf = 0.f, akl = 0.f, klr = 0.f;
    for (int i = threadIdx.x; i < S; i += kGrpoThreads) {
      l += mode == 0 ? part[S + i] / fmaxf(part[i], 1.f) : part[S + i];
      cf += part[2 * S + i];
      akl += part[3 * S + i];
      klr += part[4 * S + i];
    }
    l = block_sum<kGrpoThreads>(l, scratch);
    cf = block_sum<kGrpoThreads>(cf, scratch);
    akl = block_sum<kGrpoThreads>(akl, scratch);
    klr = block_sum<kGrpoThreads>(klr, scratch);
    if (threadIdx.x == 0) {
      const float inv = 1.f / fmaxf(cnt, 1.f);
      loss[0] = l / div;
      metrics[0] = cf * inv;
      metrics[1] = akl * inv;
      metrics[2] = klr * inv;
      metrics[3] = cnt;
    }
  }
  const int64_t base = static_cast<int64_t>(s) * T;
  const float a = adv[s];
  const float scale = (mode == 0 ? 1.f / fmaxf(part[s], 1.f) : 1.f) / div;
  if constexpr (SEQ) {
    const float sr = expf(part[5 * S + s]);
    const float l1 = -a * sr, l2 = -a * fminf(fmaxf(sr, lo), hi);
    float pg = l1 >= l2 ? l1 : 0.f;
    // g_s pg as fma(g_s, pg, 0), rounded on its own: g_s = c_s / c_s = 1 with w = 1 leaves pg exact
    if constexpr (W) pg = fmaf(part[6 * S + s] / fmaxf(part[s], 1.f), pg, 0.f);
    for (int t = threadIdx.x; t < T; t += kGrpoThreads) {
      const float mi = m[base + t];
      float g = 0.f;
      if (mi != 0.f) g = mi * scale * (pg - beta * (expf(ref[base + t] - lp[base + t]) - 1.f));
      dlp[base + t] = g;
    }
    return;
  }
  for (int t = threadIdx.x; t < T; t += kGrpoThreads) {
    const GrpoTok k = grpo_token<W>(lp[base + t], old[base + t], ref[base + t], a, lo, hi, beta, 1.f);
    const float pg = k.l1 >= k.l2 ? k.l1 : 0.f;
    if constexpr (W) {
      // w pg as fma(w, pg, 0): rounded on its own (w = 1 leaves pg exact) and not a product the
      // compiler pairs or contracts with its neighbours, so the rest of the expression compiles as
      // it does in the unweighted instantiation, in the unrolled loop and in the remainder loop
      dlp[base + t] = m[base + t] * scale * (fmaf(w[base + t], pg, 0.f) - beta * (k.edr - 1.f));
    } else {
      dlp[base + t] = m[base + t] * scale * (pg - beta * (k.edr - 1.f));
    }
  }
}

// ==============================================================================================
// Truncated importance weights for the rollout engine / trainer mismatch: the surrogate of every
// action token is multiplied by a detached w = min(pi_trainer_old(a) / pi_rollout(a), C).
// ==============================================================================================

// Launch 1 of 2: one workgroup per row writes the row's weights and five partials part[k * S + s]:
// token count, sum w, sum w^2, #{r > C}, #{r < F} (mask mode).
//   d = trainer_lp - rollout_lp;  level 0 (token): l = d;  level 1 (sequence): l = sum_t m d / max(c_s, 1)
//   r = exp(l);  mode 0 (truncate): w = min(r, C);  mode 1 (mask): w = F <= r <= C ? r : 0
// Entries outside the mask are never read into a sum (the rollout grid holds zeros there) and get
// w = 0. exp overflowing to inf is still compared and clamped correctly: every output is finite.
constexpr int kIsThreads = 256;

__global__ __launch_bounds__(kIsThreads) void rollout_is_rows_kernel(
    const float* __restrict__ tlp, const float* __restrict__ rlp, const float* __restrict__ m, int S,
    int T, float cap, float floor_, int level, int mode, float* __restrict__ w,
    float* __restrict__ part) {
  __shared__ float scratch[kIsThreads / 64];
  const int s = blockIdx.x;
  const int64_t base = static_cast<int64_t>(s) * T;
  float rseq = 0.f;
  if (level == 1) {  // the length-normalised (geometric-mean) ratio of the row
    float a = 0.f, c = 0.f;
    for (int t = threadIdx.x; t < T; t += kIsThreads) {
      const float mi = m[base + t];
      if (mi != 0.f) {
        a += tlp[base + t] - rlp[base + t];
        c += mi;
      }
    }
    a = block_sum<kIsThreads>(a, scratch);
    c = block_sum<kIsThreads>(c, scratch);
    rseq = expf(a / fmaxf(c, 1.f));
  }
  float cnt = 0.f, sw = 0.f, sw2 = 0.f, nhi = 0.f, nlo = 0.f;
  for (int t = threadIdx.x; t < T; t += kIsThreads) {
    const float mi = m[base + t];
    float wi = 0.f;
    if (mi != 0.f) {
      const float r = level == 1 ? rseq : expf(tlp[base + t] - rlp[base + t]);
      const bool high = r > cap, low = mode == 1 && r < floor_;
      wi = mode == 0 ? fminf(r, cap) : ((high || low) ? 0.f : r);
      cnt += mi;
      sw += wi;
      sw2 += wi * wi;
      nhi += high ? 1.f : 0.f;
      nlo += low ? 1.f : 0.f;
    }
    w[base + t] = wi;
  }
  cnt = block_sum<kIsThreads>(cnt, scratch);
  sw = block_sum<kIsThreads>(sw, scratch);
  sw2 = block_sum<kIsThreads>(sw2, scratch);
  nhi = block_sum<kIsThreads>(nhi, scratch);
  nlo = block_sum<kIsThreads>(nlo, scratch);
  if (threadIdx.x == 0) {
    part[s] = cnt;
    part[S + s] = sw;
    part[2 * S + s] = sw2;
    part[3 * S + s] = nhi;
    part[4 * S + s] = nlo;
  }
}

// Launch 2 of 2: one workgroup sums the S partials in a fixed order (no float atomics: two runs are
// bitwise equal) and writes, over the n action tokens,
//   metrics: [0] mean w, [1] #{r > C} / n, [2] #{r < F} / n, [3] ESS fraction
//            min((sum w)^2 / (n sum w^2), 1) (0 when sum w^2 = 0), [4] n           (n -> max(n, 1) in divisors)
__global__ __launch_bounds__(kIsThreads) void rollout_is_metrics_kernel(const float* __restrict__ part,
                                                                        int S,
                                                                        float* __restrict__ metrics) {
  __shared__ float scratch[kIsThreads / 64];
  float cnt = 0.f, sw = 0.f, sw2 = 0.f, nhi = 0.f, nlo = 0.f;
  for (int i = threadIdx.x; i < S; i += kIsThreads) {
    cnt += part[i];
    sw += part[S + i];
    sw2 += part[2 * S + i];
    nhi += part[3 * S + i];
    nlo += part[4 * S + i];
  }
  cnt = block_sum<kIsThreads>(cnt, scratch);
  sw = block_sum<kIsThreads>(sw, scratch);
  sw2 = block_sum<kIsThreads>(sw2, scratch);
  nhi = block_sum<kIsThreads>(nhi, scratch);
  nlo = block_sum<kIsThreads>(nlo, scratch);
  if (threadIdx.x == 0) {
    const float n1 = fmaxf(cnt, 1.f);
    metrics[0] = sw / n1;
    metrics[1] = nhi / n1;
    metrics[2] = nlo / n1;
    metrics[3] = sw2 > 0.f ? fminf((sw * sw) / (n1 * sw2), 1.f) : 0.f;  // <= 1 (Cauchy-Schwarz) up to rounding
    metrics[4] = cnt;
  }
}

// ----------------------------------------------------------------------------------------------
void launch_group_advantages(const float* r, int P, int G, bool scale_std, float eps, float* adv,
                             float* sd, hipStream_t st) {
  if (P == 0 || G == 0) return;
  group_advantages_kernel<<<P, 64, 0, st>>>(r, G, scale_std ? 1 : 0, eps, adv, sd);
}
void launch_grpo_loss(const float* lp, const float* old, const float* ref, const float* adv,
                      const float* m, const float* denom, int S, int T, float lo, float hi,
                      float beta, int mode, float max_len, float* part, float* loss, float* dlp,
                      float* metrics, hipStream_t st) {
  grpo_partials_kernel<false><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, S, T, lo, hi, beta,
                                                           part, nullptr);
  grpo_grad_kernel<false><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, part, denom, S, T, lo, hi,
                                                      beta, mode, max_len, loss, dlp, metrics, nullptr);
}
void launch_grpo_loss_w(const float* lp, const float* old, const float* ref, const float* adv,
                        const float* m, const float* w, const float* denom, int S, int T, float lo,
                        float hi, float beta, int mode, float max_len, float* part, float* loss,
                        float* dlp, float* metrics, hipStream_t st) {
  grpo_partials_kernel<true><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, S, T, lo, hi, beta,
                                                          part, w);
  grpo_grad_kernel<true><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, part, denom, S, T, lo, hi,
                                                     beta, mode, max_len, loss, dlp, metrics, w);
}
// part holds 7 * S floats here (rows 5 and 6: see grpo_partials_kernel); w may be nullptr
void launch_grpo_loss_seq(const float* lp, const float* old, const float* ref, const float* adv,
                          const float* m, const float* w, const float* denom, int S, int T, float lo,
                          float hi, float beta, int mode, float max_len, float* part, float* loss,
                          float* dlp, float* metrics, hipStream_t st) {
  if (w != nullptr) {
    grpo_partials_kernel<true, true><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, S, T, lo, hi,
                                                                  beta, part, w);
    grpo_grad_kernel<true, true><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, part, denom, S, T, lo,
                                                              hi, beta, mode, max_len, loss, dlp, metrics, w);
  } else {
    grpo_partials_kernel<false, true><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, S, T, lo, hi,
                                                                   beta, part, nullptr);
    grpo_grad_kernel<false, true><<<S, kGrpoThreads, 0, st>>>(lp, old, ref, adv, m, part, denom, S, T, lo,
                                                               hi, beta, mode, max_len, loss, dlp, metrics,
                                                               nullptr);
  }
}
void launch_rollout_is_weights(const float* tlp, const float* rlp, const float* m, int S, int T,
                               float cap, float floor_, int level, int mode, float* part, float* w,
                               float* metrics, hipStream_t st) {
  rollout_is_rows_kernel<<<S, kIsThreads, 0, st>>>(tlp, rlp, m, S, T, cap, floor_, level, mode, w, part);
  rollout_is_metrics_kernel<<<1, kIsThreads, 0, st>>>(part, S, metrics);
}
void launch_gae(const float* r, const float* v, const float* m, int S, int T, float gamma,
                float lam, float* adv, float* ret, hipStream_t st) {
  if (S == 0 || T == 0) return;
  gae_kernel<<<S, 64, 0, st>>>(r, v, m, T, gamma, lam, adv, ret);
}
void launch_ppo_policy_loss(const float* lp, const float* old, const float* adv, const float* m,
                            int64_t n, float eps, float* loss, float* dlp, float* metrics,
                            hipStream_t st) {
  ppo_policy_loss_kernel<false><<<1, 1024, 0, st>>>(lp, old, adv, m, n, eps, loss, dlp, metrics, nullptr);
}
void launch_ppo_policy_loss_w(const float* lp, const float* old, const float* adv, const float* m,
                              const float* w, int64_t n, float eps, float* loss, float* dlp,
                              float* metrics, hipStream_t st) {
  ppo_policy_loss_kernel<true><<<1, 1024, 0, st>>>(lp, old, adv, m, n, eps, loss, dlp, metrics, w);
}
void launch_ppo_value_loss(const float* val, const float* old, const float* ret, const float* m,
                           int64_t n, float clip, float* loss, float* dval, hipStream_t st) {
  ppo_value_loss_kernel<<<1, 1024, 0, st>>>(val, old, ret, m, n, clip, loss, dval);
}

// ----------------------------------------------------------------------------------------------
void launch_seq_reduce(const float* lp, const float* mask, int S, int T, float* sum, float* cnt,
                       hipStream_t st) {
  if (S == 0) return;
  seq_reduce_kernel<<<S, 256, 0, st>>>(lp, mask, T, sum, cnt);
}
void launch_seq_expand_grad(const float* coef, const float* mask, const float* cnt, int S, int T,
                            bool mean, float* g, hipStream_t st) {
  const int64_t n = static_cast<int64_t>(S) * T;
  if (n == 0) return;
  int64_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  seq_expand_grad_kernel<<<static_cast<unsigned>(grid), 256, 0, st>>>(coef, mask, cnt, T, S, mean, g);
}
void launch_dpo_loss(const float* pol, const float* ref, int B, float beta, float ls, float* loss,
                     float* dpol, float* rewards, float* metrics, hipStream_t st) {
  dpo_loss_kernel<<<1, 256, 0, st>>>(pol, ref, B, beta, ls, loss, dpol, rewards, metrics);
}
void launch_pairwise_loss(const float* sc, const float* sr, int B, float* loss, float* dsc,
                          float* dsr, float* acc, hipStream_t st) {
  pairwise_loss_kernel<<<1, 256, 0, st>>>(sc, sr, B, loss, dsc, dsr, acc);
}
void launch_kl_penalty_pg(const float* lp, const float* lr, const float* reward, int n,
                          float kl_coef, float* loss, float* kl_mean, float* dlp, float* adv,
                          hipStream_t st) {
  kl_penalty_pg_kernel<<<1, 256, 0, st>>>(lp, lr, reward, n, kl_coef, loss, kl_mean, dlp, adv);
}

}  // namespace dla
