// Launch contract of the sequence / token objective kernels, shared by losses.hip (launchers) and
// bindings_losses.cpp (torch ops). GrpoLossParams is host-side only: the kernels keep their scalar
// argument lists, the launcher unpacks the struct at the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dla {

// The GRPO surrogate in its four instantiations: W = w != null (importance weights on the
// policy-gradient term), SEQ = seq (GSPO: one length-normalised ratio per row).
struct GrpoLossParams {
  const float* lp;     // [S, T] policy log-probs
  const float* old;    // [S, T] old-policy log-probs
  const float* ref;    // [S, T] reference log-probs
  const float* m;      // [S, T] action mask
  const float* w;      // [S, T] detached importance weights, or null: unweighted
  const float* adv;    // [S] one advantage per rollout
  const float* denom;  // [1] replaces the final divisor, or null: the mode's divisor
  int S, T;
  float lo, hi;   // clip range of the ratio: 1 - clip_low, 1 + clip_high
  float beta;     // weight of the k3 reference-KL term
  int mode;       // 0 sequence (GRPO), 1 token (DAPO), 2 constant (Dr. GRPO): S * max_len
  float max_len;  // read in mode 2 only
  bool seq;
  float* part;     // [grpo_part_rows(seq), S] scratch between the two launches
  float* loss;     // [1]
  float* dlp;      // [S, T] dloss/dlp
  float* metrics;  // [4] clipfrac, approx KL, k3 KL to the reference, tokens
};

// Rows of `part`: token count, sum m*per, clipped count, approx-KL sum, k3 sum; the sequence ratio
// adds row 5 (l_s, which launch 2 reads back) and row 6 (sum m*w, written only with weights).
constexpr int grpo_part_rows(bool seq) { return seq ? 7 : 5; }

void launch_grpo_loss(const GrpoLossParams& p, hipStream_t st);

// w [n]: detached importance weights, or null: unweighted. metrics [3].
void launch_ppo_policy_loss(const float* lp, const float* old, const float* adv, const float* m, const float* w,
                            int64_t n, float eps, float* loss, float* dlp, float* metrics, hipStream_t st);
void launch_ppo_value_loss(const float* val, const float* old, const float* ret, const float* m, int64_t n,
                           float clip, float* loss, float* dval, hipStream_t st);
void launch_gae(const float* r, const float* v, const float* m, int S, int T, float gamma, float lam, float* adv,
                float* ret, hipStream_t st);
void launch_group_advantages(const float* r, int P, int G, bool scale_std, float eps, float* adv, float* sd,
                             hipStream_t st);
// part: [5, S] scratch; metrics [5]
void launch_rollout_is_weights(const float* tlp, const float* rlp, const float* m, int S, int T, float cap,
                               float floor_, int level, int mode, float* part, float* w, float* metrics,
                               hipStream_t st);

void launch_seq_reduce(const float* lp, const float* mask, int S, int T, float* sum, float* cnt, hipStream_t st);
void launch_seq_expand_grad(const float* coef, const float* mask, const float* cnt, int S, int T, bool mean,
                            float* g, hipStream_t st);
void launch_dpo_loss(const float* pol, const float* ref, int B, float beta, float ls, float* loss, float* dpol,
                     float* rewards, float* metrics, hipStream_t st);
void launch_pairwise_loss(const float* sc, const float* sr, int B, float* loss, float* dsc, float* dsr, float* acc,
                          hipStream_t st);
void launch_kl_penalty_pg(const float* lp, const float* lr, const float* reward, int n, float kl_coef, float* loss,
                          float* kl_mean, float* dlp, float* adv, hipStream_t st);

}  // namespace dla
