// Torch ops of the sequence / token objectives (csrc/losses.hip): seq_reduce, seq_expand_grad,
// dpo_loss, pairwise_loss, kl_penalty_pg, the PPO ops (gae, ppo_policy_loss[_w], ppo_value_loss),
// the GRPO ops (group_advantages, grpo_loss[_w|_seq]) and rollout_is_weights. Host-only: argument
// checks, output allocation, launch on the current stream; no op reads a device value.
//
// Every tensor operand goes through first() or operand(): fp32, on the GPU, contiguous, of the stated
// shape and on the first operand's device. Every size a launcher takes as int goes through to_int().
#include <ATen/ATen.h>
#include <torch/library.h>

#include <climits>
#include <cmath>
#include <tuple>

#include "bind_util.h"
#include "loss_params.h"

namespace dla {

// The operand that fixes the op's shape and device: `dim` dimensions (-1: any).
static const float* first(const at::Tensor& t, int64_t dim, const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && (dim < 0 || t.dim() == dim), op,
              ": ", name, " must be a contiguous float32 GPU tensor", dim < 0 ? "" : dim == 1 ? " [n]" : " [S, T]");
  return t.data_ptr<float>();
}

// A further operand: of `first`'s sizes, or (len >= 0: a per-row vector such as adv, coef, cnt) of
// `len` elements.
static const float* operand(const at::Tensor& t, const at::Tensor& first, const char* op, const char* name,
                            int64_t len = -1) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), op, ": ", name,
              " must be a contiguous float32 GPU tensor");
  if (len < 0) {
    TORCH_CHECK(t.sizes() == first.sizes(), op, ": ", name, " must have the first operand's shape ", first.sizes(),
                ", got ", t.sizes());
  } else {
    TORCH_CHECK(t.numel() == len, op, ": ", name, " must hold ", len, " elements, got ", t.numel());
  }
  TORCH_CHECK(t.device() == first.device(), op, ": ", name, " must be on the first operand's device");
  return t.data_ptr<float>();
}

// The kernels index rows, columns and pairs with int.
static int to_int(int64_t v, const char* op, const char* what) {
  TORCH_CHECK(v >= 0 && v <= INT_MAX, op, ": ", what, " = ", v, " does not fit the kernels' int index");
  return static_cast<int>(v);
}

using T = at::Tensor;
using T2 = std::tuple<T, T>;
using T3 = std::tuple<T, T, T>;
using T4 = std::tuple<T, T, T, T>;

// ---- sequence objectives ----
// lp / mask [S, T] -> (masked sum [S], mask count [S])
T2 seq_reduce(const T& lp, const T& mask) {
  const float* lpp = first(lp, 2, "seq_reduce", "lp");
  const float* mp = operand(mask, lp, "seq_reduce", "mask");
  const int S = to_int(lp.size(0), "seq_reduce", "S"), Tn = to_int(lp.size(1), "seq_reduce", "T");
  c10::hip::HIPGuardMasqueradingAsCUDA g(lp.device());
  auto sum = at::empty({lp.size(0)}, lp.options());
  auto cnt = at::empty({lp.size(0)}, lp.options());
  launch_seq_reduce(lpp, mp, S, Tn, sum.data_ptr<float>(), cnt.data_ptr<float>(), cur_stream(lp));
  return {sum, cnt};
}

// coef / cnt [S], mask [S, T] (the operand that fixes shape and device) -> token gradient [S, T]
T seq_expand_grad(const T& coef, const T& mask, const T& cnt, bool mean) {
  const float* mp = first(mask, 2, "seq_expand_grad", "mask");
  const float* cp = operand(coef, mask, "seq_expand_grad", "coef", mask.size(0));
  const float* np = operand(cnt, mask, "seq_expand_grad", "cnt", mask.size(0));
  const int S = to_int(mask.size(0), "seq_expand_grad", "S"), Tn = to_int(mask.size(1), "seq_expand_grad", "T");
  c10::hip::HIPGuardMasqueradingAsCUDA g(mask.device());
  auto out = at::empty_like(mask);
  launch_seq_expand_grad(cp, mp, np, S, Tn, mean, out.data_ptr<float>(), cur_stream(mask));
  return out;
}

// pol / ref [2B] (chosen then rejected) -> (loss, dloss/dpol [2B], rewards [2B], metrics [4])
T4 dpo_loss(const T& pol, const T& ref, double beta, double label_smoothing) {
  const float* pp = first(pol, -1, "dpo_loss", "pol");
  const float* rp = operand(ref, pol, "dpo_loss", "ref", pol.numel());
  TORCH_CHECK(pol.numel() % 2 == 0, "dpo_loss: pol/ref must be [2B] (chosen then rejected)");
  const int B = to_int(pol.numel() / 2, "dpo_loss", "B");
  c10::hip::HIPGuardMasqueradingAsCUDA g(pol.device());
  auto opt = pol.options();
  auto loss = at::empty({}, opt);
  auto dpol = at::empty({pol.numel()}, opt);
  auto rewards = at::empty({pol.numel()}, opt);
  auto metrics = at::empty({4}, opt);
  launch_dpo_loss(pp, rp, B, static_cast<float>(beta), static_cast<float>(label_smoothing), loss.data_ptr<float>(),
                  dpol.data_ptr<float>(), rewards.data_ptr<float>(), metrics.data_ptr<float>(), cur_stream(pol));
  return {loss, dpol, rewards, metrics};
}

// sc / sr [B] -> (loss, dloss/dsc [B], dloss/dsr [B], accuracy)
T4 pairwise_loss(const T& sc, const T& sr) {
  const float* cp = first(sc, -1, "pairwise_loss", "sc");
  const float* rp = operand(sr, sc, "pairwise_loss", "sr", sc.numel());
  const int B = to_int(sc.numel(), "pairwise_loss", "B");
  c10::hip::HIPGuardMasqueradingAsCUDA g(sc.device());
  auto opt = sc.options();
  auto loss = at::empty({}, opt);
  auto dsc = at::empty({sc.numel()}, opt);
  auto dsr = at::empty({sc.numel()}, opt);
  auto acc = at::empty({}, opt);
  launch_pairwise_loss(cp, rp, B, loss.data_ptr<float>(), dsc.data_ptr<float>(), dsr.data_ptr<float>(),
                       acc.data_ptr<float>(), cur_stream(sc));
  return {loss, dsc, dsr, acc};
}

// lp / lr / reward [n], n > 0 -> (loss, mean KL, dloss/dlp [n], advantages [n])
T4 kl_penalty_pg(const T& lp, const T& lr, const T& reward, double kl_coef) {
  const float* lpp = first(lp, -1, "kl_penalty_pg", "lp");
  const float* lrp = operand(lr, lp, "kl_penalty_pg", "lr", lp.numel());
  const float* rp = operand(reward, lp, "kl_penalty_pg", "reward", lp.numel());
  TORCH_CHECK(lp.numel() > 0, "kl_penalty_pg: no samples");
  const int n = to_int(lp.numel(), "kl_penalty_pg", "n");
  c10::hip::HIPGuardMasqueradingAsCUDA g(lp.device());
  auto opt = lp.options();
  auto loss = at::empty({}, opt);
  auto klm = at::empty({}, opt);
  auto dlp = at::empty({lp.numel()}, opt);
  auto adv = at::empty({lp.numel()}, opt);
  launch_kl_penalty_pg(lpp, lrp, rp, n, static_cast<float>(kl_coef), loss.data_ptr<float>(), klm.data_ptr<float>(),
                       dlp.data_ptr<float>(), adv.data_ptr<float>(), cur_stream(lp));
  return {loss, klm, dlp, adv};
}

// ---- PPO (actor-critic) token objectives: fp32 grids of one shape ----
// rewards / values / mask [S, T] -> (advantages, returns)
T2 gae(const T& rewards, const T& values, const T& mask, double gamma, double lam) {
  const float* rp = first(rewards, 2, "gae", "rewards");
  const float* vp = operand(values, rewards, "gae", "values");
  const float* mp = operand(mask, rewards, "gae", "mask");
  const int S = to_int(rewards.size(0), "gae", "S"), Tn = to_int(rewards.size(1), "gae", "T");
  c10::hip::HIPGuardMasqueradingAsCUDA g(rewards.device());
  auto adv = at::empty_like(rewards);
  auto ret = at::empty_like(rewards);
  launch_gae(rp, vp, mp, S, Tn, static_cast<float>(gamma), static_cast<float>(lam), adv.data_ptr<float>(),
             ret.data_ptr<float>(), cur_stream(rewards));
  return {adv, ret};
}

// w: the importance weights of ppo_policy_loss_w (a grid like lp), or null.
// Returns (loss, dloss/dlp, metrics [3]).
static T3 ppo_policy_loss_impl(const char* op, const T& lp, const T& old, const T& adv, const T& mask, const T* w,
                               double eps) {
  const float* lpp = first(lp, -1, op, "lp");
  const float* op_ = operand(old, lp, op, "old");
  const float* ap = operand(adv, lp, op, "adv");
  const float* mp = operand(mask, lp, op, "mask");
  const float* wp = w ? operand(*w, lp, op, "w") : nullptr;
  c10::hip::HIPGuardMasqueradingAsCUDA g(lp.device());
  auto loss = at::empty({}, lp.options());
  auto dlp = at::empty_like(lp);
  auto metrics = at::empty({3}, lp.options());
  launch_ppo_policy_loss(lpp, op_, ap, mp, wp, lp.numel(), static_cast<float>(eps), loss.data_ptr<float>(),
                         dlp.data_ptr<float>(), metrics.data_ptr<float>(), cur_stream(lp));
  return {loss, dlp, metrics};
}

T3 ppo_policy_loss(const T& lp, const T& old, const T& adv, const T& mask, double eps) {
  return ppo_policy_loss_impl("ppo_policy_loss", lp, old, adv, mask, nullptr, eps);
}
T3 ppo_policy_loss_w(const T& lp, const T& old, const T& adv, const T& mask, const T& w, double eps) {
  return ppo_policy_loss_impl("ppo_policy_loss_w", lp, old, adv, mask, &w, eps);
}

// (loss, dloss/dvalues)
T2 ppo_value_loss(const T& values, const T& old, const T& returns, const T& mask, double clip) {
  const float* vp = first(values, -1, "ppo_value_loss", "values");
  const float* op_ = operand(old, values, "ppo_value_loss", "old");
  const float* rp = operand(returns, values, "ppo_value_loss", "returns");
  const float* mp = operand(mask, values, "ppo_value_loss", "mask");
  c10::hip::HIPGuardMasqueradingAsCUDA g(values.device());
  auto loss = at::empty({}, values.options());
  auto dval = at::empty_like(values);
  launch_ppo_value_loss(vp, op_, rp, mp, values.numel(), static_cast<float>(clip), loss.data_ptr<float>(),
                        dval.data_ptr<float>(), cur_stream(values));
  return {loss, dval};
}

// ---- GRPO: group advantages + clipped surrogate with a k3 reference-KL term ----
// scores [P * G] -> (advantages [P * G], in-group std [P])
T2 group_advantages(const T& scores, int64_t G, bool scale_std, double eps) {
  const float* sp = first(scores, 1, "group_advantages", "scores");
  TORCH_CHECK(G >= 1 && scores.numel() % G == 0, "group_advantages: scores must hold whole groups of G");
  const int P = to_int(scores.numel() / G, "group_advantages", "P"), Gi = to_int(G, "group_advantages", "G");
  c10::hip::HIPGuardMasqueradingAsCUDA g(scores.device());
  auto adv = at::empty_like(scores);
  auto sd = at::empty({scores.numel() / G}, scores.options());
  launch_group_advantages(sp, P, Gi, scale_std, static_cast<float>(eps), adv.data_ptr<float>(), sd.data_ptr<float>(),
                          cur_stream(scores));
  return {adv, sd};
}

// lp / old / ref / mask: [S, T] fp32 grids, adv [S] (one value per rollout), denom: optional
// device [1] replacing the final divisor. mode: 0 sequence, 1 token, 2 constant (S * max_len).
// Returns (loss, dloss/dlp, metrics [4]).
// w: the importance weights of grpo_loss_w and grpo_loss_seq (a grid like lp), or null.
// seq: the sequence-level ratio of grpo_loss_seq (GSPO).
static T3 grpo_loss_impl(const char* op, const T& lp, const T& old, const T& ref, const T& adv, const T& mask,
                         const T* w, const c10::optional<T>& denom, double clip_low, double clip_high, double beta,
                         int64_t mode, double max_len, bool seq) {
  GrpoLossParams p{};
  p.lp = first(lp, 2, op, "lp");
  p.old = operand(old, lp, op, "old");
  p.ref = operand(ref, lp, op, "ref");
  p.m = operand(mask, lp, op, "mask");
  p.w = w ? operand(*w, lp, op, "w") : nullptr;
  p.adv = operand(adv, lp, op, "adv", lp.size(0));
  p.denom = denom.has_value() ? operand(*denom, lp, op, "denom", 1) : nullptr;
  TORCH_CHECK(mode >= 0 && mode <= 2, op, ": mode must be 0 (sequence), 1 (token), 2 (constant)");
  TORCH_CHECK(mode != 2 || max_len > 0 || denom.has_value(), op, ": constant mode needs max_len > 0");
  TORCH_CHECK(lp.size(0) > 0, op, ": no rows");
  p.S = to_int(lp.size(0), op, "S");
  p.T = to_int(lp.size(1), op, "T");
  p.lo = static_cast<float>(1.0 - clip_low);
  p.hi = static_cast<float>(1.0 + clip_high);
  p.beta = static_cast<float>(beta);
  p.mode = static_cast<int>(mode);
  p.max_len = static_cast<float>(max_len);
  p.seq = seq;
  c10::hip::HIPGuardMasqueradingAsCUDA g(lp.device());
  auto loss = at::empty({}, lp.options());
  auto dlp = at::empty_like(lp);
  auto metrics = at::empty({4}, lp.options());
  auto part = at::empty({grpo_part_rows(seq), lp.size(0)}, lp.options());
  p.part = part.data_ptr<float>();
  p.loss = loss.data_ptr<float>();
  p.dlp = dlp.data_ptr<float>();
  p.metrics = metrics.data_ptr<float>();
  launch_grpo_loss(p, cur_stream(lp));
  return {loss, dlp, metrics};
}

T3 grpo_loss(const T& lp, const T& old, const T& ref, const T& adv, const T& mask, const c10::optional<T>& denom,
             double clip_low, double clip_high, double beta, int64_t mode, double max_len) {
  return grpo_loss_impl("grpo_loss", lp, old, ref, adv, mask, nullptr, denom, clip_low, clip_high, beta, mode,
                        max_len, false);
}
// grpo_loss with detached per-token importance weights w [S, T] on the policy-gradient term.
T3 grpo_loss_w(const T& lp, const T& old, const T& ref, const T& adv, const T& mask, const T& w,
               const c10::optional<T>& denom, double clip_low, double clip_high, double beta, int64_t mode,
               double max_len) {
  return grpo_loss_impl("grpo_loss_w", lp, old, ref, adv, mask, &w, denom, clip_low, clip_high, beta, mode, max_len,
                        false);
}
// grpo_loss with the length-normalised sequence-level ratio (GSPO); w as in grpo_loss_w, optional.
T3 grpo_loss_seq(const T& lp, const T& old, const T& ref, const T& adv, const T& mask, const c10::optional<T>& w,
                 const c10::optional<T>& denom, double clip_low, double clip_high, double beta, int64_t mode,
                 double max_len) {
  return grpo_loss_impl("grpo_loss_seq", lp, old, ref, adv, mask, w.has_value() ? &*w : nullptr, denom, clip_low,
                        clip_high, beta, mode, max_len, true);
}

// trainer_lp / rollout_lp / mask: [S, T] fp32 grids. level: 0 token, 1 sequence (length-normalised);
// mode: 0 truncate at cap, 1 mask outside [floor, cap]. Returns (w [S, T], metrics [5]).
T2 rollout_is_weights(const T& trainer_lp, const T& rollout_lp, const T& mask, double cap, double floor,
                      int64_t level, int64_t mode) {
  const char* op = "rollout_is_weights";
  const float* tp = first(trainer_lp, 2, op, "trainer_lp");
  const float* rp = operand(rollout_lp, trainer_lp, op, "rollout_lp");
  const float* mp = operand(mask, trainer_lp, op, "mask");
  TORCH_CHECK(std::isfinite(cap) && cap > 0, "rollout_is_weights: cap must be finite and > 0");
  TORCH_CHECK(floor >= 0 && floor <= cap, "rollout_is_weights: floor must lie in [0, cap]");
  TORCH_CHECK(level == 0 || level == 1, "rollout_is_weights level must be 0 (token) or 1 (sequence)");
  TORCH_CHECK(mode == 0 || mode == 1, "rollout_is_weights mode must be 0 (truncate) or 1 (mask)");
  TORCH_CHECK(trainer_lp.size(0) > 0, "rollout_is_weights: no rows");
  const int S = to_int(trainer_lp.size(0), op, "S"), Tn = to_int(trainer_lp.size(1), op, "T");
  c10::hip::HIPGuardMasqueradingAsCUDA g(trainer_lp.device());
  auto w = at::empty_like(trainer_lp);
  auto metrics = at::empty({5}, trainer_lp.options());
  auto part = at::empty({5, trainer_lp.size(0)}, trainer_lp.options());
  launch_rollout_is_weights(tp, rp, mp, S, Tn, static_cast<float>(cap), static_cast<float>(floor),
                            static_cast<int>(level), static_cast<int>(mode), part.data_ptr<float>(),
                            w.data_ptr<float>(), metrics.data_ptr<float>(), cur_stream(trainer_lp));
  return {w, metrics};
}

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("seq_reduce(Tensor lp, Tensor mask) -> (Tensor, Tensor)");
  m.def("seq_expand_grad(Tensor coef, Tensor mask, Tensor cnt, bool mean) -> Tensor");
  m.def("dpo_loss(Tensor pol, Tensor ref, float beta, float label_smoothing) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("pairwise_loss(Tensor sc, Tensor sr) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("gae(Tensor rewards, Tensor values, Tensor mask, float gamma, float lam) -> (Tensor, Tensor)");
  m.def("ppo_policy_loss(Tensor lp, Tensor old, Tensor adv, Tensor mask, float eps) -> (Tensor, Tensor, Tensor)");
  m.def("ppo_value_loss(Tensor values, Tensor old, Tensor returns, Tensor mask, float clip) -> (Tensor, Tensor)");
  m.def("group_advantages(Tensor scores, int G, bool scale_std, float eps) -> (Tensor, Tensor)");
  m.def("grpo_loss(Tensor lp, Tensor old, Tensor ref, Tensor adv, Tensor mask, Tensor? denom, float clip_low, float clip_high, float beta, int mode, float max_len) -> (Tensor, Tensor, Tensor)");
  m.def("grpo_loss_w(Tensor lp, Tensor old, Tensor ref, Tensor adv, Tensor mask, Tensor w, Tensor? denom, float clip_low, float clip_high, float beta, int mode, float max_len) -> (Tensor, Tensor, Tensor)");
  m.def("grpo_loss_seq(Tensor lp, Tensor old, Tensor ref, Tensor adv, Tensor mask, Tensor? w, Tensor? denom, float clip_low, float clip_high, float beta, int mode, float max_len) -> (Tensor, Tensor, Tensor)");
  m.def("ppo_policy_loss_w(Tensor lp, Tensor old, Tensor adv, Tensor mask, Tensor w, float eps) -> (Tensor, Tensor, Tensor)");
  m.def("rollout_is_weights(Tensor trainer_lp, Tensor rollout_lp, Tensor mask, float cap, float floor, int level, int mode) -> (Tensor, Tensor)");
  m.def("kl_penalty_pg(Tensor lp, Tensor lr, Tensor reward, float kl_coef) -> (Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("seq_reduce", &dla::seq_reduce);
  m.impl("seq_expand_grad", &dla::seq_expand_grad);
  m.impl("dpo_loss", &dla::dpo_loss);
  m.impl("pairwise_loss", &dla::pairwise_loss);
  m.impl("kl_penalty_pg", &dla::kl_penalty_pg);
  m.impl("gae", &dla::gae);
  m.impl("ppo_policy_loss", &dla::ppo_policy_loss);
  m.impl("ppo_value_loss", &dla::ppo_value_loss);
  m.impl("group_advantages", &dla::group_advantages);
  m.impl("grpo_loss", &dla::grpo_loss);
  m.impl("grpo_loss_w", &dla::grpo_loss_w);
  m.impl("grpo_loss_seq", &dla::grpo_loss_seq);
  m.impl("ppo_policy_loss_w", &dla::ppo_policy_loss_w);
  m.impl("rollout_is_weights", &dla::rollout_is_weights);
}
