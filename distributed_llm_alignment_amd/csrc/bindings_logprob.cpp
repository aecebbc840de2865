// Torch ops of the vocabulary-row reductions (csrc/logprob.hip): the 15 LM-head log-prob ops, row_lse
// and ensemble_kl. Host-only: argument checks, output allocation, launch on the current stream.
//
// The 15 ops are one forward, one in-place backward and one transposing backward, each in the
// variants plain / *_temp / *_keep / entropy / entropy *_temp. Every variant goes through the same
// checks (row_params, row_vec) and the same three impl functions; the launchers pick the kernel.
#include <ATen/ATen.h>
#include <torch/library.h>

#include <cmath>
#include <tuple>

#include "bind_util.h"
#include "logprob_params.h"

namespace dla {

static void check_logits(const at::Tensor& logits) {
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1, "logits must be [N, V] row-major");
}

// The *_temp ops are the same ops on softmax(inv_temp * logits), inv_temp = float(1.0 / temperature)
// formed by the caller (the divide in double, rounded once); `inv_temp` below is null for the plain
// ops, which launch the kernels they always launched.
static float checked_inv_temp(double inv_temp) {
  const float i = static_cast<float>(inv_temp);
  TORCH_CHECK(std::isfinite(i) && i > 0.f, "inv_temp must be finite and > 0, got ", inv_temp);
  return i;
}

// The kept-set twins of the *_temp ops: row r is taken over the vocabulary entries whose bit is set
// in row keep_rows[r] of keep (uint8 [M, V / 8], bit j of byte i = entry 8 i + j; keep_rows[r] < 0 =
// the full vocabulary). Equal, bit for bit, to the *_temp ops on logits with the dropped entries
// written as -inf, without that write. keep_rows[r] < keep.size(0) is the caller's precondition (a
// check would need a sync). No vocab shard.
static void check_keep(const at::Tensor& logits, const at::Tensor& keep, const at::Tensor& keep_rows) {
  const int64_t N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V % 8 == 0, "keep mask: the vocabulary size must be a multiple of 8 (V % 8 == 0), got ", V);
  TORCH_CHECK(logits.stride(0) % 8 == 0, "keep mask: the logits row stride must be a multiple of 8 (ld % 8 == 0)");
  check_aligned16(logits, "logits");
  TORCH_CHECK(keep.is_cuda() && keep.scalar_type() == at::kByte && keep.dim() == 2 && keep.is_contiguous(),
              "keep must be a contiguous uint8 [M, V / 8] tensor on the GPU");
  TORCH_CHECK(keep.size(1) * 8 == V, "keep.size(1) * 8 must equal V");
  TORCH_CHECK(keep_rows.is_cuda() && keep_rows.scalar_type() == at::kLong && keep_rows.dim() == 1 &&
                  keep_rows.size(0) == N && keep_rows.is_contiguous(),
              "keep_rows must be int64 [N]");
  same_device(logits, keep);
  same_device(logits, keep_rows);
}

// The checks and fields every op shares: logits bf16 [N, V] row-major, targets int64 [N] contiguous on
// the logits' device; inv_temp / keep + keep_rows are null for the ops without them.
static LogprobParams row_params(const at::Tensor& logits, const at::Tensor& tgt, int64_t vocab_offset,
                                const double* inv_temp, const at::Tensor* keep, const at::Tensor* keep_rows) {
  check_logits(logits);
  TORCH_CHECK(tgt.scalar_type() == at::kLong && tgt.is_contiguous() && tgt.numel() == logits.size(0),
              "targets int64 [N]");
  same_device(logits, tgt);
  LogprobParams p{};
  p.logits = bp(logits);
  p.ld = logits.stride(0);
  p.V = static_cast<int>(logits.size(1));
  p.rows = logits.size(0);
  p.off = vocab_offset;
  p.tgt = tgt.data_ptr<int64_t>();
  p.temp = inv_temp != nullptr;
  p.inv_temp = inv_temp ? checked_inv_temp(*inv_temp) : 1.f;
  if (keep) {
    check_keep(logits, *keep, *keep_rows);
    p.keep = keep->data_ptr<uint8_t>();
    p.keep_rows = keep_rows->data_ptr<int64_t>();
  }
  return p;
}

// A per-row vector (lse, ent, grad, grad_ent): fp32, N elements, contiguous, on the logits' device.
static float* row_vec(const at::Tensor& logits, const at::Tensor& v, const char* name) {
  check_f32(v, name);
  TORCH_CHECK(v.numel() == logits.size(0) && v.is_contiguous(), name, " must be a contiguous float32 [N] vector");
  same_device(logits, v);
  return v.data_ptr<float>();
}

// (logp, lse, ent); ent stays undefined without `entropy`. The entropy twins also emit the local
// shard's softmax entropy per row (every row, whatever its target) from the same read; logp and lse
// are bitwise logprob_fwd's.
static std::tuple<at::Tensor, at::Tensor, at::Tensor> fwd_impl(const at::Tensor& logits, const at::Tensor& tgt,
                                                               int64_t vocab_offset, bool entropy,
                                                               const double* inv_temp = nullptr,
                                                               const at::Tensor* keep = nullptr,
                                                               const at::Tensor* keep_rows = nullptr) {
  LogprobParams p = row_params(logits, tgt, vocab_offset, inv_temp, keep, keep_rows);
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto opt = logits.options().dtype(at::kFloat);
  auto logp = at::empty({p.rows}, opt);
  auto lse = at::empty({p.rows}, opt);
  at::Tensor ent;
  p.logp = logp.data_ptr<float>();
  p.lse = lse.data_ptr<float>();
  if (entropy) {
    ent = at::empty({p.rows}, opt);
    p.ent = ent.data_ptr<float>();
  }
  launch_logprob_fwd(p, cur_stream(logits));
  return {logp, lse, ent};
}

static std::tuple<at::Tensor, at::Tensor> first2(std::tuple<at::Tensor, at::Tensor, at::Tensor> t) {
  return {std::get<0>(t), std::get<1>(t)};
}

// The backwards' shared checks. With grad_ent (the entropy twins) the kernels add grad_ent's term
// given the GLOBAL lse and entropy.
static LogprobParams bwd_params(const at::Tensor& logits, const at::Tensor& tgt, const at::Tensor& lse,
                                const at::Tensor& grad, const at::Tensor* ent, const at::Tensor* grad_ent,
                                int64_t vocab_offset, const double* inv_temp, const at::Tensor* keep,
                                const at::Tensor* keep_rows) {
  LogprobParams p = row_params(logits, tgt, vocab_offset, inv_temp, keep, keep_rows);
  p.lse = row_vec(logits, lse, "lse");
  p.g = row_vec(logits, grad, "grad");
  if (grad_ent) {
    p.ent = row_vec(logits, *ent, "ent");
    p.ge = row_vec(logits, *grad_ent, "grad_ent");
  }
  return p;
}

// logits <- dlogits, in place
static void bwd_impl(at::Tensor& logits, const at::Tensor& tgt, const at::Tensor& lse, const at::Tensor& grad,
                     const at::Tensor* ent, const at::Tensor* grad_ent, int64_t vocab_offset,
                     const double* inv_temp = nullptr, const at::Tensor* keep = nullptr,
                     const at::Tensor* keep_rows = nullptr) {
  const LogprobParams p = bwd_params(logits, tgt, lse, grad, ent, grad_ent, vocab_offset, inv_temp, keep, keep_rows);
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  launch_logprob_bwd(p, cur_stream(logits));
}

// The backward with the transposed gradient as a second output: logits <- dlogits (in place) and
// returns dlogitsT [V, N] (the LM head's TN weight-gradient operand). An empty tensor, and nothing
// written, when the shape is outside the kernel (N, V or the row stride not a multiple of 8): run
// the in-place op.
static at::Tensor bwd_t_impl(at::Tensor& logits, const at::Tensor& tgt, const at::Tensor& lse,
                             const at::Tensor& grad, const at::Tensor* ent, const at::Tensor* grad_ent,
                             int64_t vocab_offset, const double* inv_temp = nullptr,
                             const at::Tensor* keep = nullptr, const at::Tensor* keep_rows = nullptr) {
  LogprobParams p = bwd_params(logits, tgt, lse, grad, ent, grad_ent, vocab_offset, inv_temp, keep, keep_rows);
  if (p.rows == 0 || p.rows % 8 != 0 || p.V % 8 != 0 || p.ld % 8 != 0) return at::empty({0}, logits.options());
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto outT = at::empty({logits.size(1), p.rows}, logits.options());
  p.outT = bp(outT);
  const bool ok = launch_logprob_bwd_t(p, cur_stream(logits));
  TORCH_CHECK(ok, "logprob_bwd_t: shape");
  return outT;
}

// ---- the 15 ops: names and schemas as registered below ----
using T = at::Tensor;
using T2 = std::tuple<T, T>;
using T3 = std::tuple<T, T, T>;

T2 logprob_fwd(const T& logits, const T& tgt, int64_t off) { return first2(fwd_impl(logits, tgt, off, false)); }
void logprob_bwd(T& logits, const T& tgt, const T& lse, const T& grad, int64_t off) {
  bwd_impl(logits, tgt, lse, grad, nullptr, nullptr, off);
}
T logprob_bwd_t(T& logits, const T& tgt, const T& lse, const T& grad, int64_t off) {
  return bwd_t_impl(logits, tgt, lse, grad, nullptr, nullptr, off);
}
T3 logprob_entropy_fwd(const T& logits, const T& tgt, int64_t off) { return fwd_impl(logits, tgt, off, true); }
void logprob_entropy_bwd(T& logits, const T& tgt, const T& lse, const T& ent, const T& grad_logp, const T& grad_ent,
                         int64_t off) {
  bwd_impl(logits, tgt, lse, grad_logp, &ent, &grad_ent, off);
}
T logprob_entropy_bwd_t(T& logits, const T& tgt, const T& lse, const T& ent, const T& grad_logp, const T& grad_ent,
                        int64_t off) {
  return bwd_t_impl(logits, tgt, lse, grad_logp, &ent, &grad_ent, off);
}
T2 logprob_fwd_temp(const T& logits, const T& tgt, double inv_temp, int64_t off) {
  return first2(fwd_impl(logits, tgt, off, false, &inv_temp));
}
void logprob_bwd_temp(T& logits, const T& tgt, const T& lse, const T& grad, double inv_temp, int64_t off) {
  bwd_impl(logits, tgt, lse, grad, nullptr, nullptr, off, &inv_temp);
}
T logprob_bwd_t_temp(T& logits, const T& tgt, const T& lse, const T& grad, double inv_temp, int64_t off) {
  return bwd_t_impl(logits, tgt, lse, grad, nullptr, nullptr, off, &inv_temp);
}
T2 logprob_fwd_keep(const T& logits, const T& tgt, const T& keep, const T& keep_rows, double inv_temp) {
  return first2(fwd_impl(logits, tgt, 0, false, &inv_temp, &keep, &keep_rows));
}
void logprob_bwd_keep(T& logits, const T& tgt, const T& lse, const T& grad, const T& keep, const T& keep_rows,
                      double inv_temp) {
  bwd_impl(logits, tgt, lse, grad, nullptr, nullptr, 0, &inv_temp, &keep, &keep_rows);
}
T logprob_bwd_t_keep(T& logits, const T& tgt, const T& lse, const T& grad, const T& keep, const T& keep_rows,
                     double inv_temp) {
  return bwd_t_impl(logits, tgt, lse, grad, nullptr, nullptr, 0, &inv_temp, &keep, &keep_rows);
}
T3 logprob_entropy_fwd_temp(const T& logits, const T& tgt, double inv_temp, int64_t off) {
  return fwd_impl(logits, tgt, off, true, &inv_temp);
}
void logprob_entropy_bwd_temp(T& logits, const T& tgt, const T& lse, const T& ent, const T& grad_logp,
                              const T& grad_ent, double inv_temp, int64_t off) {
  bwd_impl(logits, tgt, lse, grad_logp, &ent, &grad_ent, off, &inv_temp);
}
T logprob_entropy_bwd_t_temp(T& logits, const T& tgt, const T& lse, const T& ent, const T& grad_logp,
                             const T& grad_ent, double inv_temp, int64_t off) {
  return bwd_t_impl(logits, tgt, lse, grad_logp, &ent, &grad_ent, off, &inv_temp);
}

at::Tensor row_lse(const at::Tensor& logits) {
  check_logits(logits);
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto lse = at::empty({logits.size(0)}, logits.options().dtype(at::kFloat));
  launch_row_lse(cbp(logits), logits.stride(0), static_cast<int>(logits.size(1)), logits.size(0),
                 lse.data_ptr<float>(), cur_stream(logits));
  return lse;
}

// s_logits [N, V] (overwritten with dKL/dz * g when write_grad), t_logits [K, N, V] contiguous
at::Tensor ensemble_kl(at::Tensor& s_logits, const at::Tensor& t_logits, const at::Tensor& s_lse,
                       const at::Tensor& t_lse, const c10::optional<at::Tensor>& grad,
                       bool write_grad) {
  check_bf16(s_logits, "s_logits");
  check_bf16(t_logits, "t_logits");
  TORCH_CHECK(s_logits.is_contiguous() && t_logits.is_contiguous() && s_logits.dim() == 2 &&
                  t_logits.dim() == 3 && t_logits.size(1) == s_logits.size(0) &&
                  t_logits.size(2) == s_logits.size(1),
              "ensemble_kl shapes (shared vocab required)");
  const int64_t N = s_logits.size(0), K = t_logits.size(0);
  check_f32(s_lse, "s_lse");
  check_f32(t_lse, "t_lse");
  TORCH_CHECK(s_lse.numel() == N && t_lse.numel() == K * N && t_lse.is_contiguous(), "lse shapes");
  const float* gp = nullptr;
  if (write_grad) {
    TORCH_CHECK(grad && grad->defined() && grad->numel() == N, "grad required");
    check_f32(*grad, "grad");
    gp = grad->data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(s_logits.device());
  auto kl = at::empty({N}, s_logits.options().dtype(at::kFloat));
  launch_ensemble_kl(bp(s_logits), cbp(t_logits), s_logits.size(1), N * s_logits.size(1),
                     static_cast<int>(K), static_cast<int>(s_logits.size(1)),
                     s_lse.data_ptr<float>(), t_lse.data_ptr<float>(), N, gp,
                     kl.data_ptr<float>(), write_grad, cur_stream(s_logits));
  return kl;
}

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("logprob_fwd(Tensor logits, Tensor targets, int vocab_offset=0) -> (Tensor, Tensor)");
  m.def("logprob_bwd(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor grad, int vocab_offset=0) -> ()");
  m.def("logprob_bwd_t(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor grad, int vocab_offset=0) -> Tensor");
  m.def("logprob_entropy_fwd(Tensor logits, Tensor targets, int vocab_offset=0) -> (Tensor, Tensor, Tensor)");
  m.def("logprob_entropy_bwd(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor ent, Tensor grad_logp, Tensor grad_ent, int vocab_offset=0) -> ()");
  m.def("logprob_entropy_bwd_t(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor ent, Tensor grad_logp, Tensor grad_ent, int vocab_offset=0) -> Tensor");
  m.def("logprob_fwd_temp(Tensor logits, Tensor targets, float inv_temp, int vocab_offset=0) -> (Tensor, Tensor)");
  m.def("logprob_bwd_temp(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor grad, float inv_temp, int vocab_offset=0) -> ()");
  m.def("logprob_bwd_t_temp(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor grad, float inv_temp, int vocab_offset=0) -> Tensor");
  m.def("logprob_fwd_keep(Tensor logits, Tensor targets, Tensor keep, Tensor keep_rows, float inv_temp) -> (Tensor, Tensor)");
  m.def("logprob_bwd_keep(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor grad, Tensor keep, Tensor keep_rows, float inv_temp) -> ()");
  m.def("logprob_bwd_t_keep(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor grad, Tensor keep, Tensor keep_rows, float inv_temp) -> Tensor");
  m.def("logprob_entropy_fwd_temp(Tensor logits, Tensor targets, float inv_temp, int vocab_offset=0) -> (Tensor, Tensor, Tensor)");
  m.def("logprob_entropy_bwd_temp(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor ent, Tensor grad_logp, Tensor grad_ent, float inv_temp, int vocab_offset=0) -> ()");
  m.def("logprob_entropy_bwd_t_temp(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor ent, Tensor grad_logp, Tensor grad_ent, float inv_temp, int vocab_offset=0) -> Tensor");
  m.def("row_lse(Tensor logits) -> Tensor");
  m.def("ensemble_kl(Tensor(a!) s_logits, Tensor t_logits, Tensor s_lse, Tensor t_lse, Tensor? grad, bool write_grad) -> Tensor");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("logprob_fwd", &dla::logprob_fwd);
  m.impl("logprob_bwd", &dla::logprob_bwd);
  m.impl("logprob_bwd_t", &dla::logprob_bwd_t);
  m.impl("logprob_entropy_fwd", &dla::logprob_entropy_fwd);
  m.impl("logprob_entropy_bwd", &dla::logprob_entropy_bwd);
  m.impl("logprob_entropy_bwd_t", &dla::logprob_entropy_bwd_t);
  m.impl("logprob_fwd_temp", &dla::logprob_fwd_temp);
  m.impl("logprob_bwd_temp", &dla::logprob_bwd_temp);
  m.impl("logprob_bwd_t_temp", &dla::logprob_bwd_t_temp);
  m.impl("logprob_fwd_keep", &dla::logprob_fwd_keep);
  m.impl("logprob_bwd_keep", &dla::logprob_bwd_keep);
  m.impl("logprob_bwd_t_keep", &dla::logprob_bwd_t_keep);
  m.impl("logprob_entropy_fwd_temp", &dla::logprob_entropy_fwd_temp);
  m.impl("logprob_entropy_bwd_temp", &dla::logprob_entropy_bwd_temp);
  m.impl("logprob_entropy_bwd_t_temp", &dla::logprob_entropy_bwd_t_temp);
  m.impl("row_lse", &dla::row_lse);
  m.impl("ensemble_kl", &dla::ensemble_kl);
}
