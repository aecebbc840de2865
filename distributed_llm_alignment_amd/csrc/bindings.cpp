// Torch custom-op registry for the gfx950 kernels: `torch.ops.dla.*`. This file opens the library
// (norms, activations, RoPE, transpose, GJSD, optimizer); the other bindings_*.cpp add their family
// as a fragment.
//
// Host side only (compiled by the host C++ compiler): every op validates operand shapes,
// dtypes, strides and devices BEFORE launching (a mis-shaped launch of a hand-written kernel
// can fault the GPU), allocates outputs through the torch caching allocator and launches on
// the caller's current HIP stream. No op synchronises the host.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <tuple>

#include "bind_util.h"
#include "gjsd_params.h"

namespace dla {

// ---- kernel launchers (defined in *.hip) ----
void launch_norm_fwd(const bf16_t*, const bf16_t*, bf16_t*, const bf16_t*, const bf16_t*, bf16_t*,
                     float*, float*, int, int, float, bool, hipStream_t);
void launch_norm_bwd(const bf16_t*, const bf16_t*, const bf16_t*, const float*, const float*,
                     const bf16_t*, bf16_t*, float*, float*, bf16_t*, bf16_t*, int, int, bool,
                     hipStream_t);
int norm_bwd_grid(int rows);
int norm_wgrad_scratch_rows();
void launch_swiglu_fwd(const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
void launch_swiglu_bwd(const bf16_t*, const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
void launch_swiglu_fwd_t(const bf16_t*, bf16_t*, bf16_t*, int64_t, int, hipStream_t);
void launch_swiglu_bwd_t(const bf16_t*, const bf16_t*, bf16_t*, bf16_t*, int64_t, int, hipStream_t);
void launch_gelu_fwd(const bf16_t*, bf16_t*, int64_t, hipStream_t);
void launch_gelu_bwd(const bf16_t*, const bf16_t*, bf16_t*, int64_t, hipStream_t);
void launch_rope_fwd(const bf16_t*, int64_t, bf16_t*, bf16_t*, const float*, const float*,
                     const int*, int64_t, int, int, int, int, int, int, hipStream_t);
void launch_rope_bwd(const bf16_t*, const bf16_t*, bf16_t*, int64_t, const float*, const float*,
                     const int*, int64_t, int, int, int, int, int, int, hipStream_t);
void launch_adamw(bf16_t*, float*, const void*, bool, float*, float*, int64_t, float, float,
                  float, float, float, int, const float*, float, hipStream_t);
void launch_grad_sumsq(const void*, bool, int64_t, float*, float*, bool, hipStream_t);
int sumsq_grid(int64_t n);
void launch_clip_coef(const float*, float, float*, float*, hipStream_t);

void launch_transpose_bf16(const bf16_t*, int64_t, int64_t, int64_t, bf16_t*, int64_t, hipStream_t);

// ================================= norms ======================================================
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> norm_fwd(
    const at::Tensor& x, const c10::optional<at::Tensor>& res, const at::Tensor& w,
    const c10::optional<at::Tensor>& b, double eps, bool rms) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  TORCH_CHECK(x.is_contiguous(), "x must be contiguous");
  const int64_t H = x.size(-1);
  // forward kernels cover H <= 8192 (wave per row, 16 x 8 columns per lane)
  TORCH_CHECK(H % 8 == 0 && H <= 8192, "norm_fwd: hidden size must be a multiple of 8 and <= 8192");
  TORCH_CHECK(w.numel() == H && w.is_contiguous(), "w shape");
  // the RMS kernels are instantiated without a bias (no model has one): reject, never drop it
  TORCH_CHECK(!(rms && b && b->defined()), "norm_fwd: RMSNorm takes no bias");
  const int64_t rows = x.numel() / H;
  TORCH_CHECK(rows < (1ll << 31), "too many rows");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  auto y = at::empty_like(x);
  at::Tensor so;
  const bf16_t* rptr = nullptr;
  if (res && res->defined()) {
    check_bf16(*res, "res");
    TORCH_CHECK(res->sizes() == x.sizes() && res->is_contiguous(), "res shape");
    so = at::empty_like(x);
    rptr = cbp(*res);
  }
  const bf16_t* bptr = nullptr;
  if (b && b->defined()) {
    check_bf16(*b, "b");
    TORCH_CHECK(b->numel() == H && b->is_contiguous(), "b shape");
    bptr = cbp(*b);
  }
  auto opt = x.options().dtype(at::kFloat);
  auto rstd = at::empty({rows}, opt);
  auto mean = rms ? at::empty({0}, opt) : at::empty({rows}, opt);
  check_aligned16(x, "x");
  launch_norm_fwd(cbp(x), rptr, so.defined() ? bp(so) : nullptr, cbp(w), bptr, bp(y),
                  rstd.data_ptr<float>(), rms ? nullptr : mean.data_ptr<float>(),
                  static_cast<int>(rows), static_cast<int>(H), static_cast<float>(eps), rms,
                  cur_stream(x));
  return {y, so.defined() ? so : at::empty({0}, x.options()), rstd, mean};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> norm_bwd(const at::Tensor& dy, const at::Tensor& s,
                                                        const at::Tensor& w,
                                                        const at::Tensor& rstd,
                                                        const c10::optional<at::Tensor>& mean,
                                                        const c10::optional<at::Tensor>& dres,
                                                        bool has_bias, bool rms) {
  check_bf16(dy, "dy");
  check_bf16(s, "s");
  check_bf16(w, "w");
  check_f32(rstd, "rstd");
  TORCH_CHECK(dy.is_contiguous() && s.is_contiguous() && dy.sizes() == s.sizes(), "dy/s shape");
  const int64_t H = s.size(-1);
  const int64_t rows = s.numel() / H;
  TORCH_CHECK(H % 8 == 0 && H <= 16384, "hidden size");
  // no RMS kernel writes db partials: folding them would return uninitialised memory as db
  TORCH_CHECK(!(has_bias && rms), "norm_bwd: RMSNorm takes no bias");
  TORCH_CHECK(rstd.numel() == rows, "rstd shape");
  const float* mptr = nullptr;
  if (!rms) {
    TORCH_CHECK(mean && mean->defined() && mean->numel() == rows, "LayerNorm needs mean");
    mptr = mean->data_ptr<float>();
  }
  const bf16_t* dr = nullptr;
  if (dres && dres->defined()) {
    check_bf16(*dres, "dres");
    TORCH_CHECK(dres->sizes() == s.sizes() && dres->is_contiguous(), "dres shape");
    dr = cbp(*dres);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(s.device());
  auto ds = at::empty_like(s);
  const int grid = norm_bwd_grid(static_cast<int>(rows));
  auto fopt = s.options().dtype(at::kFloat);
  const int srows = grid + norm_wgrad_scratch_rows();  // partials + stage-1 scratch
  auto dwp = at::empty({srows, H}, fopt);
  auto dbp = has_bias ? at::empty({srows, H}, fopt) : at::empty({0}, fopt);
  auto dw = at::empty({H}, w.options());
  auto db = has_bias ? at::empty({H}, w.options()) : at::empty({0}, w.options());
  launch_norm_bwd(cbp(dy), cbp(s), cbp(w), rstd.data_ptr<float>(), mptr, dr, bp(ds),
                  dwp.data_ptr<float>(), has_bias ? dbp.data_ptr<float>() : nullptr, bp(dw),
                  has_bias ? bp(db) : nullptr, static_cast<int>(rows), static_cast<int>(H), rms,
                  cur_stream(s));
  return {ds, dw, db};
}

// ================================= activations ================================================
at::Tensor swiglu_fwd(const at::Tensor& gu) {
  check_bf16(gu, "gu");
  TORCH_CHECK(gu.is_contiguous(), "gu contiguous");
  const int64_t two_f = gu.size(-1);
  TORCH_CHECK(two_f % 16 == 0, "2F must be a multiple of 16");
  const int64_t F = two_f / 2, rows = gu.numel() / two_f;
  auto sizes = gu.sizes().vec();
  sizes.back() = F;
  c10::hip::HIPGuardMasqueradingAsCUDA g(gu.device());
  auto out = at::empty(sizes, gu.options());
  launch_swiglu_fwd(cbp(gu), bp(out), rows, static_cast<int>(F), cur_stream(gu));
  return out;
}

at::Tensor swiglu_bwd(const at::Tensor& gu, const at::Tensor& dout) {
  check_bf16(gu, "gu");
  check_bf16(dout, "dout");
  TORCH_CHECK(gu.is_contiguous() && dout.is_contiguous(), "contiguous");
  const int64_t two_f = gu.size(-1), F = two_f / 2, rows = gu.numel() / two_f;
  TORCH_CHECK(two_f % 16 == 0 && dout.numel() == rows * F, "shapes");
  c10::hip::HIPGuardMasqueradingAsCUDA g(gu.device());
  auto dgu = at::empty_like(gu);
  launch_swiglu_bwd(cbp(gu), cbp(dout), bp(dgu), rows, static_cast<int>(F), cur_stream(gu));
  return dgu;
}

// SwiGLU that also writes the transposed output ([F, rows]) for the TN weight-gradient GEMMs.
std::tuple<at::Tensor, at::Tensor> swiglu_fwd_t(const at::Tensor& gu) {
  check_bf16(gu, "gu");
  TORCH_CHECK(gu.is_contiguous() && gu.dim() == 2, "gu: contiguous [rows, 2F]");
  const int64_t rows = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(gu.size(1) == 2 * F && F % 64 == 0, "F must be a multiple of 64");
  c10::hip::HIPGuardMasqueradingAsCUDA g(gu.device());
  auto out = at::empty({rows, F}, gu.options());
  auto outT = at::empty({F, rows}, gu.options());
  launch_swiglu_fwd_t(cbp(gu), bp(out), bp(outT), rows, static_cast<int>(F), cur_stream(gu));
  return {out, outT};
}

std::tuple<at::Tensor, at::Tensor> swiglu_bwd_t(const at::Tensor& gu, const at::Tensor& dout) {
  check_bf16(gu, "gu");
  check_bf16(dout, "dout");
  TORCH_CHECK(gu.is_contiguous() && dout.is_contiguous() && gu.dim() == 2, "contiguous 2-D");
  const int64_t rows = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(gu.size(1) == 2 * F && F % 64 == 0 && dout.numel() == rows * F, "shapes");
  c10::hip::HIPGuardMasqueradingAsCUDA g(gu.device());
  auto dgu = at::empty_like(gu);
  auto dguT = at::empty({2 * F, rows}, gu.options());
  launch_swiglu_bwd_t(cbp(gu), cbp(dout), bp(dgu), bp(dguT), rows, static_cast<int>(F),
                      cur_stream(gu));
  return {dgu, dguT};
}

at::Tensor gelu_fwd(const at::Tensor& x) {
  check_bf16(x, "x");
  TORCH_CHECK(x.is_contiguous() && x.numel() % 8 == 0, "x contiguous, numel % 8");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  auto y = at::empty_like(x);
  launch_gelu_fwd(cbp(x), bp(y), x.numel(), cur_stream(x));
  return y;
}

at::Tensor gelu_bwd(const at::Tensor& x, const at::Tensor& dy) {
  check_bf16(x, "x");
  check_bf16(dy, "dy");
  TORCH_CHECK(x.is_contiguous() && dy.is_contiguous() && x.numel() == dy.numel() &&
                  x.numel() % 8 == 0,
              "shapes");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  auto dx = at::empty_like(x);
  launch_gelu_bwd(cbp(x), cbp(dy), bp(dx), x.numel(), cur_stream(x));
  return dx;
}

// ================================= rope =======================================================
static void check_rope_common(const at::Tensor& cos_t, const at::Tensor& sin_t,
                              const c10::optional<at::Tensor>& pos, int64_t tokens, int64_t D,
                              int64_t rot, int64_t T, int64_t pos_offset) {
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  TORCH_CHECK(cos_t.is_contiguous() && sin_t.is_contiguous() && cos_t.dim() == 2 &&
                  cos_t.sizes() == sin_t.sizes() && cos_t.size(1) == rot / 2,
              "cos/sin tables must be [max_pos, rot/2]");
  TORCH_CHECK(D % 8 == 0 && rot % 16 == 0 && rot <= D, "rot must be a multiple of 16 <= D");
  if (pos && pos->defined()) {
    TORCH_CHECK(pos->scalar_type() == at::kInt && pos->is_contiguous() && pos->numel() == tokens,
                "pos must be int32 [tokens]");
  } else {
    // implicit positions t + pos_offset, t < T, must stay inside the table (as attn_fwd checks)
    TORCH_CHECK(pos_offset >= 0 && T + pos_offset <= cos_t.size(0),
                "rope: T + pos_offset exceeds the cos/sin table length");
  }
}

std::tuple<at::Tensor, at::Tensor> rope_fwd(const at::Tensor& qkv, const at::Tensor& cos_t,
                                            const at::Tensor& sin_t,
                                            const c10::optional<at::Tensor>& pos, int64_t Hq,
                                            int64_t Hkv, int64_t D, int64_t rot, int64_t T,
                                            int64_t pos_offset) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1, "qkv must be [tokens, C] with unit col stride");
  TORCH_CHECK(qkv.size(1) >= (Hq + 2 * Hkv) * D, "qkv width");
  TORCH_CHECK(qkv.stride(0) % 8 == 0, "qkv row stride must be a multiple of 8");
  const int64_t tokens = qkv.size(0);
  TORCH_CHECK(T > 0 && tokens % T == 0, "tokens must be a multiple of T");
  check_rope_common(cos_t, sin_t, pos, tokens, D, rot, T, pos_offset);
  c10::hip::HIPGuardMasqueradingAsCUDA g(qkv.device());
  auto q = at::empty({tokens, Hq * D}, qkv.options());
  auto k = at::empty({tokens, Hkv * D}, qkv.options());
  launch_rope_fwd(cbp(qkv), qkv.stride(0), bp(q), bp(k), cos_t.data_ptr<float>(),
                  sin_t.data_ptr<float>(),
                  (pos && pos->defined()) ? pos->data_ptr<int>() : nullptr, tokens,
                  static_cast<int>(T), static_cast<int>(pos_offset), static_cast<int>(Hq),
                  static_cast<int>(Hkv), static_cast<int>(D), static_cast<int>(rot),
                  cur_stream(qkv));
  return {q, k};
}

void rope_bwd(const at::Tensor& dq, const at::Tensor& dk, at::Tensor& dqkv,
              const at::Tensor& cos_t, const at::Tensor& sin_t,
              const c10::optional<at::Tensor>& pos, int64_t Hq, int64_t Hkv, int64_t D,
              int64_t rot, int64_t T, int64_t pos_offset) {
  check_bf16(dq, "dq");
  check_bf16(dk, "dk");
  check_bf16(dqkv, "dqkv");
  const int64_t tokens = dqkv.size(0);
  TORCH_CHECK(dq.is_contiguous() && dk.is_contiguous() && dq.numel() == tokens * Hq * D &&
                  dk.numel() == tokens * Hkv * D,
              "dq/dk shape");
  TORCH_CHECK(dqkv.dim() == 2 && dqkv.stride(1) == 1 && dqkv.stride(0) % 8 == 0 &&
                  dqkv.size(1) >= (Hq + 2 * Hkv) * D,
              "dqkv layout");
  TORCH_CHECK(T > 0 && tokens % T == 0, "tokens must be a multiple of T");
  check_rope_common(cos_t, sin_t, pos, tokens, D, rot, T, pos_offset);
  c10::hip::HIPGuardMasqueradingAsCUDA g(dqkv.device());
  launch_rope_bwd(cbp(dq), cbp(dk), bp(dqkv), dqkv.stride(0), cos_t.data_ptr<float>(),
                  sin_t.data_ptr<float>(),
                  (pos && pos->defined()) ? pos->data_ptr<int>() : nullptr, tokens,
                  static_cast<int>(T), static_cast<int>(pos_offset), static_cast<int>(Hq),
                  static_cast<int>(Hkv), static_cast<int>(D), static_cast<int>(rot),
                  cur_stream(dqkv));
}

// out [C, R] <- in [R, C]^T (both row-major with unit column stride, 16-byte aligned rows)
void transpose_bf16(const at::Tensor& in, at::Tensor& out) {
  check_bf16(in, "in");
  check_bf16(out, "out");
  TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && in.stride(1) == 1 && out.stride(1) == 1 &&
                  out.size(0) == in.size(1) && out.size(1) == in.size(0),
              "transpose_bf16: in [R, C], out [C, R], unit column stride");
  TORCH_CHECK(in.stride(0) % 8 == 0 && out.stride(0) % 8 == 0, "16-byte aligned rows");
  check_aligned16(in, "in");
  check_aligned16(out, "out");
  same_device(in, out);
  c10::hip::HIPGuardMasqueradingAsCUDA g(in.device());
  launch_transpose_bf16(cbp(in), in.size(0), in.size(1), in.stride(0), bp(out), out.stride(0),
                        cur_stream(in));
}

// ================================= JSD(beta) distillation (GKD) ===============================
// s [N, V] bf16, t [K, N, V] bf16 (last dim contiguous, any row strides), row_mask [N] float or
// uint8 (0: the row is skipped and every output of it is 0). inv_temp = float(1.0 / temperature)
// formed by the caller. See gjsd.hip for the formulas.
static GjsdParams gjsd_params(const at::Tensor& s, const at::Tensor& t, const c10::optional<at::Tensor>& row_mask,
                              double beta, double inv_temp) {
  check_bf16(s, "s");
  check_bf16(t, "t");
  same_device(s, t);
  TORCH_CHECK(s.dim() == 2 && t.dim() == 3 && t.size(1) == s.size(0) && t.size(2) == s.size(1),
              "gjsd: s [N, V] and t [K, N, V] (shared vocabulary required)");
  TORCH_CHECK(s.size(1) >= 1 && s.size(1) < (int64_t(1) << 31) && s.size(0) < (int64_t(1) << 31), "gjsd: N, V range");
  TORCH_CHECK(t.size(0) >= 1 && t.size(0) <= kGjsdMaxTeachers, "gjsd: 1 to ", kGjsdMaxTeachers, " teachers, got ",
              t.size(0));
  TORCH_CHECK((s.size(1) == 1 || s.stride(1) == 1) && (t.size(2) == 1 || t.stride(2) == 1) && s.stride(0) >= s.size(1) &&
                  t.stride(1) >= t.size(2) && t.stride(0) >= 0,
              "gjsd: logits must be row-major with non-overlapping rows");
  TORCH_CHECK(beta >= 0.0 && beta <= 1.0, "gjsd: beta must be in [0, 1], got ", beta);
  GjsdParams p{};
  p.it = static_cast<float>(inv_temp);
  TORCH_CHECK(std::isfinite(p.it) && p.it > 0.f, "inv_temp must be finite and > 0, got ", inv_temp);
  p.s = cbp(s);
  p.t = cbp(t);
  p.s_ld = s.stride(0);
  p.t_sk = t.stride(0);
  p.t_ld = t.stride(1);
  p.N = s.size(0);
  p.K = static_cast<int>(t.size(0));
  p.V = static_cast<int>(s.size(1));
  if (row_mask && row_mask->defined()) {
    const at::Tensor& m = *row_mask;
    check_cuda(m, "row_mask");
    same_device(s, m);
    TORCH_CHECK(m.scalar_type() == at::kFloat || m.scalar_type() == at::kByte, "row_mask must be float32 or uint8");
    TORCH_CHECK(m.dim() == 1 && m.size(0) == p.N && m.is_contiguous(), "row_mask [N] contiguous");
    p.mask = m.data_ptr();
    p.mask_u8 = m.scalar_type() == at::kByte;
  }
  p.beta = static_cast<float>(beta);
  p.c = beta == 1.0 ? 1.f : static_cast<float>(1.0 - beta);
  p.lb = beta > 0.0 ? static_cast<float>(std::log(beta)) : 0.f;
  p.l1b = beta < 1.0 ? static_cast<float>(std::log1p(-beta)) : 0.f;
  p.logK = static_cast<float>(std::log(static_cast<double>(p.K)));
  p.invK = static_cast<float>(1.0 / static_cast<double>(p.K));
  return p;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> gjsd_fwd(const at::Tensor& s, const at::Tensor& t,
                                                                    const c10::optional<at::Tensor>& row_mask,
                                                                    double beta, double inv_temp) {
  GjsdParams p = gjsd_params(s, t, row_mask, beta, inv_temp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(s.device());
  const auto f32 = s.options().dtype(at::kFloat);
  auto loss = at::empty({p.N}, f32), aux = at::empty({p.N}, f32), s_lse = at::empty({p.N}, f32);
  auto t_lse = at::empty({static_cast<int64_t>(p.K), p.N}, f32);
  p.loss = loss.data_ptr<float>();
  p.aux = aux.data_ptr<float>();
  p.s_lse = s_lse.data_ptr<float>();
  p.t_lse = t_lse.data_ptr<float>();
  launch_gjsd(p, false, cur_stream(s));
  return {loss, aux, s_lse, t_lse};
}

at::Tensor gjsd_bwd(const at::Tensor& s, const at::Tensor& t, const at::Tensor& s_lse, const at::Tensor& t_lse,
                    const at::Tensor& aux, const c10::optional<at::Tensor>& row_mask, const at::Tensor& grad,
                    double beta, double inv_temp) {
  GjsdParams p = gjsd_params(s, t, row_mask, beta, inv_temp);
  for (const at::Tensor* x : {&s_lse, &t_lse, &aux, &grad}) {
    check_f32(*x, "s_lse / t_lse / aux / grad");
    same_device(s, *x);
    TORCH_CHECK(x->is_contiguous(), "gjsd_bwd: row scalars must be contiguous");
  }
  TORCH_CHECK(s_lse.numel() == p.N && aux.numel() == p.N && grad.numel() == p.N &&
                  t_lse.numel() == static_cast<int64_t>(p.K) * p.N,
              "gjsd_bwd: s_lse / aux / grad [N], t_lse [K, N]");
  c10::hip::HIPGuardMasqueradingAsCUDA g(s.device());
  auto ds = at::empty({p.N, static_cast<int64_t>(p.V)}, s.options());
  p.s_lse = s_lse.data_ptr<float>();
  p.t_lse = t_lse.data_ptr<float>();
  p.aux = aux.data_ptr<float>();
  p.g = grad.data_ptr<float>();
  p.ds = bp(ds);
  launch_gjsd(p, true, cur_stream(s));
  return ds;
}

// ================================= optimizer ==================================================
void adamw_step(const c10::optional<at::Tensor>& param, const c10::optional<at::Tensor>& master,
                const at::Tensor& grad, at::Tensor& m, at::Tensor& v, double lr, double b1,
                double b2, double eps, double wd, int64_t step,
                const c10::optional<at::Tensor>& clip, double grad_scale) {
  const int64_t n = grad.numel();
  TORCH_CHECK(n % 8 == 0, "flat buffers must be padded to a multiple of 8 elements");
  TORCH_CHECK(grad.is_contiguous() && m.is_contiguous() && v.is_contiguous(), "contiguous");
  check_cuda(grad, "grad");
  TORCH_CHECK(grad.scalar_type() == at::kBFloat16 || grad.scalar_type() == at::kFloat,
              "grad must be bf16 or fp32");
  check_f32(m, "m");
  check_f32(v, "v");
  TORCH_CHECK(m.numel() == n && v.numel() == n, "m/v size");
  bf16_t* pp = nullptr;
  float* mp = nullptr;
  if (param && param->defined()) {
    check_bf16(*param, "param");
    TORCH_CHECK(param->is_contiguous() && param->numel() == n, "param size");
    pp = bp(*param);
  }
  if (master && master->defined()) {
    check_f32(*master, "master");
    TORCH_CHECK(master->is_contiguous() && master->numel() == n, "master size");
    mp = master->data_ptr<float>();
  }
  TORCH_CHECK(pp || mp, "need bf16 param or fp32 master");
  const float* cp = nullptr;
  if (clip && clip->defined()) {
    check_f32(*clip, "clip");
    cp = clip->data_ptr<float>();
  }
  TORCH_CHECK(step >= 1, "step must be >= 1");
  c10::hip::HIPGuardMasqueradingAsCUDA g(grad.device());
  launch_adamw(pp, mp, grad.data_ptr(), grad.scalar_type() == at::kBFloat16, m.data_ptr<float>(),
               v.data_ptr<float>(), n, static_cast<float>(lr), static_cast<float>(b1),
               static_cast<float>(b2), static_cast<float>(eps), static_cast<float>(wd),
               static_cast<int>(step), cp, static_cast<float>(grad_scale), cur_stream(grad));
}

void grad_sumsq(const at::Tensor& grad, at::Tensor& out, bool accumulate) {
  check_cuda(grad, "grad");
  check_f32(out, "out");
  TORCH_CHECK(grad.is_contiguous() && grad.numel() % 8 == 0, "grad contiguous, numel % 8");
  TORCH_CHECK(grad.scalar_type() == at::kBFloat16 || grad.scalar_type() == at::kFloat, "dtype");
  TORCH_CHECK(out.numel() >= 1, "out");
  c10::hip::HIPGuardMasqueradingAsCUDA g(grad.device());
  auto partial = at::empty({sumsq_grid(grad.numel())}, out.options());
  launch_grad_sumsq(grad.data_ptr(), grad.scalar_type() == at::kBFloat16, grad.numel(),
                    partial.data_ptr<float>(), out.data_ptr<float>(), accumulate,
                    cur_stream(grad));
}

std::tuple<at::Tensor, at::Tensor> clip_coef(const at::Tensor& sumsq, double max_norm) {
  check_f32(sumsq, "sumsq");
  c10::hip::HIPGuardMasqueradingAsCUDA g(sumsq.device());
  auto norm = at::empty({}, sumsq.options());
  auto coef = at::empty({}, sumsq.options());
  launch_clip_coef(sumsq.data_ptr<float>(), static_cast<float>(max_norm), norm.data_ptr<float>(),
                   coef.data_ptr<float>(), cur_stream(sumsq));
  return {norm, coef};
}

}  // namespace dla

TORCH_LIBRARY(dla, m) {
  m.def("norm_fwd(Tensor x, Tensor? res, Tensor w, Tensor? b, float eps, bool rms) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("norm_bwd(Tensor dy, Tensor s, Tensor w, Tensor rstd, Tensor? mean, Tensor? dres, bool has_bias, bool rms) -> (Tensor, Tensor, Tensor)");
  m.def("swiglu_fwd(Tensor gu) -> Tensor");
  m.def("swiglu_bwd(Tensor gu, Tensor dout) -> Tensor");
  m.def("swiglu_fwd_t(Tensor gu) -> (Tensor, Tensor)");
  m.def("swiglu_bwd_t(Tensor gu, Tensor dout) -> (Tensor, Tensor)");
  m.def("gelu_fwd(Tensor x) -> Tensor");
  m.def("gelu_bwd(Tensor x, Tensor dy) -> Tensor");
  m.def("rope_fwd(Tensor qkv, Tensor cos, Tensor sin, Tensor? pos, int Hq, int Hkv, int D, int rot, int T, int pos_offset) -> (Tensor, Tensor)");
  m.def("rope_bwd(Tensor dq, Tensor dk, Tensor(a!) dqkv, Tensor cos, Tensor sin, Tensor? pos, int Hq, int Hkv, int D, int rot, int T, int pos_offset) -> ()");
  m.def("transpose_bf16(Tensor input, Tensor(a!) out) -> ()");
  m.def("gjsd_fwd(Tensor s, Tensor t, Tensor? row_mask, float beta, float inv_temp) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("gjsd_bwd(Tensor s, Tensor t, Tensor s_lse, Tensor t_lse, Tensor aux, Tensor? row_mask, Tensor grad, float beta, float inv_temp) -> Tensor");
  m.def("adamw_step(Tensor(a!)? param, Tensor(b!)? master, Tensor grad, Tensor(c!) m, Tensor(d!) v, float lr, float b1, float b2, float eps, float wd, int step, Tensor? clip, float grad_scale) -> ()");
  m.def("grad_sumsq(Tensor grad, Tensor(a!) out, bool accumulate) -> ()");
  m.def("clip_coef(Tensor sumsq, float max_norm) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("norm_fwd", &dla::norm_fwd);
  m.impl("norm_bwd", &dla::norm_bwd);
  m.impl("swiglu_fwd", &dla::swiglu_fwd);
  m.impl("swiglu_bwd", &dla::swiglu_bwd);
  m.impl("swiglu_fwd_t", &dla::swiglu_fwd_t);
  m.impl("swiglu_bwd_t", &dla::swiglu_bwd_t);
  m.impl("gelu_fwd", &dla::gelu_fwd);
  m.impl("gelu_bwd", &dla::gelu_bwd);
  m.impl("rope_fwd", &dla::rope_fwd);
  m.impl("rope_bwd", &dla::rope_bwd);
  m.impl("transpose_bf16", &dla::transpose_bf16);
  m.impl("gjsd_fwd", &dla::gjsd_fwd);
  m.impl("gjsd_bwd", &dla::gjsd_bwd);
  m.impl("adamw_step", &dla::adamw_step);
  m.impl("grad_sumsq", &dla::grad_sumsq);
  m.impl("clip_coef", &dla::clip_coef);
}
