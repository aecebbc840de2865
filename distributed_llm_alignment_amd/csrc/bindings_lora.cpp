// torch.ops.dla LoRA adapter ops (kernels in lora.hip). Host-side validation only; both are
// graph-capture safe (output from the caching allocator, no workspace, no host sync).
#include <ATen/ATen.h>
#include <torch/library.h>

#include "bind_util.h"

namespace dla {

void launch_lora_shrink(const bf16_t*, int64_t, const bf16_t*, int64_t, bf16_t*, int64_t, int64_t, int,
                        int, float, hipStream_t);
void launch_lora_expand_add(bf16_t*, int64_t, const bf16_t*, int64_t, const bf16_t*, int64_t, bool,
                            int64_t, int, int, float, hipStream_t);
void launch_lora_tile_weight(const bf16_t*, int64_t, const bf16_t*, const bf16_t*, int64_t, int, float,
                             const bf16_t*, bf16_t*, int, int, bool, hipStream_t);
void launch_lora_quant_tile_f8(const bf16_t*, int64_t, const bf16_t*, const bf16_t*, int64_t, int, float,
                               const bf16_t*, uint8_t*, float*, int, int, bool, hipStream_t);
void launch_transpose_bf16(const bf16_t*, int64_t, int64_t, int64_t, bf16_t*, int64_t, hipStream_t);

static bool lora_rank_ok(int64_t r) { return r == 8 || r == 16 || r == 32 || r == 64; }

// [rows, cols] bf16 with unit inner stride, cols % 8 == 0, 16-byte aligned base and rows
static void check_rows16(const at::Tensor& t, const char* name) {
  check_bf16(t, name);
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) % 8 == 0 && t.size(1) % 8 == 0 &&
                  t.stride(0) >= t.size(1),
              name, ": 2-D, unit inner stride, width % 8 == 0, 16-byte aligned rows");
  check_aligned16(t, name);
}

// t [M, R] = bf16(scale * x [M, K] . a [R, K]^T)
at::Tensor lora_shrink(const at::Tensor& x, const at::Tensor& a, double scale) {
  check_rows16(x, "x");
  check_rows16(a, "a");
  same_device(x, a);
  const int64_t M = x.size(0), K = x.size(1), R = a.size(0);
  TORCH_CHECK(a.size(1) == K, "x [M, K], a [R, K]");
  TORCH_CHECK(lora_rank_ok(R), "rank must be 8, 16, 32 or 64");
  TORCH_CHECK(K >= 8 && K < (1ll << 30), "K out of range");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  auto t = at::empty({M, R}, x.options());
  launch_lora_shrink(cbp(x), x.stride(0), cbp(a), a.stride(0), bp(t), R, M, (int)K, (int)R,
                     static_cast<float>(scale), cur_stream(x));
  return t;
}

// y [M, N] += scale * t [M, R] . b^T in place, one rounding; b is [N, R], or [R, N] with
// `transposed` (any row stride there: that layout is read with 2-byte loads)
void lora_expand_add_(at::Tensor& y, const at::Tensor& t, const at::Tensor& b, double scale,
                      bool transposed) {
  check_rows16(y, "y");
  check_rows16(t, "t");
  same_device(y, t);
  same_device(y, b);
  const int64_t M = y.size(0), N = y.size(1), R = t.size(1);
  TORCH_CHECK(t.size(0) == M, "y [M, N], t [M, R]");
  TORCH_CHECK(lora_rank_ok(R), "rank must be 8, 16, 32 or 64");
  TORCH_CHECK(N >= 8 && N < (1ll << 22), "N out of range");
  if (transposed) {
    check_bf16(b, "b");
    TORCH_CHECK(b.dim() == 2 && b.size(0) == R && b.size(1) == N && b.stride(1) == 1 && b.stride(0) >= N,
                "b [R, N] with unit inner stride");
  } else {
    check_rows16(b, "b");
    TORCH_CHECK(b.size(0) == N && b.size(1) == R, "b [N, R]");
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(y.device());
  launch_lora_expand_add(bp(y), y.stride(0), cbp(t), t.stride(0), cbp(b), b.stride(0), transposed, M,
                         (int)N, (int)R, static_cast<float>(scale), cur_stream(y));
}

// ---- decode weight copies from W + scale B A in one pass (kernels in skinny64.hip) ----
// Shared checks; returns A^T [K, R] contiguous (r K elements per refresh; the refresh never runs
// inside a graph capture, ops/decode.py _cached).
static at::Tensor merged_operands(const at::Tensor& w, const at::Tensor& a, const at::Tensor& b,
                                  const c10::optional<at::Tensor>& nw, bool glu_il, int64_t kmult,
                                  const bf16_t** nwp) {
  check_bf16(w, "w");
  TORCH_CHECK(w.dim() == 2 && w.stride(1) == 1 && w.stride(0) % 8 == 0 && w.stride(0) >= w.size(1),
              "w [N, K], unit inner stride, row stride % 8 == 0");
  check_aligned16(w, "w");
  check_rows16(a, "a");
  check_rows16(b, "b");
  same_device(w, a);
  same_device(w, b);
  const int64_t N = w.size(0), K = w.size(1), R = a.size(0);
  TORCH_CHECK(lora_rank_ok(R), "rank must be 8, 16, 32 or 64");
  TORCH_CHECK(a.size(1) == K && b.size(0) == N && b.size(1) == R, "w [N, K], a [R, K], b [N, R]");
  TORCH_CHECK(N > 0 && N % 16 == 0 && K > 0 && K % kmult == 0 && N < (1ll << 30) && K < (1ll << 30),
              "N % 16 == 0, K % ", kmult, " == 0");
  TORCH_CHECK(!glu_il || (N / 2) % 8 == 0, "glu_il: N = 2F, F % 8 == 0");
  *nwp = nullptr;
  if (nw.has_value() && nw->defined()) {
    check_bf16(*nw, "nw");
    TORCH_CHECK(nw->dim() == 1 && nw->size(0) == K && nw->is_contiguous(), "nw [K] contiguous");
    check_aligned16(*nw, "nw");
    same_device(w, *nw);
    *nwp = cbp(*nw);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(w.device());
  auto at_ = at::empty({K, R}, a.options());
  launch_transpose_bf16(cbp(a), R, K, a.stride(0), bp(at_), R, cur_stream(w));
  return at_;
}

void lora_tile_weight(const at::Tensor& w, const at::Tensor& a, const at::Tensor& b, double scale,
                      const c10::optional<at::Tensor>& nw, at::Tensor& out, bool glu_il) {
  const bf16_t* np = nullptr;
  const at::Tensor at_ = merged_operands(w, a, b, nw, glu_il, 32, &np);
  const int64_t N = w.size(0), K = w.size(1);
  check_bf16(out, "out");
  TORCH_CHECK(out.dim() == 5 && out.size(0) == N / 16 && out.size(1) == K / 32 && out.size(2) == 4 &&
                  out.size(3) == 16 && out.size(4) == 8 && out.is_contiguous(),
              "out [N/16, K/32, 4, 16, 8] contiguous");
  check_aligned16(out, "out");
  same_device(w, out);
  c10::hip::HIPGuardMasqueradingAsCUDA g(w.device());
  launch_lora_tile_weight(cbp(w), w.stride(0), cbp(at_), cbp(b), b.stride(0), (int)a.size(0),
                          static_cast<float>(scale), np, bp(out), (int)N, (int)K, glu_il, cur_stream(w));
}

void lora_quant_tile_f8(const at::Tensor& w, const at::Tensor& a, const at::Tensor& b, double scale,
                        const c10::optional<at::Tensor>& nw, at::Tensor& out8, at::Tensor& scale_out,
                        bool glu_il) {
  const bf16_t* np = nullptr;
  const at::Tensor at_ = merged_operands(w, a, b, nw, glu_il, 64, &np);
  const int64_t N = w.size(0), K = w.size(1);
  check_cuda(out8, "out8");
  TORCH_CHECK(out8.scalar_type() == at::kByte && out8.is_contiguous() && out8.dim() == 4 &&
                  out8.size(0) == N / 16 && out8.size(1) == K / 64 && out8.size(2) == 64 && out8.size(3) == 16,
              "out8 uint8 [N/16, K/64, 64, 16] contiguous");
  check_f32(scale_out, "scale_out");
  TORCH_CHECK(scale_out.is_contiguous() && scale_out.dim() == 1 && scale_out.size(0) == N, "scale_out fp32 [N]");
  check_aligned16(out8, "out8");
  same_device(w, out8);
  same_device(w, scale_out);
  c10::hip::HIPGuardMasqueradingAsCUDA g(w.device());
  launch_lora_quant_tile_f8(cbp(w), w.stride(0), cbp(at_), cbp(b), b.stride(0), (int)a.size(0),
                            static_cast<float>(scale), np, out8.data_ptr<uint8_t>(), scale_out.data_ptr<float>(),
                            (int)N, (int)K, glu_il, cur_stream(w));
}

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("lora_tile_weight(Tensor w, Tensor a, Tensor b, float scale, Tensor? nw, Tensor(a!) out, "
        "bool glu_il=False) -> ()");
  m.def("lora_quant_tile_f8(Tensor w, Tensor a, Tensor b, float scale, Tensor? nw, Tensor(a!) out8, "
        "Tensor(b!) scale_out, bool glu_il=False) -> ()");
  m.def("lora_shrink(Tensor x, Tensor a, float scale) -> Tensor");
  m.def("lora_expand_add_(Tensor(a!) y, Tensor t, Tensor b, float scale, bool transposed=False) -> ()");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("lora_shrink", &dla::lora_shrink);
  m.impl("lora_expand_add_", &dla::lora_expand_add_);
  m.impl("lora_tile_weight", &dla::lora_tile_weight);
  m.impl("lora_quant_tile_f8", &dla::lora_quant_tile_f8);
}
