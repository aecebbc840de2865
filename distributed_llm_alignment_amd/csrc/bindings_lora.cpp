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

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("lora_shrink(Tensor x, Tensor a, float scale) -> Tensor");
  m.def("lora_expand_add_(Tensor(a!) y, Tensor t, Tensor b, float scale, bool transposed=False) -> ()");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("lora_shrink", &dla::lora_shrink);
  m.impl("lora_expand_add_", &dla::lora_expand_add_);
}
