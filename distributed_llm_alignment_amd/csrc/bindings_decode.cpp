// torch.ops.dla decode-path ops: split-KV decode attention (decode.hip), the decode projection
// GEMMs with their weight re-layout passes (skinny.hip, skinny64.hip) and the fused sampler
// (sampling.hip). Host-side validation only; all are graph-capture safe (device-side lengths
// and RNG counter, outputs and workspaces from the caching allocator, no host sync).
#include <ATen/ATen.h>
#include <torch/library.h>

#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

#include "bind_util.h"
#include "decode_params.h"
#include "skinny_geom.h"
#include "skinny_params.h"

namespace dla {

void launch_sample(const void*, bool, int64_t, int64_t, int, float, int, float, bool,
                   const int64_t*, int64_t*, hipStream_t);
int sample_split_chunks(const void*, int64_t, int64_t, int, float, int, float, bool);
size_t sample_workspace_bytes(int64_t, int);
void launch_sample_split(const void*, bool, int64_t, int64_t, int, int, float, int, float,
                         const int64_t*, int64_t*, void*, hipStream_t);
void launch_sample_logp(const void*, bool, int64_t, int64_t, int, float, int, float, bool,
                        const int64_t*, int64_t*, float*, hipStream_t);
size_t sample_workspace_bytes_logp(int64_t, int);
void launch_sample_logp_tempered(const void*, bool, int64_t, int64_t, int, float, int, float, const int64_t*,
                                 int64_t*, float*, hipStream_t);
void launch_sample_split_logp_tempered(const void*, bool, int64_t, int64_t, int, int, float, int, float,
                                       const int64_t*, int64_t*, float*, void*, hipStream_t);
void launch_sample_split_logp(const void*, bool, int64_t, int64_t, int, int, float, int, float,
                              const int64_t*, int64_t*, float*, void*, hipStream_t);
void launch_sample_keep(const void*, bool, int64_t, int64_t, int, int, float, int, float, const int64_t*,
                        int64_t*, float*, uint8_t*, void*, hipStream_t);

void launch_kv_replicate(const bf16_t*, const bf16_t*, bf16_t*, bf16_t*, int, int, int, int, int,
                         int, const int64_t*, const int64_t*, hipStream_t);

// ---- decode projection ops (skinny.hip at M <= 16, skinny64.hip at 17..64 rows): argument
// checks shared by the ops, one fill-and-launch routine per bf16 / fp8 pair

// x [M, K] bf16 with 1 <= M <= max_rows
static void fill_x(SkinnyParams& p, const at::Tensor& x, int64_t max_rows, int64_t width) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1 && x.stride(0) % 8 == 0,
              "x [M, K]: unit inner stride, 16-byte aligned rows");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= max_rows && x.size(1) == width, "x [M, K]: 1 <= M <= ", max_rows,
              ", width K (2K with swiglu)");
  check_aligned16(x, "x");
  p.x = cbp(x);
  p.ldx = x.stride(0);
  p.M = static_cast<int>(x.size(0));
}

// bf16 weight: [N, K] row-major (unit inner stride, 16-byte aligned rows) and / or the tiled
// layout [N/16, K/32, 4, 16, 8] (skinny64.hip TW), as the op takes
static void fill_w(SkinnyParams& p, const at::Tensor& x, const at::Tensor& w, bool row_major, bool tiled) {
  check_bf16(w, "w");
  const bool tw = w.dim() == 5;
  TORCH_CHECK(tw ? (tiled && w.size(2) == 4 && w.size(3) == 16 && w.size(4) == 8 && w.is_contiguous())
                 : (row_major && w.dim() == 2 && w.stride(1) == 1 && w.stride(0) % 8 == 0),
              "w [N, K] (unit inner stride, 16-byte aligned rows) or tiled [N/16, K/32, 4, 16, 8] contiguous");
  const int64_t N = tw ? w.size(0) * 16 : w.size(0), K = tw ? w.size(1) * 32 : w.size(1);
  TORCH_CHECK(N < (1ll << 30) && K < (1ll << 30), "shape too large");
  check_aligned16(w, "w");
  same_device(x, w);
  p.w = w.data_ptr();
  p.layout = tw ? SkinnyW::kTiled : SkinnyW::kRowMajor;
  p.ldw = tw ? K : w.stride(0);
  p.N = static_cast<int>(N);
  p.K = static_cast<int>(K);
}

// fp8 weight-only decode projections (ops/decode.py fp8_tiled_weight): w8 = e4m3 tiled copy
// [N/16, K/64, 64, 16] (uint8 storage), wscale [N] fp32 per weight row
static void check_w8(const at::Tensor& w8, const at::Tensor& wscale, const at::Tensor& x, int64_t* N,
                     int64_t* K) {
  check_cuda(w8, "w8");
  TORCH_CHECK(w8.scalar_type() == at::kByte && w8.dim() == 4 && w8.size(2) == 64 && w8.size(3) == 16 &&
                  w8.is_contiguous(),
              "w8 uint8 [N/16, K/64, 64, 16] contiguous");
  *N = w8.size(0) * 16;
  *K = w8.size(1) * 64;
  check_cuda(wscale, "wscale");
  TORCH_CHECK(wscale.scalar_type() == at::kFloat && wscale.dim() == 1 && wscale.size(0) == *N &&
                  wscale.is_contiguous(),
              "wscale fp32 [N] contiguous");
  check_aligned16(w8, "w8");
  same_device(x, w8);
  same_device(x, wscale);
}

static void fill_w8(SkinnyParams& p, const at::Tensor& x, const at::Tensor& w8, const at::Tensor& wscale) {
  int64_t N = 0, K = 0;
  check_w8(w8, wscale, x, &N, &K);
  TORCH_CHECK(N < (1ll << 30) && K < (1ll << 30), "shape too large");
  p.w = w8.data_ptr();
  p.layout = SkinnyW::kTiledF8;
  p.ldw = K;
  p.wscale = wscale.data_ptr<float>();
  p.N = static_cast<int>(N);
  p.K = static_cast<int>(K);
}

// the producer's row-norm partials: fp32 [rows, nbp <= max_nbp], rows = 16 (skinny.hip) or M
static void fill_ssq_in(SkinnyParams& p, const at::Tensor& x, const at::Tensor& sq, int64_t rows, int64_t max_nbp,
                        double eps) {
  check_cuda(sq, "ssq_in");
  TORCH_CHECK(sq.scalar_type() == at::kFloat && sq.dim() == 2 && sq.size(0) == rows && sq.is_contiguous() &&
                  sq.size(1) >= 1 && sq.size(1) <= max_nbp,
              "ssq_in fp32 [", rows, ", nbp <= ", max_nbp, "] contiguous");
  same_device(x, sq);
  p.ssq_in = sq.data_ptr<float>();
  p.nbp = static_cast<int>(sq.size(1));
  p.eps = static_cast<float>(eps);
}

// res [M, N]; returns the row partials of the new residual stream, fp32 [rows, cols]
static at::Tensor fill_res(SkinnyParams& p, const at::Tensor& x, const at::Tensor& r, int64_t rows, int64_t cols) {
  check_bf16(r, "res");
  TORCH_CHECK(r.dim() == 2 && r.size(0) == p.M && r.size(1) == p.N && r.stride(1) == 1, "res [M, N]");
  same_device(x, r);
  p.res = cbp(r);
  p.ldr = r.stride(0);
  auto ssq = at::empty({rows, cols}, x.options().dtype(at::kFloat));
  p.ssq_out = ssq.data_ptr<float>();
  return ssq;
}

static at::Tensor alloc_y(SkinnyParams& p, const at::Tensor& x) {
  auto y = at::empty({p.M, p.glu_out ? p.N / 2 : p.N}, x.options());
  p.y = bp(y);
  p.ldy = y.stride(0);
  return y;
}

// skinny64 / skinny64_f8 (`p` arrives with the weight set): decode projection at 17..64 rows
// (skinny64.hip), the same fused-layer contract as skinny_fused below with row-norm partials per
// (row, 1024 columns):
//   * plain: y = x w^T;
//   * res given: (s = bf16(bf16(x w^T) + res), ssq [M, ceil(N / 1024)]);
//   * ssq_in given ([M, nbp], nbp <= 64): y = rstd[m] * (x w^T), w with the norm weight folded in;
//     with `glu` the gate|up projection + SwiGLU epilogue (w = [gate; up], output [M, F]).
static std::tuple<at::Tensor, at::Tensor> m64_step(SkinnyParams& p, const at::Tensor& x,
                                                   const c10::optional<at::Tensor>& res,
                                                   const c10::optional<at::Tensor>& ssq_in, double eps, bool glu) {
  fill_x(p, x, 64, p.K);
  TORCH_CHECK(m64_shape_ok(p.N, p.K), "skinny64: K % 256 == 0 and N % 128 == 0");
  if (ssq_in.has_value()) fill_ssq_in(p, x, *ssq_in, p.M, 64, eps);
  TORCH_CHECK(!(res.has_value() && (ssq_in.has_value() || glu)), "skinny64: residual output takes a plain input");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  p.glu_out = glu;
  const int S = m64_num_splits(p);
  TORCH_CHECK(glu || S > 1 || !(ssq_in.has_value() || res.has_value()),
              "skinny64: the residual / normalised-input epilogue needs a split-K shape");
  auto y = alloc_y(p, x);
  at::Tensor ws, ssq;
  if (S > 1) {
    ws = at::empty({S, p.M, p.N}, x.options().dtype(at::kFloat));
    p.ws = ws.data_ptr<float>();
  }
  // row partials per 1024 columns (written by the reduce launch)
  if (res.has_value()) ssq = fill_res(p, x, *res, p.M, (p.N + 1023) / 1024);
  launch_m64(p, cur_stream(x));
  return {y, ssq};
}

std::tuple<at::Tensor, at::Tensor> skinny64(const at::Tensor& x, const at::Tensor& w,
                                            const c10::optional<at::Tensor>& res,
                                            const c10::optional<at::Tensor>& ssq_in, double eps,
                                            bool glu) {
  SkinnyParams p{};
  fill_w(p, x, w, true, true);
  return m64_step(p, x, res, ssq_in, eps, glu);
}

// fp8 form of skinny64: w8 the e4m3 tiled copy with per-row scales `wscale` (gate|up: the plain
// [gate; up] row order, norm weight folded in)
std::tuple<at::Tensor, at::Tensor> skinny64_f8(const at::Tensor& x, const at::Tensor& w8, const at::Tensor& wscale,
                                               const c10::optional<at::Tensor>& res,
                                               const c10::optional<at::Tensor>& ssq_in, double eps, bool glu) {
  SkinnyParams p{};
  fill_w8(p, x, w8, wscale);
  return m64_step(p, x, res, ssq_in, eps, glu);
}

// out <- w [N, K] in the tiled decode layout [N/16, K/32, 4, 16, 8] (nw given: bf16(w * nw), the
// RMSNorm weight folded into the input columns)
void tile_weight(const at::Tensor& w, const c10::optional<at::Tensor>& nw, at::Tensor& out, bool glu_il) {
  check_bf16(w, "w");
  check_bf16(out, "out");
  TORCH_CHECK(w.dim() == 2 && w.stride(1) == 1 && w.stride(0) % 8 == 0, "w [N, K], unit inner stride");
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(N % 16 == 0 && K % 32 == 0 && N < (1ll << 30) && K < (1ll << 30), "N % 16 == 0, K % 32 == 0");
  TORCH_CHECK(!glu_il || N % 32 == 0, "glu_il: N = 2F, F % 16 == 0");
  TORCH_CHECK(out.dim() == 5 && out.size(0) == N / 16 && out.size(1) == K / 32 && out.size(2) == 4 &&
                  out.size(3) == 16 && out.size(4) == 8 && out.is_contiguous(),
              "out [N/16, K/32, 4, 16, 8] contiguous");
  check_aligned16(w, "w");
  check_aligned16(out, "out");
  same_device(w, out);
  const bf16_t* np = nullptr;
  if (nw.has_value()) {
    check_bf16(*nw, "nw");
    TORCH_CHECK(nw->dim() == 1 && nw->size(0) == K && nw->is_contiguous(), "nw [K]");
    check_aligned16(*nw, "nw");
    same_device(w, *nw);
    np = cbp(*nw);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(w.device());
  launch_tile_weight(cbp(w), w.stride(0), np, bp(out), (int)N, (int)K, glu_il, cur_stream(w));
}

// w [N, K] bf16 (+ nw folded, glu_il interleave) -> out8 uint8 [N/16, K/64, 64, 16] e4m3 tiled
// and scale fp32 [N] (per tiled row), in place (a captured decode graph keeps reading them)
void quant_tile_f8(const at::Tensor& w, const c10::optional<at::Tensor>& nw, at::Tensor& out8, at::Tensor& scale,
                   bool glu_il) {
  check_bf16(w, "w");
  TORCH_CHECK(w.dim() == 2 && w.stride(1) == 1 && w.stride(0) % 8 == 0, "w [N, K], unit inner stride");
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(N % 32 == 0 && K % 64 == 0 && N < (1ll << 30) && K < (1ll << 30), "N % 32 == 0, K % 64 == 0");
  check_cuda(out8, "out8");
  TORCH_CHECK(out8.scalar_type() == at::kByte && out8.is_contiguous() && out8.numel() == N * K,
              "out8 uint8 contiguous, N * K bytes");
  check_cuda(scale, "scale");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.is_contiguous() && scale.numel() == N, "scale fp32 [N]");
  check_aligned16(w, "w");
  check_aligned16(out8, "out8");
  same_device(w, out8);
  same_device(w, scale);
  const bf16_t* np = nullptr;
  if (nw.has_value() && nw->defined()) {
    check_bf16(*nw, "nw");
    TORCH_CHECK(nw->dim() == 1 && nw->size(0) == K && nw->is_contiguous(), "nw [K] contiguous");
    same_device(w, *nw);
    np = cbp(*nw);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(w.device());
  launch_quant_tile_f8(cbp(w), w.stride(0), np, out8.data_ptr<uint8_t>(), scale.data_ptr<float>(), (int)N, (int)K,
                       glu_il, cur_stream(w));
}

// skinny_glu_il / skinny_glu_il_f8 (`p` arrives with the weight set): decode gate|up + SwiGLU at
// M <= 16 over the interleaved tiled weight (tile_weight / quant_tile_f8 glu_il, norm folded) from
// the producer's row-norm partials: [M, F] = silu(rstd * g) * (rstd * u)
static at::Tensor glu_il_step(SkinnyParams& p, const at::Tensor& x, const at::Tensor& ssq_in, double eps) {
  fill_x(p, x, 16, p.K);
  TORCH_CHECK(p.K % 512 == 0 && (p.layout != SkinnyW::kTiledF8 || p.N % 32 == 0) &&
                  skinny_lds_bytes(p.M, p.K) <= kSkLdsNormX,
              "skinny_glu_il: K % 512 == 0 (fp8: 2F % 32 == 0), x fits LDS");
  fill_ssq_in(p, x, ssq_in, 16, 512, eps);
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  p.glu_out = true;
  auto m = alloc_y(p, x);
  launch_skinny_glu_il(p, cur_stream(x));
  return m;
}

at::Tensor skinny_glu_il(const at::Tensor& x, const at::Tensor& wt, const at::Tensor& ssq_in, double eps) {
  SkinnyParams p{};
  fill_w(p, x, wt, false, true);
  return glu_il_step(p, x, ssq_in, eps);
}

at::Tensor skinny_glu_il_f8(const at::Tensor& x, const at::Tensor& w8, const at::Tensor& wscale,
                            const at::Tensor& ssq_in, double eps) {
  SkinnyParams p{};
  fill_w8(p, x, w8, wscale);
  return glu_il_step(p, x, ssq_in, eps);
}

// skinny_fused / skinny_fused_f8 (`p` arrives with the weight set): fused decode-layer projection
// (M <= 16, skinny.hip KsFuse):
//   * res given: returns (s = bf16(bf16(x w^T) + res) [M, N], ssq [16, N/16] fp32 partial sums of
//     s^2 per (row, 16-column workgroup)) -- the o / down projection producing the residual;
//   * ssq_in given: x is a residual stream s and w a weight with the RMSNorm weight folded in
//     (w o norm_w, ops/decode.py): returns rstd[m] * (s w^T), rstd = rsqrt(sum(ssq_in[m]) / K +
//     eps) -- RMSNorm(s) @ W^T without a norm launch: the qkv projection, or with `glu` (bf16
//     weights) the gate|up projection with the SwiGLU epilogue (w = [gate; up], output [M, F]).
static std::tuple<at::Tensor, at::Tensor> fused_step(SkinnyParams& p, const at::Tensor& x,
                                                     const c10::optional<at::Tensor>& res,
                                                     const c10::optional<at::Tensor>& ssq_in, double eps, bool glu) {
  fill_x(p, x, 16, p.K);
  if (ssq_in.has_value()) fill_ssq_in(p, x, *ssq_in, 16, 512, eps);
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  if (glu) {
    TORCH_CHECK(ssq_in.has_value() && !res.has_value(), "glu: normalised input, no residual");
    TORCH_CHECK(p.N % 128 == 0 && skinny_lds_bytes(p.M, p.K) <= kSkLdsNormX, "glu: 2F % 128 == 0, x fits LDS");
    p.glu_out = true;
    auto m = alloc_y(p, x);
    launch_skinny_gemm(p, cur_stream(x));
    return {m, at::Tensor()};
  }
  // (a plain fp8 projection -- the LM head -- may be any width: one workgroup per 16 columns)
  const bool wide_ok = p.layout == SkinnyW::kTiledF8 && !res.has_value() && !ssq_in.has_value();
  TORCH_CHECK(wide_ok ? (p.N % 16 == 0 && p.K % 1024 == 0) : skinny_use_ksplit(p.N, p.K),
              "fused skinny: N % 16 == 0, K % 1024 == 0, N < 16384 (but a plain fp8 projection)");
  auto y = alloc_y(p, x);
  at::Tensor ssq;
  if (res.has_value()) ssq = fill_res(p, x, *res, 16, p.N / 16);
  launch_skinny_ksplit(p, true, cur_stream(x));
  return {y, ssq};
}

std::tuple<at::Tensor, at::Tensor> skinny_fused(const at::Tensor& x, const at::Tensor& w,
                                                const c10::optional<at::Tensor>& res,
                                                const c10::optional<at::Tensor>& ssq_in, double eps,
                                                bool glu) {
  SkinnyParams p{};
  fill_w(p, x, w, true, true);
  return fused_step(p, x, res, ssq_in, eps, glu);
}

std::tuple<at::Tensor, at::Tensor> skinny_fused_f8(const at::Tensor& x, const at::Tensor& w8,
                                                   const at::Tensor& wscale,
                                                   const c10::optional<at::Tensor>& res,
                                                   const c10::optional<at::Tensor>& ssq_in, double eps) {
  SkinnyParams p{};
  fill_w8(p, x, w8, wscale);
  return fused_step(p, x, res, ssq_in, eps, false);
}

// Decode gate|up with the SwiGLU epilogue on the in-workgroup split-K kernel: w = [gate; up]
// (2F rows) -> m = silu(x gate^T) * (x up^T) [M, F], one workgroup per 16 features.
at::Tensor skinny_glu_ks(const at::Tensor& x, const at::Tensor& w) {
  SkinnyParams p{};
  fill_w(p, x, w, true, false);
  fill_x(p, x, 64, p.K);
  TORCH_CHECK(skinny_glu_ks_ok(p.N, p.K), "skinny GLU: K % 512 == 0 and 2F % 32 == 0");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  p.glu_out = true;
  auto m = alloc_y(p, x);
  launch_skinny_ksplit(p, false, cur_stream(x));
  return m;
}

// y[M, N] = x[M, K] @ w[N, K]^T for M <= 16 (decode). With `swiglu`, x is the fused gate|up
// output gu[M, 2K] and the kernel applies silu(g) * u while staging it. `counters` (int32,
// zero-initialised once, re-armed by the kernel) holds one split-K arrival counter per 128
// output columns. With `glu_out`, w = [gate; up] (2F rows) -> silu(x gate^T) * (x up^T) [M, F].
at::Tensor skinny_gemm(const at::Tensor& x, const at::Tensor& w, at::Tensor& counters, bool swiglu,
                       bool glu_out) {
  check_i32(counters, "counters");
  SkinnyParams p{};
  fill_w(p, x, w, true, false);
  fill_x(p, x, 64, swiglu ? 2 * p.K : p.K);
  // narrow N, no fused swiglu input: the in-workgroup split-K kernel, the only one at 17..64 rows
  const bool ksplit = !swiglu && !glu_out && skinny_use_ksplit(p.N, p.K);
  TORCH_CHECK(p.M <= 16 || ksplit,
              "skinny GEMM: 1 <= M <= 16 (<= 64 on the split-K path: N < 16384, K % 1024 == 0)");
  TORCH_CHECK(p.K % 256 == 0 && p.N % 16 == 0, "skinny GEMM: K % 256 == 0 and N % 16 == 0");
  same_device(x, counters);
  TORCH_CHECK(counters.is_contiguous() && counters.numel() >= (p.N + 127) / 128, "counters: one per 128 columns");
  p.counters = reinterpret_cast<unsigned*>(counters.data_ptr<int>());
  p.swiglu = swiglu;
  p.glu_out = glu_out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  if (glu_out) {
    TORCH_CHECK(!swiglu && p.N % 128 == 0, "glu_out: 2F rows with F % 64 == 0, no swiglu input");
    TORCH_CHECK(skinny_lds_bytes(p.M, p.K) <= kSkLdsGluMax, "skinny GEMM: x exceeds LDS");
  }
  at::Tensor ws;
  if (!glu_out && !ksplit) {
    const int S = skinny_splits(p.M, p.N, p.K);
    TORCH_CHECK(skinny_lds_bytes(p.M, p.K / S) <= kSkLdsMax, "skinny GEMM: x slice exceeds LDS");
    if (S > 1) {
      ws = at::empty({S, p.M, p.N}, x.options().dtype(at::kFloat));
      p.ws = ws.data_ptr<float>();
    }
  }
  auto y = alloc_y(p, x);
  if (ksplit) launch_skinny_ksplit(p, false, cur_stream(x));
  else launch_skinny_gemm(p, cur_stream(x));
  return y;
}

// Per-device arrival counters of the in-kernel split combine (decode.hip dec_arrive_combine):
// zeroed once here, re-armed to 0 by the block that combines. Created only outside a stream
// capture (generation runs an eager decode step before capturing); nullptr -> the combine launch.
// One buffer per device: two decode attention kernels must not run concurrently on one device.
// DLA_DECODE_FUSED_COMBINE=0 keeps the separate combine launch.
constexpr int64_t kDecCounters = 4096;
static int* decode_counters(const at::Tensor& like, int64_t n) {
  static const bool on = [] {
    const char* e = std::getenv("DLA_DECODE_FUSED_COMBINE");
    return !(e != nullptr && std::atoi(e) == 0);
  }();
  if (!on || n > kDecCounters) return nullptr;
  static auto* bufs = new std::map<int, at::Tensor>();  // never destroyed (outlives the allocator)
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  const int dev = like.get_device();
  auto it = bufs->find(dev);
  if (it != bufs->end()) return it->second.data_ptr<int>();
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(cur_stream(like), &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
    return nullptr;
  auto t = at::zeros({kDecCounters}, like.options().dtype(at::kInt));
  bufs->emplace(dev, t);
  return t.data_ptr<int>();
}

// ---- decode attention ops: argument checks shared by the forms, one fill-and-launch routine

// k / v caches [B, Tmax, Hkv, D] sharing strides, head dim contiguous
static void check_kv_caches(const at::Tensor& k_cache, const at::Tensor& v_cache, int64_t B, int64_t Hkv,
                            int64_t D) {
  check_bf16(k_cache, "k_cache");
  check_bf16(v_cache, "v_cache");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == B && k_cache.size(2) == Hkv &&
                  k_cache.size(3) == D && k_cache.sizes() == v_cache.sizes() &&
                  k_cache.strides() == v_cache.strides() && k_cache.stride(3) == 1,
              "caches [B, Tmax, Hkv, D]: cache batch / head dim, k/v caches must share strides");
  check_aligned16(k_cache, "k_cache");
  check_aligned16(v_cache, "v_cache");
}

// The raw-qkv rope step: qkv [B, 1, (Hq + 2 Hkv) D] rows of the newest token, fp32 tables
// [max_pos, rot / 2], pos int32 [B], slot int64 [1] on the device
static void check_rope_step(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                            const at::Tensor& pos, const at::Tensor& slot, int64_t Hq, int64_t Hkv,
                            int64_t D, int64_t rot) {
  check_bf16(qkv, "qkv");
  check_f32(cos, "cos");
  check_f32(sin, "sin");
  check_i32(pos, "pos");
  check_cuda(slot, "slot");
  TORCH_CHECK(slot.scalar_type() == at::kLong && slot.numel() >= 1, "slot int64");
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(1) == 1 && qkv.size(2) == (Hq + 2 * Hkv) * D &&
                  qkv.stride(2) == 1 && qkv.stride(0) % 8 == 0,
              "qkv [B, 1, (Hq+2Hkv)D] with 16-byte aligned rows");
  TORCH_CHECK(rot % 16 == 0 && rot <= D, "rot % 16 == 0, rot <= D");
  TORCH_CHECK(cos.is_contiguous() && sin.is_contiguous() && cos.size(-1) == rot / 2, "rope tables");
  TORCH_CHECK(pos.numel() == qkv.size(0) && pos.is_contiguous(), "pos [B]");
  check_aligned16(qkv, "qkv");
}

// What the four decode attention ops share: cache / kv_len / kv_start / GQA / head-dim checks,
// the group arguments, then partials + output, the rest of `p` and the launch. `x` is q or qkv;
// `p` arrives with q (or rope) set.
static at::Tensor decode_step(const at::Tensor& x, DecodeParams& p, const at::Tensor& k_cache,
                              const at::Tensor& v_cache, const at::Tensor& kv_len,
                              const c10::optional<at::Tensor>& kv_start, int64_t window, double scale,
                              int64_t B, int64_t Hq, int64_t Hkv, int64_t D, bool grouped,
                              int64_t group_size, int64_t prefix_len) {
  check_kv_caches(k_cache, v_cache, B, Hkv, D);
  check_i32(kv_len, "kv_len");
  TORCH_CHECK(D == 64 || D == 128, "decode attention supports head_dim 64 or 128");
  TORCH_CHECK(Hq % Hkv == 0, "Hq % Hkv");
  const int64_t GQ = Hq / Hkv;
  TORCH_CHECK(GQ == 1 || GQ == 2 || GQ == 4 || GQ == 8, "GQA group size must be 1, 2, 4 or 8");
  TORCH_CHECK(k_cache.stride(1) % 8 == 0 && k_cache.stride(2) % 8 == 0 && k_cache.stride(0) % 8 == 0,
              "16-byte aligned cache rows");
  if (kv_start && kv_start->defined()) {
    check_i32(*kv_start, "kv_start");
    TORCH_CHECK(kv_start->numel() == B && kv_start->is_contiguous(), "kv_start [B]");
    p.kv_start = kv_start->data_ptr<int>();
  }
  const int64_t Tmax = k_cache.size(1);
  if (grouped) {
    TORCH_CHECK(group_size >= 1 && B % group_size == 0, "group_size must divide the batch");
    TORCH_CHECK(prefix_len >= 1 && prefix_len <= Tmax, "1 <= prefix_len <= Tmax");
    p.G = static_cast<int>(group_size);
    p.Tp = static_cast<int>(prefix_len);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  p.kc = bp(k_cache);
  p.vc = bp(v_cache);
  p.c_sb = k_cache.stride(0);
  p.c_st = k_cache.stride(1);
  p.c_sh = k_cache.stride(2);
  p.kv_len = kv_len.data_ptr<int>();
  p.window = static_cast<int>(window);
  p.scale_log2 = static_cast<float>(scale * 1.4426950408889634);
  p.B = static_cast<int>(B);
  p.Hq = static_cast<int>(Hq);
  p.Hkv = static_cast<int>(Hkv);
  p.D = static_cast<int>(D);
  p.Tmax = static_cast<int>(Tmax);
  const int nsplit = decode_splits(p);
  auto fopt = x.options().dtype(at::kFloat);
  auto part_o = at::empty({B, Hq, nsplit, D}, fopt);
  auto part_ml = at::empty({B, Hq, nsplit, 2}, fopt);
  auto out = at::empty({B, Hq, D}, x.options());
  p.part_o = part_o.data_ptr<float>();
  p.part_ml = part_ml.data_ptr<float>();
  p.out = bp(out);
  p.o_sb = out.stride(0);
  p.o_sh = out.stride(1);
  p.cnt = decode_counters(x, B * Hkv);
  launch_decode(p, cur_stream(x));
  return out;
}

// q [B, Hq, D] already rotated, the newest token already in the caches
static at::Tensor decode_q(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                           const at::Tensor& kv_len, const c10::optional<at::Tensor>& kv_start,
                           int64_t window, double scale, bool grouped, int64_t group_size,
                           int64_t prefix_len) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4, "q [B, Hq, D], caches [B, Tmax, Hkv, D]");
  TORCH_CHECK(q.stride(2) == 1, "head dim must be contiguous");
  TORCH_CHECK(q.stride(1) % 8 == 0, "16-byte aligned rows");
  TORCH_CHECK(kv_len.numel() >= 1, "kv_len");
  DecodeParams p{};
  p.q = cbp(q);
  p.q_sb = q.stride(0);
  p.q_sh = q.stride(1);
  return decode_step(q, p, k_cache, v_cache, kv_len, kv_start, window, scale, q.size(0), q.size(1),
                     k_cache.size(2), q.size(2), grouped, group_size, prefix_len);
}

// One decode step's attention with the rope + cache write of the newest token fused in (one
// launch pair instead of rope_cache_write + decode_attn): qkv [B, 1, (Hq + 2 Hkv) D] raw row,
// caches [B, Tmax, Hkv, D] (row `slot` is written), kv_len = slot + 1 (device).
static at::Tensor decode_qkv(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                             const at::Tensor& pos, const at::Tensor& k_cache, const at::Tensor& v_cache,
                             const at::Tensor& slot, const at::Tensor& kv_len,
                             const c10::optional<at::Tensor>& kv_start, int64_t window, double scale,
                             int64_t Hq, int64_t Hkv, int64_t D, int64_t rot, bool grouped,
                             int64_t group_size, int64_t prefix_len) {
  check_rope_step(qkv, cos, sin, pos, slot, Hq, Hkv, D, rot);
  TORCH_CHECK(rot > 0, "rot % 16 == 0, 0 < rot <= D");
  DecodeParams p{};
  p.rope = DecRope{cbp(qkv), qkv.stride(0), cos.data_ptr<float>(), sin.data_ptr<float>(),
                   pos.data_ptr<int>(), slot.data_ptr<int64_t>(), static_cast<int>(rot),
                   static_cast<int>(Hkv)};
  return decode_step(qkv, p, k_cache, v_cache, kv_len, kv_start, window, scale, qkv.size(0), Hq, Hkv, D,
                     grouped, group_size, prefix_len);
}

at::Tensor decode_attn(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                       const at::Tensor& kv_len, const c10::optional<at::Tensor>& kv_start,
                       int64_t window, double scale) {
  return decode_q(q, k_cache, v_cache, kv_len, kv_start, window, scale, false, 0, 0);
}

at::Tensor decode_attn_rope(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                            const at::Tensor& pos, at::Tensor& k_cache, at::Tensor& v_cache,
                            const at::Tensor& slot, const at::Tensor& kv_len,
                            const c10::optional<at::Tensor>& kv_start, int64_t window, double scale,
                            int64_t Hq, int64_t Hkv, int64_t D, int64_t rot) {
  return decode_qkv(qkv, cos, sin, pos, k_cache, v_cache, slot, kv_len, kv_start, window, scale, Hq, Hkv,
                    D, rot, false, 0, 0);
}

// Group-structured forms of decode_attn / decode_attn_rope (decode.hip DecGroup): rows
// p * G .. p * G + G - 1 share prompt p, and keys [kv_start, prefix_len) are read from row p * G
// only, once per (prompt, kv head) for the whole group. Preconditions (not checked on the device):
// the G rows of a group hold identical K / V in [0, prefix_len), share kv_start < prefix_len, and
// kv_len > prefix_len. decode_attn_rope_group with kv_len <= prefix_len (the newest token's slot
// below the prefix boundary) is undefined: the suffix launch owns only chunks from
// prefix_len / 128 on, so a slot below them is never written, and the prefix launch reads whatever
// that slot held before. KVCache.attend refuses that state on the host.
at::Tensor decode_attn_group(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                             const at::Tensor& kv_len, const c10::optional<at::Tensor>& kv_start,
                             int64_t window, double scale, int64_t group_size, int64_t prefix_len) {
  return decode_q(q, k_cache, v_cache, kv_len, kv_start, window, scale, true, group_size, prefix_len);
}

at::Tensor decode_attn_rope_group(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                                  const at::Tensor& pos, at::Tensor& k_cache, at::Tensor& v_cache,
                                  const at::Tensor& slot, const at::Tensor& kv_len,
                                  const c10::optional<at::Tensor>& kv_start, int64_t window, double scale,
                                  int64_t Hq, int64_t Hkv, int64_t D, int64_t rot, int64_t group_size,
                                  int64_t prefix_len) {
  return decode_qkv(qkv, cos, sin, pos, k_cache, v_cache, slot, kv_len, kv_start, window, scale, Hq, Hkv,
                    D, rot, true, group_size, prefix_len);
}

// qkv [B, 1, (Hq + 2 Hkv) D] of the newest token -> rotated q [B, Hq, D]; k/v written into
// k_cache/v_cache [B, Tmax, Hkv, D] at row `slot` (int64 [1] on device). Any D % 8 == 0 (phi-2's
// D = 80), rot = 0 allowed.
at::Tensor rope_cache_write(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                            const at::Tensor& pos, at::Tensor& k_cache, at::Tensor& v_cache,
                            const at::Tensor& slot, int64_t Hq, int64_t Hkv, int64_t D, int64_t rot) {
  TORCH_CHECK(D % 8 == 0, "D % 8");
  check_rope_step(qkv, cos, sin, pos, slot, Hq, Hkv, D, rot);
  const int64_t B = qkv.size(0);
  check_kv_caches(k_cache, v_cache, B, Hkv, D);
  c10::hip::HIPGuardMasqueradingAsCUDA g(qkv.device());
  auto q = at::empty({B, Hq, D}, qkv.options());
  launch_rope_cache(cbp(qkv), qkv.stride(0), bp(q), bp(k_cache), bp(v_cache), k_cache.stride(0),
                    k_cache.stride(1), k_cache.stride(2), slot.data_ptr<int64_t>(),
                    cos.data_ptr<float>(), sin.data_ptr<float>(), pos.data_ptr<int>(), (int)B,
                    (int)Hq, (int)Hkv, (int)D, (int)rot, cur_stream(qkv));
  return q;
}

static void check_sample_args(const at::Tensor& logits, double top_p, const at::Tensor& rng) {
  check_cuda(logits, "logits");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat,
              "logits must be bf16 or fp32");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1, "logits [B, V] with unit vocab stride");
  check_cuda(rng, "rng");
  TORCH_CHECK(rng.scalar_type() == at::kLong && rng.numel() >= 2, "rng int64 [seed, counter]");
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "top_p in (0, 1]");
  TORCH_CHECK(logits.size(1) < (1ll << 31), "vocab too large");
}

at::Tensor sample_tokens(const at::Tensor& logits, double temperature, int64_t top_k,
                         double top_p, bool greedy, const at::Tensor& rng) {
  check_sample_args(logits, top_p, rng);
  const int64_t B = logits.size(0), V = logits.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  const float inv_t = temperature > 0.0 ? static_cast<float>(1.0 / temperature) : 0.f;
  const bool is_bf16 = logits.scalar_type() == at::kBFloat16;
  const int G = sample_split_chunks(logits.data_ptr(), logits.stride(0), B, (int)V, inv_t,
                                    (int)top_k, static_cast<float>(top_p), greedy);
  if (G > 0) {  // top-k / top-p on a large vocabulary: row-split multi-launch sampler
    auto ws = at::empty({(int64_t)sample_workspace_bytes(B, G)}, logits.options().dtype(at::kByte));
    launch_sample_split(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, G, inv_t,
                        (int)top_k, static_cast<float>(top_p), rng.data_ptr<int64_t>(),
                        out.data_ptr<int64_t>(), ws.data_ptr(), cur_stream(logits));
    return out;
  }
  launch_sample(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, inv_t, (int)top_k,
                static_cast<float>(top_p), greedy, rng.data_ptr<int64_t>(),
                out.data_ptr<int64_t>(), cur_stream(logits));
  return out;
}

// sample_tokens plus logp [B] fp32: log softmax(logits)[token] at temperature 1 over the full
// vocabulary (the engine's model log-prob of the draw). Same checks and the same path choice; the
// LOGP kernel instantiations return the tokens of the plain op bit for bit.
std::tuple<at::Tensor, at::Tensor> sample_tokens_logp(const at::Tensor& logits, double temperature,
                                                      int64_t top_k, double top_p, bool greedy,
                                                      const at::Tensor& rng) {
  check_sample_args(logits, top_p, rng);
  const int64_t B = logits.size(0), V = logits.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  auto logp = at::empty({B}, logits.options().dtype(at::kFloat));
  const float inv_t = temperature > 0.0 ? static_cast<float>(1.0 / temperature) : 0.f;
  const bool is_bf16 = logits.scalar_type() == at::kBFloat16;
  const int G = sample_split_chunks(logits.data_ptr(), logits.stride(0), B, (int)V, inv_t,
                                    (int)top_k, static_cast<float>(top_p), greedy);
  if (G > 0) {
    auto ws = at::empty({(int64_t)sample_workspace_bytes_logp(B, G)},
                        logits.options().dtype(at::kByte));
    launch_sample_split_logp(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, G, inv_t,
                             (int)top_k, static_cast<float>(top_p), rng.data_ptr<int64_t>(),
                             out.data_ptr<int64_t>(), logp.data_ptr<float>(), ws.data_ptr(),
                             cur_stream(logits));
    return {out, logp};
  }
  launch_sample_logp(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, inv_t, (int)top_k,
                     static_cast<float>(top_p), greedy, rng.data_ptr<int64_t>(),
                     out.data_ptr<int64_t>(), logp.data_ptr<float>(), cur_stream(logits));
  return {out, logp};
}

// sample_tokens_logp with the log-prob at the DRAW temperature: logp = log softmax(logits *
// inv_temp)[token] over the full vocabulary (no top-k / top-p filter), the quantity
// token_logprobs(temperature=) returns. Tokens are sample_tokens' bit for bit. greedy or
// temperature <= 0 has no draw temperature: sample_tokens_logp's result.
std::tuple<at::Tensor, at::Tensor> sample_tokens_logp_tempered(const at::Tensor& logits, double temperature,
                                                               int64_t top_k, double top_p, bool greedy,
                                                               const at::Tensor& rng) {
  if (greedy || !(temperature > 0.0)) return sample_tokens_logp(logits, temperature, top_k, top_p, greedy, rng);
  check_sample_args(logits, top_p, rng);
  const int64_t B = logits.size(0), V = logits.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  auto logp = at::empty({B}, logits.options().dtype(at::kFloat));
  const float inv_t = static_cast<float>(1.0 / temperature);
  const bool is_bf16 = logits.scalar_type() == at::kBFloat16;
  const int G = sample_split_chunks(logits.data_ptr(), logits.stride(0), B, (int)V, inv_t,
                                    (int)top_k, static_cast<float>(top_p), greedy);
  if (G > 0) {
    auto ws = at::empty({(int64_t)sample_workspace_bytes_logp(B, G)},
                        logits.options().dtype(at::kByte));
    launch_sample_split_logp_tempered(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, G, inv_t,
                                      (int)top_k, static_cast<float>(top_p), rng.data_ptr<int64_t>(),
                                      out.data_ptr<int64_t>(), logp.data_ptr<float>(), ws.data_ptr(),
                                      cur_stream(logits));
    return {out, logp};
  }
  launch_sample_logp_tempered(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, inv_t, (int)top_k,
                              static_cast<float>(top_p), rng.data_ptr<int64_t>(), out.data_ptr<int64_t>(),
                              logp.data_ptr<float>(), cur_stream(logits));
  return {out, logp};
}

// sample_tokens plus the set every token was drawn from: keep uint8 [B, V / 8], bit j (LSB first) of
// byte i = vocabulary entry 8 i + j kept by the top-k / top-p filter (the z >= -64 window without a
// filter), and logp [B] fp32 = the log-prob under that FILTERED distribution at the draw
// temperature, z_t - log(kept mass). Tokens are sample_tokens' bit for bit; the launch count is
// sample_tokens'. A greedy / temperature <= 0 call has no kept set and is rejected.
std::tuple<at::Tensor, at::Tensor, at::Tensor> sample_tokens_keep(const at::Tensor& logits, double temperature,
                                                                  int64_t top_k, double top_p,
                                                                  const at::Tensor& rng) {
  check_sample_args(logits, top_p, rng);
  TORCH_CHECK(temperature > 0.0, "sample_tokens_keep: temperature must be > 0 (a greedy call has no kept set)");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V % 8 == 0, "sample_tokens_keep: the vocabulary size must be a multiple of 8 (V % 8 == 0), got ", V);
  TORCH_CHECK(logits.stride(0) % 8 == 0, "sample_tokens_keep: the row stride must be a multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
              "sample_tokens_keep: logits must be 16-byte aligned");
  c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  auto logp = at::empty({B}, logits.options().dtype(at::kFloat));
  auto keep = at::empty({B, V / 8}, logits.options().dtype(at::kByte));
  const float inv_t = static_cast<float>(1.0 / temperature);
  const bool is_bf16 = logits.scalar_type() == at::kBFloat16;
  const int G = sample_split_chunks(logits.data_ptr(), logits.stride(0), B, (int)V, inv_t, (int)top_k,
                                    static_cast<float>(top_p), false);
  at::Tensor ws;
  if (G > 0) ws = at::empty({(int64_t)sample_workspace_bytes(B, G)}, logits.options().dtype(at::kByte));
  launch_sample_keep(logits.data_ptr(), is_bf16, logits.stride(0), B, (int)V, G, inv_t, (int)top_k,
                     static_cast<float>(top_p), rng.data_ptr<int64_t>(), out.data_ptr<int64_t>(),
                     logp.data_ptr<float>(), keep.data_ptr<uint8_t>(), G > 0 ? ws.data_ptr() : nullptr,
                     cur_stream(logits));
  return {out, logp, keep};
}

// Shared-prefill replication: keys / values [0, Tp) of every layer of the P-row prefill cache
// (src_k / src_v [L, P, Tp, Hkv, D]) go to rows p*G .. p*G+G-1 of the P*G-row decode cache
// (dst_k / dst_v [L, P*G, Tmax >= Tp, Hkv, D]); any strides with D contiguous and 16-byte
// aligned rows (head-major or token-major storage). Positions >= Tp of dst are not written.
void kv_replicate(const at::Tensor& src_k, const at::Tensor& src_v, at::Tensor& dst_k,
                  at::Tensor& dst_v, int64_t G) {
  check_bf16(src_k, "src_k");
  check_bf16(src_v, "src_v");
  check_bf16(dst_k, "dst_k");
  check_bf16(dst_v, "dst_v");
  same_device(src_k, dst_k);
  same_device(src_v, dst_k);
  same_device(dst_v, dst_k);
  TORCH_CHECK(src_k.dim() == 5 && dst_k.dim() == 5, "kv_replicate: caches are [L, rows, T, Hkv, D]");
  TORCH_CHECK(src_v.sizes() == src_k.sizes() && src_v.strides() == src_k.strides(),
              "kv_replicate: src_k / src_v must share shape and strides");
  TORCH_CHECK(dst_v.sizes() == dst_k.sizes() && dst_v.strides() == dst_k.strides(),
              "kv_replicate: dst_k / dst_v must share shape and strides");
  const int64_t L = src_k.size(0), P = src_k.size(1), Tp = src_k.size(2), H = src_k.size(3),
                D = src_k.size(4);
  TORCH_CHECK(G >= 1 && G < (1 << 20), "kv_replicate: bad group size");
  TORCH_CHECK(dst_k.size(0) == L && dst_k.size(1) == P * G && dst_k.size(2) >= Tp &&
                  dst_k.size(3) == H && dst_k.size(4) == D,
              "kv_replicate: destination must be [L, P*G, >= Tp, Hkv, D]");
  TORCH_CHECK(D % 8 == 0, "kv_replicate: head_dim * 2 bytes must be a multiple of 16");
  TORCH_CHECK(L * P <= 65535 && Tp < (1ll << 31) && H < (1ll << 31) && Tp * H * (D / 8) < (1ll << 40),
              "kv_replicate: shape out of range");
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&src_k, &src_v, &dst_k, &dst_v}) {
    TORCH_CHECK(t->stride(4) == 1 || D == 1, "kv_replicate: head_dim must be contiguous");
    for (int i = 0; i < 4; ++i)
      TORCH_CHECK(t->stride(i) % 8 == 0 && t->stride(i) >= 0, "kv_replicate: strides must be multiples of 8 elements");
    check_aligned16(*t, "kv_replicate operand");
  }
  const int64_t sstr[4] = {src_k.stride(0), src_k.stride(1), src_k.stride(2), src_k.stride(3)};
  const int64_t dstr[4] = {dst_k.stride(0), dst_k.stride(1), dst_k.stride(2), dst_k.stride(3)};
  c10::hip::HIPGuardMasqueradingAsCUDA g(dst_k.device());
  launch_kv_replicate(cbp(src_k), cbp(src_v), bp(dst_k), bp(dst_v), static_cast<int>(L),
                      static_cast<int>(P), static_cast<int>(G), static_cast<int>(Tp),
                      static_cast<int>(H), static_cast<int>(D), sstr, dstr, cur_stream(dst_k));
}

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("kv_replicate(Tensor src_k, Tensor src_v, Tensor(a!) dst_k, Tensor(b!) dst_v, int G) -> ()");
  m.def("decode_attn(Tensor q, Tensor k_cache, Tensor v_cache, Tensor kv_len, Tensor? kv_start, int window, float scale) -> Tensor");
  m.def("rope_cache_write(Tensor qkv, Tensor cos, Tensor sin, Tensor pos, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slot, int Hq, int Hkv, int D, int rot) -> Tensor");
  m.def("decode_attn_rope(Tensor qkv, Tensor cos, Tensor sin, Tensor pos, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slot, Tensor kv_len, Tensor? kv_start, int window, float scale, int Hq, int Hkv, int D, int rot) -> Tensor");
  m.def("decode_attn_group(Tensor q, Tensor k_cache, Tensor v_cache, Tensor kv_len, Tensor? kv_start, int window, float scale, int group_size, int prefix_len) -> Tensor");
  m.def("decode_attn_rope_group(Tensor qkv, Tensor cos, Tensor sin, Tensor pos, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slot, Tensor kv_len, Tensor? kv_start, int window, float scale, int Hq, int Hkv, int D, int rot, int group_size, int prefix_len) -> Tensor");
  m.def("sample_tokens(Tensor logits, float temperature, int top_k, float top_p, bool greedy, Tensor rng) -> Tensor");
  m.def("sample_tokens_logp(Tensor logits, float temperature, int top_k, float top_p, bool greedy, Tensor rng) -> (Tensor, Tensor)");
  m.def("sample_tokens_logp_tempered(Tensor logits, float temperature, int top_k, float top_p, bool greedy, Tensor rng) -> (Tensor, Tensor)");
  m.def("sample_tokens_keep(Tensor logits, float temperature, int top_k, float top_p, Tensor rng) -> (Tensor, Tensor, Tensor)");
  m.def("skinny_gemm(Tensor x, Tensor w, Tensor(a!) counters, bool swiglu, bool glu_out=False) -> Tensor");
  m.def("skinny_glu_ks(Tensor x, Tensor w) -> Tensor");
  m.def("skinny_fused(Tensor x, Tensor w, Tensor? res, Tensor? ssq_in, float eps, bool glu) -> (Tensor, Tensor)");
  m.def("skinny64(Tensor x, Tensor w, Tensor? res, Tensor? ssq_in, float eps, bool glu) -> (Tensor, Tensor)");
  m.def("skinny64_f8(Tensor x, Tensor w8, Tensor wscale, Tensor? res, Tensor? ssq_in, float eps, bool glu) -> (Tensor, Tensor)");
  m.def("tile_weight(Tensor w, Tensor? nw, Tensor(a!) out, bool glu_il=False) -> ()");
  m.def("quant_tile_f8(Tensor w, Tensor? nw, Tensor(a!) out8, Tensor(b!) scale, bool glu_il=False) -> ()");
  m.def("skinny_glu_il(Tensor x, Tensor wt, Tensor ssq_in, float eps) -> Tensor");
  m.def("skinny_fused_f8(Tensor x, Tensor w8, Tensor wscale, Tensor? res, Tensor? ssq_in, float eps) -> (Tensor, Tensor)");
  m.def("skinny_glu_il_f8(Tensor x, Tensor w8, Tensor wscale, Tensor ssq_in, float eps) -> Tensor");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("kv_replicate", &dla::kv_replicate);
  m.impl("decode_attn", &dla::decode_attn);
  m.impl("decode_attn_group", &dla::decode_attn_group);
  m.impl("decode_attn_rope_group", &dla::decode_attn_rope_group);
  m.impl("sample_tokens", &dla::sample_tokens);
  m.impl("sample_tokens_logp", &dla::sample_tokens_logp);
  m.impl("sample_tokens_logp_tempered", &dla::sample_tokens_logp_tempered);
  m.impl("sample_tokens_keep", &dla::sample_tokens_keep);
  m.impl("rope_cache_write", &dla::rope_cache_write);
  m.impl("decode_attn_rope", &dla::decode_attn_rope);
  m.impl("skinny_gemm", &dla::skinny_gemm);
  m.impl("skinny_glu_ks", &dla::skinny_glu_ks);
  m.impl("skinny_fused", &dla::skinny_fused);
  m.impl("skinny64", &dla::skinny64);
  m.impl("skinny64_f8", &dla::skinny64_f8);
  m.impl("tile_weight", &dla::tile_weight);
  m.impl("quant_tile_f8", &dla::quant_tile_f8);
  m.impl("skinny_glu_il", &dla::skinny_glu_il);
  m.impl("skinny_fused_f8", &dla::skinny_fused_f8);
  m.impl("skinny_glu_il_f8", &dla::skinny_glu_il_f8);
}
