// Launch contract of the decode projection GEMMs, shared by skinny.hip / skinny64.hip (launchers)
// and bindings_decode.cpp (torch ops). KsFuse is a kernel argument as it stands: residual add +
// RMSNorm split across the producing projection (RES) and the consuming one (NIN). SkinnyParams is
// host-side only: the kernels keep their own `const ... __restrict__` pointer parameters.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dla {

using bf16_t = uint16_t;

struct KsFuse {
  const uint16_t* res;     // RES: residual stream [M, N], row stride ldr
  int64_t ldr;
  float* ssq_out;        // RES: [16][gridDim.x] per-(row, workgroup) sums of squares
  const float* ssq_in;   // NIN: [16][nbp] partial sums of squares of x's rows (nbp <= 512)
  int nbp;
  float eps;             // NIN: RMSNorm epsilon (the norm weight is folded into W by the caller)
  const float* wscale;   // F8 weights: per weight-row dequantisation scale (y[:, n] *= wscale[n])
  int straight;          // 1: branch-free ring (ks_body): every slot refill issued unconditionally
};

enum class SkinnyW {
  kRowMajor,  // bf16 [N, K], row stride ldw
  kTiled,     // bf16 [N/16, K/32, 4, 16, 8] (skinny64.hip TW; skinny_glu_il: gate / up interleaved)
  kTiledF8,   // e4m3 [N/16, K/64, 64, 16 B] (skinny_ks.h F8) with per-row scales `wscale`
};

// y = x w^T and its decode-layer epilogues. M <= 16 on skinny.hip (64 on the plain / GLU
// in-workgroup split-K launches), 17..64 on skinny64.hip, where the row partials are per
// (row, 1024 columns) instead of per (row, 16-column workgroup).
struct SkinnyParams {
  const bf16_t* x;  // [M, K], row stride ldx ([M, 2K] with swiglu)
  int64_t ldx;
  int M, N, K;      // N weight rows (glu_out: 2F), K the weight's inner dim
  const void* w;    // bf16_t or uint8_t by layout
  SkinnyW layout;
  int64_t ldw;      // kRowMajor only
  const float* wscale;  // kTiledF8: [N] fp32, in the weight's (tiled) row order
  bf16_t* y;        // [M, N], row stride ldy ([M, N/2] with glu_out)
  int64_t ldy;
  const bf16_t* res;  // [M, N] row stride ldr: y = bf16(bf16(x w^T) + res), row partials of y^2 into ssq_out
  int64_t ldr;
  float* ssq_out;     // [16, N/16] (skinny.hip) or [M, ceil(N/1024)] (skinny64.hip)
  const float* ssq_in;  // [16, nbp <= 512] or [M, nbp <= 64] partials of x's rows: y = rstd[m] * (x w^T)
  int nbp;
  float eps;
  bool glu_out;  // w = [gate; up] (2F rows): y = silu(gate) * up [M, F]
  bool swiglu;   // launch_skinny_gemm: x = gu [M, 2K], silu(g) * u applied while staging
  float* ws;           // launch_skinny_gemm [skinny_splits, M, N] / launch_m64 [m64_num_splits, M, N], splits > 1
  unsigned* counters;  // launch_skinny_gemm: one arrival counter per 128 columns, zero between launches
};

// LDS-staged skinny_gemm_kernel: plain / swiglu input (cross-workgroup split-K by skinny_splits),
// glu_out, and glu_out on a normalised input (ssq_in; row-major or tiled weight)
void launch_skinny_gemm(const SkinnyParams& p, hipStream_t st);
// in-workgroup split-K skinny_ksplit_kernel: plain or glu_out on a row-major weight (M <= 64); with
// `fused` the decode-layer form (res / ssq_in, every layout, M <= 16)
void launch_skinny_ksplit(const SkinnyParams& p, bool fused, hipStream_t st);
// skinny_glu_il_kernel: gate|up over the interleaved tiled weight (kTiled / kTiledF8), ssq_in given
void launch_skinny_glu_il(const SkinnyParams& p, hipStream_t st);
// m64_gemm_kernel, then m64_reduce_kernel with the res / ssq_in epilogue when m64_num_splits > 1
int m64_num_splits(const SkinnyParams& p);
void launch_m64(const SkinnyParams& p, hipStream_t st);

// w [N, K] (+ nw [K] folded, glu_il: gate / up rows interleaved 8 + 8 per tile) -> the tiled bf16
// layout, or the e4m3 tiled copy and its per-row scales
void launch_tile_weight(const bf16_t* w, int64_t ldw, const bf16_t* nw, bf16_t* out, int N, int K,
                        bool glu_il, hipStream_t st);
void launch_quant_tile_f8(const bf16_t* w, int64_t ldw, const bf16_t* nw, uint8_t* out, float* scale,
                          int N, int K, bool glu_il, hipStream_t st);

}  // namespace dla
