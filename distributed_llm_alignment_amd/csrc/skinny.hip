// Skinny GEMM for the decode path: y[M, N] = x[M, K] @ W[N, K]^T with M <= 16 rows (the
// sampling batch), bf16 in/out, fp32 accumulate. Optionally the input is the fused gate|up GEMM
// output gu[M, 2K] and the kernel applies SwiGLU (silu(g) * u, rounded to bf16 exactly as the
// standalone swiglu kernel does) while staging it, so the MLP's down projection reads gu directly.
//
// Reference: every autoregressive step of HF `generate` in src/training/train_rlhf.py:115-121 and
// src/training/generate_teacher_data.py:60-80 runs these projections with a handful of rows.
//
// Why a hand-written kernel: at M <= 16 a GEMM is a weight stream (Llama-3-8B decode reads
// ~16 GB of weights per token) and the library's tiles for it ran at 2.2-4.9 TB/s in a real
// decode step on MI355X. The layout here is built for that stream (measured results and the
// split-K caveat: profiles/r1_decode_skinny.md):
//   * the workgroup stages its K-slice of x in LDS once (rows >= M are never read: those lanes
//     feed zeros to the MFMA);
//   * each wave owns 16 weight rows and walks its K-slice with 16-byte loads, 8 k-steps
//     (8 x 16 B per lane) in flight ahead of the MFMAs (v_mfma_f32_16x16x32_bf16: B fragment =
//     16 weight rows x 32 k, exactly what one 16-byte load per lane delivers);
//   * split-K over workgroups fills the 256 CUs for N = 4096; partial tiles go to an fp32
//     workspace and the last-arriving workgroup of a column (agent-scope release/acquire +
//     ticket counter, re-armed by that workgroup: no memset, graph-capture safe) sums them in a
//     FIXED order: deterministic.
#include "common.h"
#include "skinny_geom.h"
#include "skinny_params.h"
#include "skinny_ks.h"

#include <type_traits>

namespace dla {

// grid: (ceil(N / 128), S), 8 waves. LDS: M x (kc + 8) bf16 (row pad of 16 B keeps the 16-row fragment
// reads on distinct banks).
// GLU_OUT (decode gate|up projection): W is [gate; up] (2F rows) and the output is
// m = silu(gate) * up [M, F]. Block b's waves 0-3 take gate rows [64b, 64b + 64), waves 4-7 the
// matching up rows F + [64b, 64b + 64); the tile is exchanged through LDS and SwiGLU applied in
// the epilogue (after the same bf16 rounding of gate/up as the unfused path): no gu round trip,
// no separate swiglu launch.
// (A NORM variant that formed s = x + res and RMSNorm(s) inside this kernel's staging measured
// 4.39 vs 4.28 ms/token -- 224 workgroups each re-deriving the row norm -- and was removed.)

// Decode-layer fusion of the residual add + RMSNorm across two launches (no norm launch):
//   RES (producer, the o / down projections): the epilogue writes the new residual stream
//       s = bf16(bf16(x W^T) + res) instead of the projection, plus per-(row, workgroup) partial
//       sums of s^2 over the workgroup's 16 columns (fixed order) into ssq_out [16][gridDim.x];
//   NIN (consumer, the qkv / gate|up projections of the next sublayer): RMSNorm(s) W^T =
//       rstd[m] * (s (W o w)^T) -- the per-row rsqrt(mean(s^2) + eps) factors out of the GEMM and
//       the norm weight w is folded into a cached copy of W (ops/decode.py). So the consumer is a
//       plain GEMM on s whose epilogue scales row m by rstd[m], computed from the producer's
//       partials (prefetched at kernel start, reduced in fixed order at the end): the weight
//       stream starts at once, and no per-element normalisation is needed.
// Deterministic (eager == graph); the rounding differs from the separate-norm path (h is never
// rounded to bf16; W o w is), so the two agree to bf16 accuracy, not bitwise.

template <bool SWIGLU, bool GLU_OUT = false, bool NTW = false, bool NPRE = false, bool TW = false>
__global__ __launch_bounds__(64 * kSkWaves) void skinny_gemm_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ W, int64_t ldw,
    bf16_t* __restrict__ y, int64_t ldy, float* __restrict__ ws, unsigned* __restrict__ counters,
    int M, int N, int K, int kc, KsFuse fz = KsFuse{}) {
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];
  // NPRE: per-row rstd from the producer's partial sums (see KsFuse)
  __shared__ __attribute__((aligned(16))) float rstd_p[16];
  const int S = gridDim.y;
  const int s = blockIdx.y;
  const int k0 = s * kc;
  const int klen = min(kc, K - k0);
  const int ldl = kc + 8;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int F = N >> 1;
  const int n0 = GLU_OUT ? (wave < 4 ? 0 : F) + blockIdx.x * 64 + (wave & 3) * 16
                         : blockIdx.x * kSkCols + wave * 16;
  const int r = lane & 15, q = lane >> 4;  // fragment row (m for A, n for B), k quarter
  const bool active = n0 < N;
  // TW: W in the tiled layout [N/16, K/32, 4, 16, 8] (skinny64.hip): wp(k) = k-offset k of this lane
  const bf16_t* wrow = TW ? W + static_cast<int64_t>(active ? n0 >> 4 : 0) * 16 * K + (k0 >> 5) * 512 + lane * 8
                          : W + static_cast<int64_t>(active ? n0 + r : 0) * ldw + k0 + q * 8;
  auto wp = [&](int kk) { return TW ? wrow + (kk >> 5) * 512 : wrow + kk; };

  // the first two weight chunks are in flight before x is staged (independent of LDS)
  const int nchunks = klen / kSkChunk;
  s16x8 b0[kSkUnroll], b1[kSkUnroll];
  if (active) {
#pragma unroll
    for (int u = 0; u < kSkUnroll; ++u) b0[u] = load_w<NTW>(wp(u * 32));
    if (nchunks > 1) {
#pragma unroll
      for (int u = 0; u < kSkUnroll; ++u) b1[u] = load_w<NTW>(wp(kSkChunk + u * 32));
    }
  }

  KsPart part{};
  if constexpr (NPRE) part = ks_part_load(fz, M, wave, lane);  // reduced in the epilogue
  // ---- stage x[:, k0:k0+klen] (or swiglu(gu) of it) into LDS: 8 independent 16-byte loads per
  // thread per pass (all issued before the first LDS store, so the pass costs one latency)
  const int vecs = klen >> 3;
  const int total = M * vecs;
  constexpr int NT = 64 * kSkWaves;
  for (int base = 0; base < total; base += 8 * NT) {
    bf16x8 v[8];
    if constexpr (SWIGLU) {
      bf16x8 gg[8], uu[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = base + j * NT + threadIdx.x;
        if (i < total) {
          const int m = i / vecs, c = (i - m * vecs) << 3;
          gg[j] = load_bf16x8(x + m * ldx + k0 + c);
          uu[j] = load_bf16x8(x + m * ldx + K + k0 + c);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = f2bf(silu_sk(bf2f(gg[j][e])) * bf2f(uu[j][e]));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = base + j * NT + threadIdx.x;
        if (i < total) {
          const int m = i / vecs, c = (i - m * vecs) << 3;
          v[j] = load_bf16x8(x + m * ldx + k0 + c);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = base + j * NT + threadIdx.x;
      if (i < total) {
        const int m = i / vecs, c = (i - m * vecs) << 3;
        store_bf16x8(xs + m * ldl + c, v[j]);
      }
    }
  }
  __syncthreads();

  // ---- main loop: ping-pong register buffers, the next chunk's 8 loads stay in flight while
  // the current chunk's 8 MFMAs run (no wait on the newest loads until they are consumed)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    const bf16_t* xrow = xs + r * ldl + q * 8;
    const bool arow = r < M;
    auto compute = [&](const s16x8* b, int kk) {
#pragma unroll
      for (int u = 0; u < kSkUnroll; ++u) {
        s16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (arow) a = __builtin_bit_cast(s16x8, load_bf16x8(xrow + kk + u * 32));
        acc = mfma16(a, b[u], acc);
      }
    };
    // two register sets in a ring: compute chunk c while chunk c+1 is in flight, then refill
    for (int c = 0; c < nchunks; c += 2) {
      compute(b0, c * kSkChunk);
      if (c + 2 < nchunks) {
#pragma unroll
        for (int u = 0; u < kSkUnroll; ++u)
          b0[u] = load_w<NTW>(wp((c + 2) * kSkChunk + u * 32));
      }
      if (c + 1 < nchunks) {
        compute(b1, (c + 1) * kSkChunk);
        if (c + 3 < nchunks) {
#pragma unroll
          for (int u = 0; u < kSkUnroll; ++u)
            b1[u] = load_w<NTW>(wp((c + 3) * kSkChunk + u * 32));
        }
      }
    }
  }

  // ---- epilogue. Lane holds C[m = 4q + i][n = n0 + r], i = 0..3.
  const int n = n0 + r;
  if constexpr (GLU_OUT) {
    __shared__ float glu[2][16][64];  // [gate|up][m][column within the block]
    const int half = wave >> 2, col = (wave & 3) * 16 + r;
    if constexpr (NPRE) {  // RMSNorm row factor of the folded-weight GEMM (see KsFuse)
      ks_rstd(part, fz, M, K, wave, lane, rstd_p);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] *= (4 * q + i < M) ? rstd_p[4 * q + i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) glu[half][4 * q + i][col] = bf2f(f2bf(acc[i]));
    __syncthreads();
    for (int i = threadIdx.x; i < M * 64; i += blockDim.x) {
      const int m = i >> 6, c = i & 63, nn = blockIdx.x * 64 + c;
      if (nn < F) y[m * ldy + nn] = f2bf(silu_sk(glu[0][m][c]) * glu[1][m][c]);
    }
    return;
  }
  if (S == 1) {
    if (n < N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * q + i;
        if (m < M) y[m * ldy + n] = f2bf(acc[i]);
      }
    }
    return;
  }
  // split-K: partial tile -> fp32 slab ws[s][m][n] (plain stores); then one agent-scope release
  // + ticket per workgroup, and one acquire in the last arriver, which sums the S slabs of its 64
  // columns in split order (fixed -> deterministic) with plain loads
  if (n < N) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * q + i;
      if (m < M) ws[(static_cast<int64_t>(s) * M + m) * N + n] = acc[i];
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's slab stores are complete; the x image in LDS is dead
  unsigned* flag = reinterpret_cast<unsigned*>(xs);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev = __hip_atomic_fetch_add(&counters[blockIdx.x], 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = (prev == static_cast<unsigned>(S - 1)) ? 1u : 0u;
  }
  __syncthreads();
  if (flag[0] == 0u) return;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    counters[blockIdx.x] = 0u;  // re-arm for the next launch (kernel boundary orders it)
  }
  __syncthreads();
  const int nb0 = blockIdx.x * kSkCols;
  for (int i = threadIdx.x; i < M * kSkCols; i += blockDim.x) {
    const int m = i / kSkCols, nn = nb0 + (i - m * kSkCols);
    if (nn >= N) continue;
    const float* p = ws + static_cast<int64_t>(m) * N + nn;
    const int64_t slab = static_cast<int64_t>(M) * N;
    float t = 0.f;
    for (int ss = 0; ss < S; ++ss) t += p[ss * slab];
    y[m * ldy + nn] = f2bf(t);
  }
}

// Non-temporal loads on the TILED decode weight streams (each byte read once per step by one CU):
// 3.54 vs 3.70 ms/token at B=8 (profiles/r3_decode_tiled.md). On the row-major layout nt lost
// (4.31 vs 4.19 ms/token: the weights rotated past the Infinity Cache), so the row-major kernels
// use default-policy loads: every launcher below passes NT = TW.
template <SkinnyW L>
using sk_layout = std::integral_constant<SkinnyW, L>;
template <int N>
using sk_int = std::integral_constant<int, N>;

// f(layout) with the weight layout as an integral constant
template <class F>
static void skinny_layout_dispatch(SkinnyW layout, F f) {
  switch (layout) {
    case SkinnyW::kTiledF8: f(sk_layout<SkinnyW::kTiledF8>{}); break;
    case SkinnyW::kTiled: f(sk_layout<SkinnyW::kTiled>{}); break;
    default: f(sk_layout<SkinnyW::kRowMajor>{}); break;
  }
}

// S = 1 at K = 4096 stages up to 16 x 4104 bf16 (> 64 KB default): raise the kernel's dynamic LDS
// limit once per process
template <class K>
static void skinny_lds_limit(K* kernel, int64_t bytes) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(bytes));
  (void)hipGetLastError();  // never leave a sticky error for the caller's next launch check
}

void launch_skinny_gemm(const SkinnyParams& p, hipStream_t st) {
  // glu_out: N = 2F weight rows -> F outputs, 64 per block, never split
  const int S = p.glu_out ? 1 : skinny_splits(p.M, p.N, p.K);
  const KsFuse fz{nullptr, 0, nullptr, p.ssq_in, p.nbp, p.eps, nullptr, 0};
  auto launch = [&](auto swiglu, auto glu, auto npre, auto tw) {
    constexpr bool GLU = decltype(glu)::value, NPRE = decltype(npre)::value, TW = decltype(tw)::value;
    auto* kernel = &skinny_gemm_kernel<decltype(swiglu)::value, GLU, TW, NPRE, TW>;
    static const bool attr_set = [kernel] {
      skinny_lds_limit(kernel, NPRE ? kSkLdsNormMax : GLU ? kSkLdsGluMax : kSkLdsMax);
      return true;
    }();
    (void)attr_set;
    const int kc = p.K / S;
    const dim3 grid(GLU ? p.N / 2 / 64 : (p.N + kSkCols - 1) / kSkCols, S);
    kernel<<<grid, 64 * kSkWaves, skinny_lds_bytes(p.M, kc), st>>>(
        p.x, p.ldx, static_cast<const bf16_t*>(p.w), p.ldw, p.y, p.ldy, p.ws, p.counters, p.M, p.N, p.K, kc, fz);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (p.glu_out && p.ssq_in != nullptr) {  // the fused decode layer's gate|up (KsFuse NIN)
    if (p.layout == SkinnyW::kTiled) launch(no, yes, yes, yes);
    else launch(no, yes, yes, no);
  } else if (p.glu_out) {
    launch(no, yes, no, no);
  } else if (p.swiglu) {
    launch(yes, no, no, no);
  } else {
    launch(no, no, no, no);
  }
}

// Narrow outputs (N <= ~16K: qkv, o, down at Llama-3-8B): ONE workgroup per 16 output columns,
// its 8 waves split K among themselves (wave w: k in [w K/8, (w+1) K/8)) and reduce their
// 16 x 16 accumulators through LDS. No cross-workgroup combine (whose agent-scope release made
// the split-K form slow inside a real decode step), 8 waves per CU for N = 4096. x is read as
// MFMA A fragments straight from global memory (tiny, L2-resident), in the same two-set ring as
// the weights.
// GLU (decode gate|up with the SwiGLU epilogue, W = [gate; up], 2F rows -> m [M, F]): the
// workgroup owns 16 features; waves 0-3 take the gate rows, waves 4-7 the matching up rows, each
// over a quarter of K (F / 16 workgroups).
// MT = row tiles of 16 (M <= 16 MT): every weight fragment feeds MT MFMAs, one per 16 rows of x
// (larger decode batches, e.g. the reference's 64 rollouts per RLHF step on one GPU); UNR k-steps
// per ring slot (4 at MT = 1; 2 above, which keeps the x fragments at ~110 VGPRs for MT = 4, four
// waves per SIMD).
template <int DEPTH, bool NT, bool GLU, int MT = 1, int UNR = kKsUnroll, bool RES = false, bool NIN = false,
          bool TW = false, bool F8 = false>
__global__ __launch_bounds__(512) void skinny_ksplit_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ W, int64_t ldw,
    bf16_t* __restrict__ y, int64_t ldy, int M, int N, int K, KsFuse fz = KsFuse{}) {
  ks_body<DEPTH, NT, GLU, MT, UNR, RES, NIN, TW, F8>(blockIdx.x, gridDim.x, x, ldx, W, ldw, y, ldy, M,
                                                             N, K, fz);
}

// `fused`: the decode-layer launches (KsFuse) -- the residual-producing projection (res) and the
// norm-consuming qkv projection (ssq_in), or a plain one, on any weight layout, M <= 16. They run
// ks_body's branch-free ring (KsFuse::straight) on every shape it covers; its A/B switch went in
// round 6 (3.557 / 3.554 vs 3.581 / 3.569 ms/token at B = 8, profiles/r5_decode_fp8.md). Ring
// depth: skinny_ks_depth; fp8 weights (e4m3 tiled copy + per-row scales, ks_body F8: the o / down /
// qkv projections at half the weight bytes) skinny_ks_f8_depth.
// Otherwise the plain projection, or with glu_out gate|up (N = 2F weight rows) -> m = silu(gate) *
// up [M, F] on F / 16 workgroups, of a row-major weight at M <= 64, the ring as ks_body's default.
void launch_skinny_ksplit(const SkinnyParams& p, bool fused, hipStream_t st) {
  const KsFuse fz{p.res, p.ldr, p.ssq_out, p.ssq_in, p.nbp, p.eps, p.wscale, fused ? 1 : 0};
  const int nb = p.glu_out ? p.N / 32 : p.N / 16;
  auto launch = [&](auto depth, auto mt, auto glu, auto res, auto nin, auto lay) {
    constexpr int MT = decltype(mt)::value;
    constexpr bool TW = decltype(lay)::value != SkinnyW::kRowMajor, F8 = decltype(lay)::value == SkinnyW::kTiledF8;
    skinny_ksplit_kernel<decltype(depth)::value, TW, decltype(glu)::value, MT, MT == 1 ? kKsUnroll : 2,
                         decltype(res)::value, decltype(nin)::value, TW, F8><<<nb, 512, 0, st>>>(
        p.x, p.ldx, static_cast<const bf16_t*>(p.w), p.ldw, p.y, p.ldy, p.M, p.N, p.K, fz);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (fused) {
    skinny_layout_dispatch(p.layout, [&](auto lay) {
      auto epilogue = [&](auto depth) {
        if (p.res != nullptr && p.ssq_in != nullptr) launch(depth, sk_int<1>{}, no, yes, yes, lay);
        else if (p.res != nullptr) launch(depth, sk_int<1>{}, no, yes, no, lay);
        else if (p.ssq_in != nullptr) launch(depth, sk_int<1>{}, no, no, yes, lay);
        else launch(depth, sk_int<1>{}, no, no, no, lay);
      };
      const int depth = p.layout == SkinnyW::kTiledF8 ? skinny_ks_f8_depth() : skinny_ks_depth(p.K);
      if (depth == 4) epilogue(sk_int<4>{});
      else epilogue(sk_int<2>{});
    });
    return;
  }
  constexpr sk_layout<SkinnyW::kRowMajor> rm{};
  auto rows = [&](auto glu) {
    if (p.M <= 16) {
      if constexpr (!decltype(glu)::value) {
        if (skinny_ks_depth(p.K) == 4) return launch(sk_int<4>{}, sk_int<1>{}, glu, no, no, rm);
      }
      launch(sk_int<2>{}, sk_int<1>{}, glu, no, no, rm);
    } else if (p.M <= 32) {
      launch(sk_int<2>{}, sk_int<2>{}, glu, no, no, rm);
    } else {
      launch(sk_int<2>{}, sk_int<4>{}, glu, no, no, rm);
    }
  };
  if (p.glu_out) rows(yes);
  else rows(no);
}

// Decode gate|up (M <= 16) over an INTERLEAVED tiled weight (ops/decode.py `glu_weight`): tile t
// (16 rows) holds gate rows 8t .. 8t+7 (r < 8) and the matching up rows F + 8t .. (r >= 8), the RMSNorm
// weight folded in. One wave per tile, so a lane's gate and up sums meet by one lane swap
// (lane ^ 8) -- no LDS exchange -- and the workgroup size is free: 7 waves give exactly 256
// workgroups at Llama-3-8B (F = 14336: 1792 tiles), where the 8-wave gate|up kernel
// (skinny_gemm_kernel GLU_OUT) runs 224 and leaves 32 CUs idle. Same K order, rstd and bf16
// rounding as that kernel: bitwise the same output.
// F8: Wt is the e4m3 interleaved tiled copy [2F/16, K/64, 64, 16 B] (ks_body F8 layout) and
// fz.wscale the per-row scales in the same interleaved row order; one 1-KB wave load feeds two
// k-steps, so a ring slot of kSkUnroll k-steps is kSkUnroll / 2 loads.
template <int DEPTH, bool F8 = false>
__global__ __launch_bounds__(512) void skinny_glu_il_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                           const bf16_t* __restrict__ Wt,
                                                           bf16_t* __restrict__ y, int64_t ldy, int M,
                                                           int ntiles, int K, KsFuse fz) {
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];
  __shared__ float rstd_s[16];
  const int nwv = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int t = blockIdx.x * nwv + wave;
  const bool active = t < ntiles;
  const int ldl = K + 8;
  const bf16_t* wrow = Wt + static_cast<int64_t>(active ? t : 0) * 16 * K + lane * 8;
  const uint8_t* wrow8 = reinterpret_cast<const uint8_t*>(Wt) + static_cast<int64_t>(active ? t : 0) * 16 * K +
                         lane * 16;
  constexpr int UB = F8 ? kSkUnroll / 2 : kSkUnroll;  // wave loads per ring slot
  const int nchunks = K / kSkChunk;
  // DEPTH chunks of kSkUnroll k-steps in flight (a ring of register sets)
  s16x8 b[DEPTH][F8 ? 1 : kSkUnroll];
  ks_u32x4 b8[DEPTH][F8 ? UB : 1];
  auto wload = [&](int j, int c) {
    if constexpr (F8) {
#pragma unroll
      for (int u = 0; u < UB; ++u) b8[j][u] = *reinterpret_cast<const ks_u32x4*>(wrow8 + (c * UB + u) * 1024);
    } else {
#pragma unroll
      for (int u = 0; u < kSkUnroll; ++u)
        b[j][u] = __builtin_bit_cast(s16x8, load_bf16x8(wrow + (c * kSkUnroll + u) * 512));
    }
  };
  if (active) {
#pragma unroll
    for (int j = 0; j < DEPTH; ++j)
      if (j < nchunks) wload(j, j);
  }
  // this wave's rows' norm partials (rows wave, wave + nwv, ...: 4 cover M <= 16 at >= 4 waves),
  // reduced after the main loop
  float pv[4][8];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int m = wave + rr * nwv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = lane + 64 * j;
      pv[rr][j] = (m < M && i < fz.nbp) ? fz.ssq_in[m * fz.nbp + i] : 0.f;
    }
  }
  // stage x [M, K] into LDS, 4 independent 16-byte loads per thread per pass
  const int vecs = K >> 3, total = M * vecs, nthr = blockDim.x;
  for (int base = 0; base < total; base += 4 * nthr) {
    bf16x8 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = base + j * nthr + threadIdx.x;
      if (i < total) {
        const int m = i / vecs, c = (i - m * vecs) << 3;
        v[j] = load_bf16x8(x + m * ldx + c);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = base + j * nthr + threadIdx.x;
      if (i < total) {
        const int m = i / vecs, c = (i - m * vecs) << 3;
        store_bf16x8(xs + m * ldl + c, v[j]);
      }
    }
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    const bf16_t* xrow = xs + r * ldl + q * 8;
    const bool arow = r < M;
    auto compute = [&](int j, int kk) {
#pragma unroll
      for (int u = 0; u < kSkUnroll; ++u) {
        s16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (arow) a = __builtin_bit_cast(s16x8, load_bf16x8(xrow + kk + u * 32));
        s16x8 bu;
        if constexpr (F8) {
          const ks_u32x4 wv = b8[j][u >> 1];
          bu = (u & 1) ? f8x8_to_bf16(wv[2], wv[3]) : f8x8_to_bf16(wv[0], wv[1]);
        } else {
          bu = b[j][u];
        }
        acc = mfma16(a, bu, acc);
      }
    };
    for (int c0 = 0; c0 < nchunks; c0 += DEPTH) {
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        const int c = c0 + j;
        if (c < nchunks) {
          compute(j, c * kSkChunk);
          if (c + DEPTH < nchunks) wload(j, c + DEPTH);
        }
      }
    }
  }
  // rstd per row: in-lane sum in order, then the butterfly (as ks_rstd)
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int m = wave + rr * nwv;
    float tt = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) tt += pv[rr][j];
    tt = wave_sum(tt);
    if (lane == 0 && m < M && m < 16) rstd_s[m] = rsqrtf(tt / static_cast<float>(K) + fz.eps);
  }
  __syncthreads();
  if (!active) return;
  // lane holds C[m = 4q + i][row r of the tile]: gate (r < 8) and up (r >= 8) of feature 8t + (r & 7)
  const float wsc = F8 ? fz.wscale[16 * t + r] : 1.f;  // this lane's weight row (interleaved order)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = 4 * q + i;
    const float v = bf2f(f2bf((F8 ? acc[i] * wsc : acc[i]) * (m < M ? rstd_s[m] : 0.f)));
    const float o = __shfl_xor(v, 8, 64);
    if (r < 8 && m < M) y[m * ldy + 8 * t + r] = f2bf(silu_sk(v) * o);
  }
}

// gate|up over the interleaved tiled weight (2F rows -> [M, F]); waves per workgroup and ring depth
// in skinny_geom.h (fp8: the interleaved e4m3 tiled copy, fz.wscale)
void launch_skinny_glu_il(const SkinnyParams& p, hipStream_t st) {
  const bool f8 = p.layout == SkinnyW::kTiledF8;
  const int ntiles = p.N / 16, w = glu_il_waves(ntiles, p.M, f8);
  const KsFuse fz{nullptr, 0, nullptr, p.ssq_in, p.nbp, p.eps, p.wscale, 0};
  auto launch = [&](auto depth, auto f8c) {
    auto* kernel = &skinny_glu_il_kernel<decltype(depth)::value, decltype(f8c)::value>;
    static const bool attr_set = [kernel] {
      skinny_lds_limit(kernel, kSkLdsNormMax);
      return true;
    }();
    (void)attr_set;
    kernel<<<(ntiles + w - 1) / w, 64 * w, skinny_lds_bytes(p.M, p.K), st>>>(
        p.x, p.ldx, static_cast<const bf16_t*>(p.w), p.y, p.ldy, p.M, ntiles, p.K, fz);
  };
  auto ring = [&](auto f8c) {
    switch (glu_il_depth(f8)) {
      case 2: launch(sk_int<2>{}, f8c); break;
      case 3: launch(sk_int<3>{}, f8c); break;
      default: launch(sk_int<4>{}, f8c); break;
    }
  };
  if (f8) ring(std::true_type{});
  else ring(std::false_type{});
}

}  // namespace dla
