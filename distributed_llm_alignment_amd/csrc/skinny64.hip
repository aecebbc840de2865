// Decode GEMMs at 17..64 rows: y[M, N] = x[M, K] @ W[N, K]^T, bf16 in/out, fp32 accumulate.
//
// Reference: the rollout batch of src/training/train_rlhf.py:115-124 (config/rlhf_config.yaml:
// 64 prompts per step) runs every projection of every generated token at 64 rows.
//
// Why a separate kernel from skinny.hip (M <= 16): there every workgroup holds ALL of x for its
// K-slice in LDS (16 x 4096 bf16 = 128 KB), or re-reads x fragments per 16 output columns from
// L2. At 64 rows x is 512 KB: it does not fit, and per-16-column re-reads cost ~1.7 GB of L2
// traffic per layer (README "Tried": 11.6 vs 6.1 ms/token). hipBLASLt's 64-row tiles run the
// narrow projections at 2.2-3.0 TB/s (profiles/r3_decode.md, B = 64). Layout here:
//   * a workgroup owns 128 output columns (8 waves x 16; GLU: 64 gate + the matching 64 up
//     columns) and a K-slice; x streams through a 2-slot LDS ring in 256-deep chunks shared by
//     the 8 waves (x traffic from L2 = 1/8 of the per-16-column form);
//   * each wave streams its 16 weight rows with 16-byte loads straight into registers (two
//     256-deep ring slots = 16 loads in flight per lane), B fragments of
//     v_mfma_f32_16x16x32_bf16; every weight fragment feeds MT = M/16 MFMAs (one per 16 rows);
//   * narrow outputs split K over workgroups (>= 256 workgroups) into fp32 slabs, reduced in a
//     FIXED order with the decode-layer epilogue (residual add + row sum of squares, or the
//     RMSNorm row factor) by a second small launch (m64_reduce_kernel) -- deterministic,
//     graph-capture safe;
//   * the gate|up projection (wide, no split) applies RMSNorm's row factor and SwiGLU in its
//     own epilogue.
#include "common.h"
#include "skinny_geom.h"
#include "skinny_params.h"

#include <type_traits>

namespace dla {

namespace {

constexpr int kM64Steps = kM64Ck / 32;  // MFMA k-steps per chunk
constexpr int kM64MaxNbp = 64;          // row-norm partials per row (N / 128 <= 64: H <= 8192)
constexpr int kM64RegNbp = 8;           // partials held in registers (reduce-launch producers: N / 1024)

__device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// F8 (weight-only fp8 decode, TW + nt only): W is the e4m3 tiled copy [N/16, K/64, 64 lanes, 16 B]
// of csrc/skinny_ks.h F8 (ops/decode.py fp8_tiled_weight): one 16-byte load per lane holds its B
// fragments of two consecutive k-steps, so a 256-deep chunk is 4 loads per lane instead of 8 and
// the stream is half the bytes; e4m3 -> bf16 in registers (exact), the bf16 MFMA unchanged, and
// the per-row scale wsc[n] applied to the fp32 sum before any epilogue.
// Weight layouts: row-major W [N, K], or TW (tiled, ops/decode.py `tiled_weight`):
// Wt[N / 16][K / 32][4][16][8] with Wt[t][kk][q][r][e] = W[16 t + r][32 kk + 8 q + e], i.e. the
// 16-byte pieces in the order lane (r = lane & 15, q = lane >> 4) of an MFMA B fragment reads them:
// one weight load instruction is 1 KB contiguous and a wave's 256-deep chunk 8 KB, instead of 16
// rows x 64 B at an 8 KB (K = 4096) stride.
}  // namespace

// grid (N / 16 NW [GLU: F / 8 NW], S), 64 NW threads. LDS: 2 x 16 MT x kM64Ld bf16.
// GLU: W = [gate; up] (2F rows), output m = silu(rstd * g) * (rstd * u) [M, F] where rstd comes
// from ssq_in (the producer's row partial sums, [M][nbp]) when NIN, else 1; gate / up are
// rounded to bf16 before SwiGLU exactly as the unfused GEMM + swiglu pair.
// Otherwise S == 1 writes y = bf16(x W^T); S > 1 writes fp32 slab ws[s][m][n].
template <int MT, bool GLU, bool NIN, bool TW, int DEPTH, int NW = kM64Waves, bool NTL = false, bool F8 = false>
__global__ __launch_bounds__(64 * NW) void m64_gemm_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ W, int64_t ldw,
    bf16_t* __restrict__ y, int64_t ldy, float* __restrict__ ws, int M, int N, int K, int kc,
    const float* __restrict__ ssq_in, int nbp, float eps, const float* __restrict__ wsc) {
  static_assert(!F8 || (TW && NTL), "fp8 weights: tiled layout, nt stream");
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];
  __shared__ float rstd_s[64];
  constexpr int RB = 16 * MT * kM64Ld;  // one ring slot
  constexpr int NTH = 64 * NW;
  constexpr int XPASS = 16 * MT * 32 / NTH;  // x staging passes (32 threads per 256-deep row)
  constexpr int FPW = 8 * NW;                // GLU: features per workgroup
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  const int F = N >> 1;
  const int n0 = GLU ? (wave < NW / 2 ? 0 : F) + blockIdx.x * FPW + (wave % (NW / 2)) * 16
                     : blockIdx.x * (16 * NW) + wave * 16;
  const int s = blockIdx.y;
  const int k0 = s * kc;
  const int nch = kc / kM64Ck;
  const bf16_t* wrow = TW ? W + static_cast<int64_t>(n0 >> 4) * 16 * K + (k0 >> 5) * 512 + lane * 8
                         : W + static_cast<int64_t>(n0 + r) * ldw + k0 + q * 8;
  const uint8_t* wrow8 = reinterpret_cast<const uint8_t*>(W) + static_cast<int64_t>(n0 >> 4) * 16 * K +
                         (k0 >> 6) * 1024 + lane * 16;

  // NIN: this row's producer partials (thread m < M holds row m); up to kM64RegNbp are loaded
  // here, ahead of the first chunk, and summed once those loads land
  float pv[kM64RegNbp];
  if constexpr (NIN) {
#pragma unroll
    for (int j = 0; j < kM64RegNbp; ++j)
      pv[j] = (tid < M && j < nbp && nbp <= kM64RegNbp) ? ssq_in[tid * nbp + j] : 0.f;
  }

  // Pipeline: chunk j = x(j) (this thread's 16-byte pieces of 16 MT rows, into register set
  // j % DEPTH) followed by W(j) (8 loads per lane into ring slot j % DEPTH) -- ALWAYS in that
  // issue order, because s_waitcnt vmcnt is in-order: storing x(c + 1) into LDS waits only for
  // loads older than it, so W(c + 1) stays in flight (loading x after W made every step wait a
  // full HBM round trip for the next weight chunk). DEPTH chunks are in flight; x rows >= M are
  // zeros so the A fragments need no row test.
  const int xm = tid >> 5, xc = (tid & 31) * 8;
  typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
  constexpr int KS8 = kM64Steps / 2;  // fp8: 16-byte weight loads per lane per chunk
  bf16x8 xr[DEPTH][XPASS];
  s16x8 b[DEPTH][F8 ? 1 : kM64Steps];
  u32x4v b8[DEPTH][F8 ? KS8 : 1];
  auto issue = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
#pragma unroll
    for (int t = 0; t < XPASS; ++t) {
      const int m = xm + (NTH / 32) * t;
      xr[j][t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (m < M) xr[j][t] = load_bf16x8(x + static_cast<int64_t>(m) * ldx + k0 + c * kM64Ck + xc);
    }
    if constexpr (F8) {
#pragma unroll
      for (int u = 0; u < KS8; ++u)
        b8[j][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4v*>(wrow8 + (c * KS8 + u) * 1024));
      return;
    }
#pragma unroll
    for (int u = 0; u < kM64Steps; ++u)
      b[j][u] = NTL ? __builtin_bit_cast(s16x8, __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(
                          TW ? wrow + (c * kM64Steps + u) * 512 : wrow + c * kM64Ck + u * 32)))
                    : __builtin_bit_cast(s16x8, load_bf16x8(TW ? wrow + (c * kM64Steps + u) * 512 : wrow + c * kM64Ck + u * 32));
  };
  auto xstore = [&](auto J, int slot) {
    constexpr int j = decltype(J)::value;
#pragma unroll
    for (int t = 0; t < XPASS; ++t) store_bf16x8(xs + slot * RB + (xm + (NTH / 32) * t) * kM64Ld + xc, xr[j][t]);
  };
  issue(std::integral_constant<int, 0>{}, 0);
  if (1 < nch) issue(std::integral_constant<int, 1>{}, 1);
  if constexpr (DEPTH > 2) {
    if (2 < nch) issue(std::integral_constant<int, 2>{}, 2);
  }
  if constexpr (DEPTH > 3) {
    if (3 < nch) issue(std::integral_constant<int, 3>{}, 3);
  }
  // NIN: the row's partials summed now, in order (their loads are older than the chunk loads, so
  // this waits only for them), one register live through the loop; the in-kernel-combine
  // producers' N / 128 partials (> kM64RegNbp) are summed by a plain loop
  float rsum = 0.f;
  if constexpr (NIN) {
    if (nbp <= kM64RegNbp) {
#pragma unroll
      for (int j = 0; j < kM64RegNbp; ++j) rsum += pv[j];
    } else if (tid < M) {
      for (int j = 0; j < nbp; ++j) rsum += ssq_in[tid * nbp + j];
    }
    asm volatile("" : "+v"(rsum));
  }
  xstore(std::integral_constant<int, 0>{}, 0);
  __syncthreads();

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int aoff = r * kM64Ld + q * 8;
  auto step = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const bf16_t* xb = xs + (c & 1) * RB + aoff;
#pragma unroll
    for (int u = 0; u < kM64Steps; ++u) {
      s16x8 bu;
      if constexpr (F8) {
        const u32x4v wv = b8[j][u >> 1];
        bu = (u & 1) ? f8x8_to_bf16(wv[2], wv[3]) : f8x8_to_bf16(wv[0], wv[1]);
      } else {
        bu = b[j][u];
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const s16x8 a = __builtin_bit_cast(s16x8, *reinterpret_cast<const bf16x8*>(xb + t * 16 * kM64Ld + u * 32));
        acc[t] = mfma16(a, bu, acc[t]);
      }
    }
    if (c + 1 < nch) xstore(std::integral_constant<int, (j + 1) % DEPTH>{}, (c + 1) & 1);
    __syncthreads();
    if (c + DEPTH < nch) issue(J, c + DEPTH);
  };
  for (int c = 0; c < nch; c += DEPTH) {
    step(std::integral_constant<int, 0>{}, c);
    if (c + 1 < nch) step(std::integral_constant<int, 1>{}, c + 1);
    if constexpr (DEPTH > 2) {
      if (c + 2 < nch) step(std::integral_constant<int, 2>{}, c + 2);
    }
    if constexpr (DEPTH > 3) {
      if (c + 3 < nch) step(std::integral_constant<int, 3>{}, c + 3);
    }
  }

  // lane holds C[m = 16 t + 4 q + i][n = n0 + r]
  if constexpr (F8) {
    const float sc = wsc[n0 + r];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] *= sc;
  }
  if constexpr (GLU) {
    if constexpr (NIN) {
      if (tid < M) rstd_s[tid] = rsqrtf(rsum / static_cast<float>(K) + eps);
    }
    // the ring is dead after the loop's last barrier: exchange the gate / up tiles through it
    float* glu = reinterpret_cast<float*>(xs);  // [2][64][FPW]
    const int half = wave / (NW / 2), col = (wave % (NW / 2)) * 16 + r;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 16 * t + 4 * q + i;
        float v = acc[t][i];
        if constexpr (NIN) v *= m < M ? rstd_s[m] : 0.f;
        glu[(half * 64 + m) * FPW + col] = bf2f(f2bf(v));
      }
    __syncthreads();
    // 8 consecutive features of one row per thread, one 16-byte store
    for (int e = tid; e < M * (FPW / 8); e += NTH) {
      const int m = e / (FPW / 8), c8 = (e % (FPW / 8)) * 8;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = glu[m * FPW + c8 + j], u = glu[(64 + m) * FPW + c8 + j];
        o[j] = g / (1.f + __expf(-g)) * u;
      }
      store_bf16x8(y + static_cast<int64_t>(m) * ldy + blockIdx.x * FPW + c8, pack_bf16x8(o));
    }
    return;
  }
  const int n = n0 + r;
  if (gridDim.y == 1) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 16 * t + 4 * q + i;
        if (m < M) y[static_cast<int64_t>(m) * ldy + n] = f2bf(acc[t][i]);
      }
    return;
  }
  float* slab = ws + static_cast<int64_t>(s) * M * N;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 16 * t + 4 * q + i;
      if (m < M) slab[static_cast<int64_t>(m) * N + n] = acc[t][i];
    }
}

// Split-K reduce + decode-layer epilogue. grid (ceil(N / 1024), M), 256 threads x 4 columns.
//   MODE 0: y = bf16(sum_s ws[s])
//   MODE 1 (NIN): y = bf16(rstd[m] * sum), rstd = rsqrt(sum_j ssq_in[m][j] / N_norm + eps)
//   MODE 2 (RES): y = s = bf16(bf16(sum) + res) and ssq_out[m][blockIdx.x] = sum over the
//                 block's 1024 columns of s^2 (fixed order) -- the next NIN consumer's partials
template <int MODE, int S>
__global__ __launch_bounds__(256) void m64_reduce_kernel(const float* __restrict__ ws, int M,
                                                         int N, bf16_t* __restrict__ y, int64_t ldy,
                                                         const bf16_t* __restrict__ res, int64_t ldr,
                                                         const float* __restrict__ ssq_in, int nbp,
                                                         int knorm, float eps, float* __restrict__ ssq_out) {
  __shared__ float red[4];
  const int m = blockIdx.y;
  const int n = blockIdx.x * 1024 + threadIdx.x * 4;
  const float* p = ws + static_cast<int64_t>(m) * N + n;
  const int64_t slab = static_cast<int64_t>(M) * N;
  const bool live = n < N;  // N % 128 == 0: a thread's 4 columns are all in or all out
  // all S slab loads in flight at once (compile-time count), summed in split order
  f32x4 v[S];
  if (live) {
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = *reinterpret_cast<const f32x4*>(p + s * slab);
  }
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int s = 0; s < S; ++s) t += v[s];
  }
  if constexpr (MODE == 1) {
    float a = 0.f;
    for (int j = 0; j < nbp; ++j) a += ssq_in[m * nbp + j];
    t *= rsqrtf(a / static_cast<float>(knorm) + eps);
  }
  bf16x4 o;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!live) break;
    if constexpr (MODE == 2) {
      const float v = bf2f(f2bf(bf2f(f2bf(t[i])) + bf2f(res[static_cast<int64_t>(m) * ldr + n + i])));
      o[i] = f2bf(v);
      ss += v * v;
    } else {
      o[i] = f2bf(t[i]);
    }
  }
  if (live) *reinterpret_cast<bf16x4*>(y + static_cast<int64_t>(m) * ldy + n) = o;
  if constexpr (MODE == 2) {
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) ssq_out[m * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

template <int N>
using m64_int = std::integral_constant<int, N>;

// split count of a launch (skinny_geom.h m64_splits on this device's CU count); the gate|up
// projection is wide and never splits
int m64_num_splits(const SkinnyParams& p) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    (void)hipGetLastError();
    return n;
  }();
  return p.glu_out ? 1 : m64_splits(p.N, p.K, cus);
}

// The GEMM (S > 1: fp32 slabs into p.ws), then the split-K reduce with the res / ssq_in epilogue.
// NW = 8 waves per workgroup (gate|up: 64 features per workgroup). 4 waves (448 gate|up
// workgroups at Llama-3-8B, two per CU) measured 55.0 vs 53.2 us: README "Tried".
// Non-temporal loads on the tiled weight streams only (see skinny.hip), two weight chunks in flight
// per wave on the bf16 ones (3 or 4 measured 5.10 / 5.27 vs 5.01 ms/token at B = 64: more bytes in
// flight only lengthen the queues; removed), m64_f8_depth on the e4m3 tiled copy (p.wscale its
// per-row scales).
void launch_m64(const SkinnyParams& p, hipStream_t st) {
  const int S = m64_num_splits(p);
  auto gemm = [&](auto mt, auto glu, auto nin, auto tw, auto f8, auto depth) {
    constexpr int MT = decltype(mt)::value;
    constexpr bool GLU = decltype(glu)::value, NIN = decltype(nin)::value, TW = decltype(tw)::value;
    auto* kernel = &m64_gemm_kernel<MT, GLU, NIN, TW, decltype(depth)::value, kM64Waves, TW, decltype(f8)::value>;
    static const bool attr = [kernel] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kM64LdsMax));
      (void)hipGetLastError();
      return true;
    }();
    (void)attr;
    const dim3 grid(GLU ? p.N / 2 / (8 * kM64Waves) : p.N / (16 * kM64Waves), S);
    // the plain rows leave res / ssq_in to the reduce launch
    kernel<<<grid, 64 * kM64Waves, m64_lds_bytes(MT), st>>>(
        p.x, p.ldx, static_cast<const bf16_t*>(p.w), p.ldw, p.y, p.ldy, p.ws, p.M, p.N, p.K, p.K / S,
        NIN ? p.ssq_in : nullptr, NIN ? p.nbp : 0, NIN ? p.eps : 0.f, p.wscale);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  auto epilogue = [&](auto mt, auto tw, auto f8, auto depth) {
    if (p.glu_out && p.ssq_in != nullptr) gemm(mt, yes, yes, tw, f8, depth);
    else if (p.glu_out) gemm(mt, yes, no, tw, f8, depth);
    else gemm(mt, no, no, tw, f8, depth);
  };
  auto weight = [&](auto mt) {
    if (p.layout == SkinnyW::kRowMajor) return epilogue(mt, no, no, m64_int<2>{});
    if (p.layout == SkinnyW::kTiled) return epilogue(mt, yes, no, m64_int<2>{});
    switch (m64_f8_depth()) {
      case 2: epilogue(mt, yes, yes, m64_int<2>{}); break;
      case 4: epilogue(mt, yes, yes, m64_int<4>{}); break;
      default: epilogue(mt, yes, yes, m64_int<3>{}); break;
    }
  };
  if (m64_row_tiles(p.M) == 2) weight(m64_int<2>{});
  else weight(m64_int<4>{});
  if (S == 1) return;

  const dim3 rgrid((p.N + 1023) / 1024, p.M);
  auto reduce = [&](auto mode, auto s) {
    m64_reduce_kernel<decltype(mode)::value, decltype(s)::value><<<rgrid, 256, 0, st>>>(
        p.ws, p.M, p.N, p.y, p.ldy, p.res, p.ldr, p.ssq_in, p.nbp, p.K, p.eps, p.ssq_out);
  };
  auto splits = [&](auto mode) {
    switch (S) {  // the split counts m64_splits chooses from
      case 2: reduce(mode, m64_int<2>{}); break;
      case 4: reduce(mode, m64_int<4>{}); break;
      case 7: reduce(mode, m64_int<7>{}); break;
      case 8: reduce(mode, m64_int<8>{}); break;
      case 14: reduce(mode, m64_int<14>{}); break;
      case 16: reduce(mode, m64_int<16>{}); break;
      default: break;
    }
  };
  if (p.res != nullptr) splits(m64_int<2>{});
  else if (p.ssq_in != nullptr) splits(m64_int<1>{});
  else splits(m64_int<0>{});
}

// Shared by the weight-copy kernels below (tile_weight / quant_tile_f8 and their LoRA-merged forms).
// Row r of 16-row tile t -> weight row. glu_f > 0 (gate|up, F = glu_f): rows r < 8 are gate rows
// 8t + r, rows r >= 8 up rows F + 8t + r - 8.
__device__ __forceinline__ int64_t tile_row_of(int64_t t, int r, int glu_f) {
  return glu_f > 0 ? (r < 8 ? 8 * t + r : glu_f + 8 * t + r - 8) : t * 16 + r;
}

// bf16(v * nw) on 8 columns (torch.mul's rounding); nw_col == nullptr: v
__device__ __forceinline__ bf16x8 fold_norm8(bf16x8 v, const bf16_t* nw_col) {
  if (nw_col != nullptr) {
    const bf16x8 g = load_bf16x8(nw_col);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = f2bf(bf2f(v[e]) * bf2f(g[e]));
  }
  return v;
}

// One 16-byte lane piece of the F8 tiled layout: e4m3(clamp(v / sc, +-448)) of lo (k = 8 qd ..) then
// hi (k = 32 + 8 qd ..), round to nearest even; bytes 4j .. 4j+3 hold elements 4j .. 4j+3
__device__ __forceinline__ uint4 pack_f8_piece(const bf16x8& lo, const bf16x8& hi, float sc) {
  auto q8 = [&](bf16_t x) { return fminf(fmaxf(bf2f(x) / sc, -448.f), 448.f); };
  uint32_t wv[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bf16x8& v = h ? hi : lo;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint32_t wd = __builtin_amdgcn_cvt_pk_fp8_f32(q8(v[4 * j]), q8(v[4 * j + 1]), 0u, false);
      wd = __builtin_amdgcn_cvt_pk_fp8_f32(q8(v[4 * j + 2]), q8(v[4 * j + 3]), wd, true);
      wv[2 * h + j] = wd;
    }
  }
  return make_uint4(wv[0], wv[1], wv[2], wv[3]);
}

// W [N, K] (row stride ldw) -> the tiled layout [N/16, K/32, 4, 16, 8] (see TW above; glu_il: gate /
// up rows interleaved 8 + 8 per tile, skinny.hip skinny_glu_il_kernel), with nw
// the RMSNorm weight folded in (bf16(W * nw), torch.mul's rounding). One 16-byte output piece per
// thread: a wave writes 1 KB contiguous and reads 16 rows x 64 B. Rebuilt whenever the weights
// moved (every RLHF step): one pass instead of mul + a strided permute copy.
__global__ __launch_bounds__(256) void tile_weight_kernel(const bf16_t* __restrict__ W, int64_t ldw,
                                                          const bf16_t* __restrict__ nw,
                                                          bf16_t* __restrict__ out, int K,
                                                          int64_t total, int glu_f) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = static_cast<int>(i & 63);
  const int64_t blk = i >> 6;
  const int kb = K >> 5;
  const int64_t t = blk / kb;
  const int kk = static_cast<int>(blk - t * kb);
  const int col = kk * 32 + (lane >> 4) * 8;
  const int64_t row = tile_row_of(t, lane & 15, glu_f);
  const bf16x8 v = fold_norm8(load_bf16x8(W + row * ldw + col), nw != nullptr ? nw + col : nullptr);
  store_bf16x8(out + i * 8, v);
}

void launch_tile_weight(const bf16_t* W, int64_t ldw, const bf16_t* nw, bf16_t* out, int N, int K,
                        bool glu_il, hipStream_t st) {
  const int64_t total = static_cast<int64_t>(N) * K / 8;
  tile_weight_kernel<<<static_cast<unsigned>((total + 255) / 256), 256, 0, st>>>(W, ldw, nw, out, K, total,
                                                                                 glu_il ? N / 2 : 0);
}

// Weight-only fp8 decode copy in one pass (ops/decode.py fp8_tiled_weight; refreshed every RLHF
// step): W [N, K] (row stride ldw), nw folded as bf16(W * nw), glu_f > 0 = gate / up rows
// interleaved 8 + 8 per tile (as tile_weight_kernel) -> per-row scale amax / 448 and the e4m3
// tiled layout [N/16, K/64, 64, 16 B] of csrc/skinny_ks.h F8. One 256-thread workgroup per 16-row
// tile: 16 threads per row reduce its amax (the rows then sit in L2 for the second pass), every
// thread then writes whole 16-byte lane pieces (round to nearest even, values pre-clamped to
// +-448 as the torch reference does).
__global__ __launch_bounds__(256) void quant_tile_f8_kernel(const bf16_t* __restrict__ W, int64_t ldw,
                                                            const bf16_t* __restrict__ nw,
                                                            uint8_t* __restrict__ out, float* __restrict__ scale,
                                                            int K, int glu_f) {
  __shared__ float inv_s[16];
  const int t = blockIdx.x, tid = threadIdx.x;
  auto row_of = [&](int r) -> int64_t { return tile_row_of(t, r, glu_f); };
  auto fetch = [&](int64_t row, int col) {
    return fold_norm8(load_bf16x8(W + row * ldw + col), nw != nullptr ? nw + col : nullptr);
  };
  {
    const int r = tid >> 4, sub = tid & 15;
    const int64_t row = row_of(r);
    float am = 0.f;
    for (int c = sub * 8; c < K; c += 128) {
      const bf16x8 v = fetch(row, c);
#pragma unroll
      for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(bf2f(v[e])));
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 16));
    if (sub == 0) {
      const float sc = fmaxf(am / 448.f, 1e-12f);
      scale[16 * static_cast<int64_t>(t) + r] = sc;
      inv_s[r] = sc;
    }
  }
  __syncthreads();
  const int pieces = (K >> 6) * 64;
  uint8_t* otile = out + static_cast<int64_t>(t) * 16 * K;
  for (int p = tid; p < pieces; p += 256) {
    const int kt = p >> 6, lane = p & 63, r = lane & 15, qd = lane >> 4;
    const int64_t row = row_of(r);
    const float sc = inv_s[r];
    const bf16x8 lo = fetch(row, 64 * kt + 8 * qd), hi = fetch(row, 64 * kt + 32 + 8 * qd);
    *reinterpret_cast<uint4*>(otile + static_cast<int64_t>(p) * 16) = pack_f8_piece(lo, hi, sc);
  }
}

void launch_quant_tile_f8(const bf16_t* W, int64_t ldw, const bf16_t* nw, uint8_t* out, float* scale, int N,
                          int K, bool glu_il, hipStream_t st) {
  quant_tile_f8_kernel<<<N / 16, 256, 0, st>>>(W, ldw, nw, out, scale, K, glu_il ? N / 2 : 0);
}

// ---- LoRA-merged forms: the same copies built from W + s B A in one pass (ops/decode.py `lora=`) ----
//   m[n, k] = bf16(float(w[n, k]) + s * sum_j b[n, j] a[j, k])      sum in fp32 (MFMA), one fma
//   v       = nw ? bf16(float(m) * float(nw[k])) : m                then the layout of the op above
// mfma_f32_16x16x32_bf16 on the transposed 16 x 32 block (fragment maps: lora.hip): the A operand's
// rows are k, the B operand's columns the tile's 16 weight rows. Two MFMAs h = 0, 1 take their A
// rows interleaved (row r' of h holds k = 8 (r' / 4) + 4 h + r' % 4), so lane (fr, fq) ends up
// with k = 8 fq .. 8 fq + 7 of tile row fr: exactly the tiled layout's 16-byte piece, and the w
// load, the nw load and the store are those of tile_weight_kernel. B operand: 8 consecutive j of
// one b row, invariant along K, held in registers. A operand: 8 consecutive j of one column of a,
// read from a contiguous A^T [K, R] copy (both 16-byte loads). R = 8, 16: lanes with j >= R load a
// clamped address and are zeroed with a select; R = 64: KS = 2 k-steps. No atomics.
__device__ __forceinline__ s16x8 frag_or_zero(const bf16_t* p, bool ok) {
  const s16x8 v = *reinterpret_cast<const s16x8*>(p);
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? v : z;
}

template <int KS>
__device__ __forceinline__ void lora_b_frags(const bf16_t* __restrict__ b, int64_t ldb, int64_t row, int R,
                                             int fq, s16x8 (&bf)[KS]) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int j0 = 32 * s + 8 * fq;
    const bool ok = j0 < R;
    bf[s] = frag_or_zero(b + row * ldb + (ok ? j0 : 0), ok);
  }
}

template <int KS>
__device__ __forceinline__ void lora_at_frags(const bf16_t* __restrict__ at, int R, int col0, int fr, int fq,
                                              s16x8 (&af)[2][KS]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = col0 + 8 * (fr >> 2) + 4 * h + (fr & 3);
      const int j0 = 32 * s + 8 * fq;
      const bool ok = j0 < R;
      af[h][s] = frag_or_zero(at + static_cast<int64_t>(k) * R + (ok ? j0 : 0), ok);
    }
}

// the lane's piece of v: columns col .. col + 7 of weight row `wrow`
template <int KS>
__device__ __forceinline__ bf16x8 lora_merged_piece(const bf16_t* __restrict__ wrow, const bf16_t* __restrict__ nw,
                                                    int col, const s16x8 (&af)[2][KS], const s16x8 (&bf)[KS],
                                                    float scale) {
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[h][s], bf[s], acc[h], 0, 0, 0);
  const bf16x8 wv = load_bf16x8(wrow + col);
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = fmaf(scale, acc[e >> 2][e & 3], bf2f(wv[e]));
  return fold_norm8(pack_bf16x8(o), nw != nullptr ? nw + col : nullptr);
}

constexpr int kLoraMT = 4;  // 16-row tiles per workgroup: one A^T fragment feeds all of them

// grid (ceil(ntiles / kLoraMT), ksplit), 4 waves: wave (blockIdx.y, w) walks the 32-column blocks
// kk = 4 blockIdx.y + w, + 4 gridDim.y, ... of its tiles (neighbouring waves write neighbouring KBs)
template <int KS>
__global__ __launch_bounds__(256) void lora_tile_weight_kernel(
    const bf16_t* __restrict__ W, int64_t ldw, const bf16_t* __restrict__ at, const bf16_t* __restrict__ b,
    int64_t ldb, int R, float scale, const bf16_t* __restrict__ nw, bf16_t* __restrict__ out, int K,
    int64_t ntiles, int glu_f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int kb = K >> 5;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kLoraMT;
  s16x8 bf[kLoraMT][KS];
  const bf16_t* wrow[kLoraMT];
#pragma unroll
  for (int i = 0; i < kLoraMT; ++i) {
    const int64_t t = t0 + i < ntiles ? t0 + i : ntiles - 1;  // (a tail tile is computed, not stored)
    const int64_t row = tile_row_of(t, fr, glu_f);
    wrow[i] = W + row * ldw;
    lora_b_frags<KS>(b, ldb, row, R, fq, bf[i]);
  }
  const int step = 4 * static_cast<int>(gridDim.y);
  for (int kk = 4 * static_cast<int>(blockIdx.y) + w; kk < kb; kk += step) {
    s16x8 af[2][KS];
    lora_at_frags<KS>(at, R, kk * 32, fr, fq, af);
#pragma unroll
    for (int i = 0; i < kLoraMT; ++i) {
      const bf16x8 v = lora_merged_piece<KS>(wrow[i], nw, kk * 32 + 8 * fq, af, bf[i], scale);
      if (t0 + i < ntiles) store_bf16x8(out + (((t0 + i) * kb + kk) * 64 + lane) * 8, v);
    }
  }
}

void launch_lora_tile_weight(const bf16_t* W, int64_t ldw, const bf16_t* at, const bf16_t* b, int64_t ldb, int R,
                             float scale, const bf16_t* nw, bf16_t* out, int N, int K, bool glu_il,
                             hipStream_t st) {
  const int64_t ntiles = N / 16;
  const int kb = K / 32;
  dim3 grid(static_cast<unsigned>((ntiles + kLoraMT - 1) / kLoraMT),
            static_cast<unsigned>(kb >= 32 ? (kb / 16 < 64 ? kb / 16 : 64) : 1));
  const int glu_f = glu_il ? N / 2 : 0;
  if (R <= 32)
    lora_tile_weight_kernel<1><<<grid, 256, 0, st>>>(W, ldw, at, b, ldb, R, scale, nw, out, K, ntiles, glu_f);
  else
    lora_tile_weight_kernel<2><<<grid, 256, 0, st>>>(W, ldw, at, b, ldb, R, scale, nw, out, K, ntiles, glu_f);
}

// quant_tile_f8_kernel on the merged weight: one workgroup per 16-row tile, pass 1 the row amax of
// v (wave w takes the 32-column blocks w, w + 4, ...; lanes, then waves, meet through fmaxf: order
// free), pass 2 recomputes v (a K = 14336 tile row does not fit LDS) and writes the e4m3 pieces.
template <int KS>
__global__ __launch_bounds__(256) void lora_quant_tile_f8_kernel(
    const bf16_t* __restrict__ W, int64_t ldw, const bf16_t* __restrict__ at, const bf16_t* __restrict__ b,
    int64_t ldb, int R, float scale, const bf16_t* __restrict__ nw, uint8_t* __restrict__ out,
    float* __restrict__ scale_out, int K, int glu_f) {
  __shared__ float am_s[4][16];
  __shared__ float sc_s[16];
  const int64_t t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t row = tile_row_of(t, fr, glu_f);
  const bf16_t* wrow = W + row * ldw;
  s16x8 bf[KS];
  lora_b_frags<KS>(b, ldb, row, R, fq, bf);
  auto piece = [&](int kk) {
    s16x8 af[2][KS];
    lora_at_frags<KS>(at, R, kk * 32, fr, fq, af);
    return lora_merged_piece<KS>(wrow, nw, kk * 32 + 8 * fq, af, bf, scale);
  };
  const int kb = K >> 5;
  float am = 0.f;
  for (int kk = w; kk < kb; kk += 4) {
    const bf16x8 v = piece(kk);
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(bf2f(v[e])));
  }
  am = fmaxf(am, __shfl_xor(am, 16, 64));
  am = fmaxf(am, __shfl_xor(am, 32, 64));
  if (fq == 0) am_s[w][fr] = am;
  __syncthreads();
  if (tid < 16) {
    const float a4 = fmaxf(fmaxf(am_s[0][tid], am_s[1][tid]), fmaxf(am_s[2][tid], am_s[3][tid]));
    const float sc = fmaxf(a4 / 448.f, 1e-12f);
    scale_out[16 * t + tid] = sc;
    sc_s[tid] = sc;
  }
  __syncthreads();
  const float sc = sc_s[fr];
  uint8_t* otile = out + t * 16 * K;
  for (int kt = w; kt < (K >> 6); kt += 4) {
    const bf16x8 lo = piece(2 * kt), hi = piece(2 * kt + 1);
    *reinterpret_cast<uint4*>(otile + (static_cast<int64_t>(kt) * 64 + lane) * 16) = pack_f8_piece(lo, hi, sc);
  }
}

void launch_lora_quant_tile_f8(const bf16_t* W, int64_t ldw, const bf16_t* at, const bf16_t* b, int64_t ldb, int R,
                               float scale, const bf16_t* nw, uint8_t* out, float* scale_out, int N, int K,
                               bool glu_il, hipStream_t st) {
  const int glu_f = glu_il ? N / 2 : 0;
  if (R <= 32)
    lora_quant_tile_f8_kernel<1><<<N / 16, 256, 0, st>>>(W, ldw, at, b, ldb, R, scale, nw, out, scale_out, K, glu_f);
  else
    lora_quant_tile_f8_kernel<2><<<N / 16, 256, 0, st>>>(W, ldw, at, b, ldb, R, scale, nw, out, scale_out, K, glu_f);
}

}  // namespace dla
