// Decode-shaped MoE expert block for gfx950 (M <= 64 token rows, k <= 8 experts per token): two
// launches from route_topk's (topv, topi) to the block's output, reading expert_up [E, 2F, H] and
// expert_down [E, H, F] as the parameters are stored. Contract: moe_decode_params.h.
//
//   out[t] = bf16( sum_j topv[t, j] * ( bf16(silu(x W_g^T) * (x W_u^T)) W_d^T ) ),  experts in
//   index order, fp32 accumulation, `a` rounded to bf16 once, the per-expert y never rounded.
//
// Both kernels find an expert's rows themselves: slot s = t k + j belongs to expert e when
// topi[s] == e. A wave holds the <= 512 slots 8 per lane, and one ballot per 64 slots plus a
// popcount prefix gives e's slots in ascending order (every wave keeps its own copy of the list in
// LDS, so the list needs no workgroup barrier). An expert nobody routed to costs its ballots and
// nothing else: its weights are never loaded.
//
// Fragments (v_mfma_f32_16x16x32_bf16, as the row-major skinny kernels): lane r + 16 q loads
// W[n0 + r, k0 + 8 q .. + 8] as its B fragment (16 bytes, non-temporal: a weight byte is read once
// per step) and x[row(slot_r), k0 + 8 q .. + 8] as its A fragment straight from global memory (the
// activations are L2-resident). Lanes whose row is past the expert's count load nothing and hold
// zeros. All of an expert's row tiles (MT <= 4, picked per expert from its count) reuse the
// weight fragment. K is split across the workgroup's waves by 32-wide k-step, wave w taking steps
// w, w + W, ..., so the waves together read contiguous 64 W bytes of every weight row; each wave
// keeps a ring of D k-steps in flight. Partials meet in LDS and are summed in wave order: no
// float atomics anywhere, two runs give equal bits.
//
// Departures from the recommended design: the down kernel runs 8 waves (512 threads), not 4, so
// that its H / 16 workgroups put two waves on every SIMD of a 256-CU part; the K split is
// interleaved by k-step rather than one contiguous slice per wave, which is what lets H and F be
// any multiple of 32.
#include "common.h"
#include "moe_decode_params.h"

namespace dla {

namespace {

__device__ __forceinline__ f32x4 md_mfma(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ s16x8 md_load_w(const bf16_t* p) {
  return __builtin_bit_cast(s16x8, __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p)));
}

// the lane's share of topi: slot 64 i + lane, -1 (no expert) past the last slot
struct MdTopi {
  int v[kMdMaxTopK];
};

__device__ __forceinline__ MdTopi md_load_topi(const int* __restrict__ topi, int S, int lane) {
  MdTopi t;
#pragma unroll
  for (int i = 0; i < kMdMaxTopK; ++i) {
    const int s = 64 * i + lane;
    t.v[i] = s < S ? topi[s] : -1;
  }
  return t;
}

// expert e's slots, ascending, into this wave's list sl[0 .. count); returns count <= cap = M. A
// routing that breaks the distinct-experts precondition cannot overrun the list or the row tiles
// the LDS was sized for: slots past M are dropped.
__device__ __forceinline__ int md_slots(const MdTopi& t, int S, int cap, int e, int lane, int* sl) {
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0;
#pragma unroll
  for (int i = 0; i < kMdMaxTopK; ++i) {
    if (64 * i < S) {  // wave-uniform
      const bool hit = t.v[i] == e;
      const unsigned long long b = __ballot(hit);
      const int pos = base + __popcll(b & below);
      if (hit && pos < cap) sl[pos] = 64 * i + lane;
      base += __popcll(b);
    }
  }
  __builtin_amdgcn_wave_barrier();  // the list is read back by other lanes of this wave only
  return base < cap ? base : cap;
}

// acc[nb][t] += x tile t . W_nb^T over this wave's k-steps. wrow / xrow already point at the
// lane's row and its 8 q column offset; xrow[t] is dereferenced only where arow[t].
template <int MT, int NB, int WAVES, int D>
__device__ __forceinline__ void md_stream(const bf16_t* const (&wrow)[NB], const bf16_t* const (&xrow)[MT],
                                          const bool (&arow)[MT], int nsteps, int wave,
                                          f32x4 (&acc)[NB][MT]) {
  const int n = nsteps > wave ? (nsteps - wave + WAVES - 1) / WAVES : 0;  // this wave's k-steps
  s16x8 b[D][NB], a[D][MT];
  auto load = [&](int j, int c) {
    const int k0 = 32 * (wave + WAVES * c);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) b[j][nb] = md_load_w(wrow[nb] + k0);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      a[j][t] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (arow[t]) a[j][t] = __builtin_bit_cast(s16x8, load_bf16x8(xrow[t] + k0));
    }
  };
  auto compute = [&](int j) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb][t] = md_mfma(a[j][t], b[j][nb], acc[nb][t]);
  };
#pragma unroll
  for (int j = 0; j < D; ++j)
    if (j < n) load(j, j);
  int c0 = 0;
  for (; c0 + 2 * D <= n; c0 += D) {  // steady part: every refill is in range
#pragma unroll
    for (int j = 0; j < D; ++j) {
      compute(j);
      load(j, c0 + D + j);
    }
  }
  for (; c0 < n; c0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int c = c0 + j;
      if (c < n) {
        compute(j);
        if (c + D < n) load(j, c + D);
      }
    }
  }
}

// lane holds C[m = 16 t + 4 q + i][n = r] of its wave's partial: red[wave][nb][4 t + i][lane]
template <int MT, int NB>
__device__ __forceinline__ void md_put(float* red, int wave, int lane, const f32x4 (&acc)[NB][MT]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[((wave * NB + nb) * 4 * MT + 4 * t + i) * 64 + lane] = acc[nb][t][i];
}

template <int MT, int NB, int WAVES>
__device__ __forceinline__ float md_get(const float* red, int nb, int ti, int l) {
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += red[((w * NB + nb) * 4 * MT + ti) * 64 + l];
  return s;
}

template <int MT>
__device__ __forceinline__ void md_glu_tile(const MoeDecodeParams& p, int e, int f0, const int* sl, int count,
                                            float* red) {
  constexpr int W = kMdGluWaves, D = MT <= 2 ? 8 : 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const bf16_t* gate = p.w_up + (static_cast<int64_t>(e) * 2 * p.F + f0 + r) * p.H + 8 * q;
  const bf16_t* const wrow[2] = {gate, gate + static_cast<int64_t>(p.F) * p.H};
  bool arow[MT];
  const bf16_t* xrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    arow[t] = 16 * t + r < count;
    xrow[t] = p.h2 + (arow[t] ? static_cast<int64_t>(sl[16 * t + r] / p.k) * p.ldh : 0) + 8 * q;
  }
  f32x4 acc[2][MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  md_stream<MT, 2, W, D>(wrow, xrow, arow, p.H >> 5, wave, acc);
  md_put<MT, 2>(red, wave, lane, acc);
  __syncthreads();
  for (int i = threadIdx.x; i < 256 * MT; i += 64 * W) {
    const int ti = i >> 6, l = i & 63;
    const int m = 16 * (ti >> 2) + 4 * (l >> 4) + (ti & 3);
    if (m < count) {
      const float g = md_get<MT, 2, W>(red, 0, ti, l), u = md_get<MT, 2, W>(red, 1, ti, l);
      p.a[static_cast<int64_t>(sl[m]) * p.F + f0 + (l & 15)] = f2bf(g * sigmoidf_(g) * u);
    }
  }
}

template <int MT>
__device__ __forceinline__ void md_down_tile(const MoeDecodeParams& p, int e, int n0, const int* sl, int count,
                                             float* red, float* out_acc) {
  constexpr int W = kMdDownWaves, D = 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const bf16_t* const wrow[1] = {p.w_down + (static_cast<int64_t>(e) * p.H + n0 + r) * p.F + 8 * q};
  bool arow[MT];
  const bf16_t* xrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    arow[t] = 16 * t + r < count;
    xrow[t] = p.a + (arow[t] ? static_cast<int64_t>(sl[16 * t + r]) * p.F : 0) + 8 * q;
  }
  f32x4 acc[1][MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  md_stream<MT, 1, W, D>(wrow, xrow, arow, p.F >> 5, wave, acc);
  __syncthreads();  // the previous expert's sums have been read
  md_put<MT, 1>(red, wave, lane, acc);
  __syncthreads();
  // a token has this expert at most once, so each out_acc element has one writer per expert,
  // and the barriers order the experts: a fixed summation order
  for (int i = threadIdx.x; i < 256 * MT; i += 64 * W) {
    const int ti = i >> 6, l = i & 63;
    const int m = 16 * (ti >> 2) + 4 * (l >> 4) + (ti & 3);
    if (m < count) {
      const int s = sl[m];
      out_acc[(s / p.k) * 16 + (l & 15)] += p.topv[s] * md_get<MT, 1, W>(red, 0, ti, l);
    }
  }
}

}  // namespace

// LDS: slots[waves][64] int, then red[waves][NB][4 mt][64] fp32 with mt = ceil(M / 16) row tiles
__global__ __launch_bounds__(64 * kMdGluWaves) void moe_decode_glu_kernel(const MoeDecodeParams p) {
  extern __shared__ float md_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.y, f0 = 16 * blockIdx.x, S = p.M * p.k;
  int* sl = reinterpret_cast<int*>(md_lds) + wave * kMdMaxRows;
  float* red = md_lds + kMdGluWaves * kMdMaxRows;
  const MdTopi topi = md_load_topi(p.topi, S, lane);
  const int count = md_slots(topi, S, p.M, e, lane, sl);
  if (count == 0) return;  // workgroup-uniform: nobody routed here, no weight is touched
  switch ((count + 15) >> 4) {
    case 1: md_glu_tile<1>(p, e, f0, sl, count, red); break;
    case 2: md_glu_tile<2>(p, e, f0, sl, count, red); break;
    case 3: md_glu_tile<3>(p, e, f0, sl, count, red); break;
    default: md_glu_tile<4>(p, e, f0, sl, count, red); break;
  }
}

// LDS: out_acc[M][16] fp32, slots[waves][64] int, red[waves][4 mt][64] fp32
__global__ __launch_bounds__(64 * kMdDownWaves) void moe_decode_down_kernel(const MoeDecodeParams p) {
  extern __shared__ float md_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = 16 * blockIdx.x, S = p.M * p.k;
  float* out_acc = md_lds;
  int* sl = reinterpret_cast<int*>(md_lds + p.M * 16) + wave * kMdMaxRows;
  float* red = md_lds + p.M * 16 + kMdDownWaves * kMdMaxRows;
  for (int i = threadIdx.x; i < p.M * 16; i += 64 * kMdDownWaves) out_acc[i] = 0.f;
  const MdTopi topi = md_load_topi(p.topi, S, lane);
  for (int e = 0; e < p.E; ++e) {
    const int count = md_slots(topi, S, p.M, e, lane, sl);
    if (count == 0) continue;  // workgroup-uniform
    switch ((count + 15) >> 4) {
      case 1: md_down_tile<1>(p, e, n0, sl, count, red, out_acc); break;
      case 2: md_down_tile<2>(p, e, n0, sl, count, red, out_acc); break;
      case 3: md_down_tile<3>(p, e, n0, sl, count, red, out_acc); break;
      default: md_down_tile<4>(p, e, n0, sl, count, red, out_acc); break;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < p.M * 16; i += 64 * kMdDownWaves)
    p.out[static_cast<int64_t>(i >> 4) * p.H + n0 + (i & 15)] = f2bf(out_acc[i]);
}

void launch_moe_decode_glu(const MoeDecodeParams& p, hipStream_t st) {
  const int mt = (p.M + 15) / 16;
  const size_t lds = sizeof(float) * (kMdGluWaves * kMdMaxRows + kMdGluWaves * 2 * 4 * mt * 64);
  moe_decode_glu_kernel<<<dim3(p.F / 16, p.E), 64 * kMdGluWaves, lds, st>>>(p);
}

void launch_moe_decode_down(const MoeDecodeParams& p, hipStream_t st) {
  const int mt = (p.M + 15) / 16;
  const size_t lds = sizeof(float) * (p.M * 16 + kMdDownWaves * kMdMaxRows + kMdDownWaves * 4 * mt * 64);
  moe_decode_down_kernel<<<dim3(p.H / 16), 64 * kMdDownWaves, lds, st>>>(p);
}

}  // namespace dla
