// Shared-prefill KV replication for group rollouts (generate(num_return_sequences = G)).
//
// The prompt of each of P groups is prefilled once into a P-row cache; this kernel copies the
// keys / values [0, Tp) of every layer from source row p into destination rows p*G .. p*G+G-1 of
// the P*G-row decode cache: ONE launch for K and V of all layers, each 16-byte vector of the
// source read once and stored G times (plain vector stores). Key positions >= Tp of the
// destination are never addressed.
//
// Both caches are [L, rows, T, Hkv, D] views with explicit strides (innermost D contiguous), so the
// head-major storage ([L, B, Hkv, T, D] behind the view) and the token-major layout both work.
// The launcher orders the two middle dimensions (T, Hkv) by the destination's strides so that
// consecutive lanes walk the destination's memory order: a wave's load and each of its G stores
// cover one contiguous 1 KiB run in the common case (pure copy: no LDS, no atomics).
#include "common.h"

namespace dla {

struct KvRepParams {
  const bf16_t* src[2];  // K, V of the P-row prefill cache
  bf16_t* dst[2];        // K, V of the P*G-row decode cache
  // strides in elements: layer, row, outer middle dim (A), inner middle dim (Bn)
  int64_t s_l, s_r, s_a, s_b;
  int64_t d_l, d_r, d_a, d_b;
  int P, G, nb, dv;      // nb: size of the inner middle dim, dv: D / 8 vectors per head row
  int64_t nvec;          // 16-byte vectors per (layer, source row): A * nb * dv
};

constexpr int kKvRepThreads = 256;
constexpr int kKvRepUnroll = 4;  // independent 16 B loads in flight per lane

__global__ __launch_bounds__(kKvRepThreads) void kv_replicate_kernel(KvRepParams p) {
  const int lp = blockIdx.y;  // layer * P + prompt row
  const int l = lp / p.P, row = lp - l * p.P;
  const int which = blockIdx.z;
  const bf16_t* __restrict__ src = p.src[which] + l * p.s_l + row * p.s_r;
  bf16_t* __restrict__ dst = p.dst[which] + l * p.d_l + static_cast<int64_t>(row) * p.G * p.d_r;
  const int64_t per_block = static_cast<int64_t>(kKvRepThreads) * kKvRepUnroll;
  const int per_a = p.nb * p.dv;
  for (int64_t base = blockIdx.x * per_block; base < p.nvec; base += gridDim.x * per_block) {
    bf16x8 v[kKvRepUnroll];
    int64_t doff[kKvRepUnroll];
#pragma unroll
    for (int i = 0; i < kKvRepUnroll; ++i) {
      const int64_t idx = base + i * kKvRepThreads + threadIdx.x;
      if (idx < p.nvec) {
        const int64_t a = idx / per_a;
        const int rem = static_cast<int>(idx - a * per_a);
        const int b = rem / p.dv, d = (rem - b * p.dv) * 8;
        v[i] = load_bf16x8(src + a * p.s_a + b * p.s_b + d);
        doff[i] = a * p.d_a + b * p.d_b + d;
      }
    }
#pragma unroll
    for (int i = 0; i < kKvRepUnroll; ++i) {
      const int64_t idx = base + i * kKvRepThreads + threadIdx.x;
      if (idx < p.nvec) {
        for (int g = 0; g < p.G; ++g) store_bf16x8(dst + g * p.d_r + doff[i], v[i]);
      }
    }
  }
}

// Sizes: [L, P, Tp, H, D] source, [L, P*G, >= Tp, H, D] destination; strides in elements as
// (layer, row, T, H). The caller has checked alignment (16 B bases, strides % 8 == 0, D % 8 == 0).
void launch_kv_replicate(const bf16_t* sk, const bf16_t* sv, bf16_t* dk, bf16_t* dv_, int L, int P,
                         int G, int Tp, int H, int D, const int64_t* sstr, const int64_t* dstr,
                         hipStream_t st) {
  if (L == 0 || P == 0 || G == 0 || Tp == 0 || H == 0 || D == 0) return;
  KvRepParams p;
  p.src[0] = sk, p.src[1] = sv, p.dst[0] = dk, p.dst[1] = dv_;
  p.s_l = sstr[0], p.s_r = sstr[1], p.d_l = dstr[0], p.d_r = dstr[1];
  const bool head_major = dstr[3] > dstr[2];  // a head's keys contiguous: walk (h, t, d)
  int na;
  if (head_major) {
    na = H, p.nb = Tp;
    p.s_a = sstr[3], p.s_b = sstr[2], p.d_a = dstr[3], p.d_b = dstr[2];
  } else {
    na = Tp, p.nb = H;
    p.s_a = sstr[2], p.s_b = sstr[3], p.d_a = dstr[2], p.d_b = dstr[3];
  }
  p.P = P, p.G = G, p.dv = D / 8;
  p.nvec = static_cast<int64_t>(na) * p.nb * p.dv;
  const int64_t per_block = static_cast<int64_t>(kKvRepThreads) * kKvRepUnroll;
  int64_t gx = (p.nvec + per_block - 1) / per_block;
  if (gx > 1024) gx = 1024;
  dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(L * P), 2);
  kv_replicate_kernel<<<grid, kKvRepThreads, 0, st>>>(p);
}

}  // namespace dla
