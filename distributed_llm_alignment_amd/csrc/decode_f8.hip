// e4m3 KV cache for rollouts: the quantising cache writes and split-KV decode attention over codes.
//
// Decode streams the whole cache once per token; with one byte per element plus one fp32 scale per
// (token, kv head) row for K and for V (decode_f8_params.h: format of record) that stream is
// (1 + 4/D) / 2 of the bf16 one. Three kernels:
//   * kv_quant_f8_kernel     prefill: a layer's prompt K / V slab -> codes + scales (pure stream);
//   * rope_cache_f8_kernel   decode prologue: rope q / k of the newest token, quantise k / v into
//                            the cache slot (device value: graph-capturable);
//   * decode_attn_f8_kernel  split-KV attention, the geometry of decode.hip's loop kernel (grid
//                            (splits, Hkv, B), 128-key chunks, a wave per 32 keys, fp32 partials in
//                            the same layout so decode_combine_kernel merges them) around a data
//                            path built for bytes, described at the kernel.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "decode_f8_params.h"
#include "decode_geom.h"
#include "decode_params.h"
#include "decode_rope.h"

namespace dla {

// ---- quantiser shared by the two cache-write kernels. LPK = D / 8 lanes own one head row, 8
// elements each; the row's amax crosses the (aligned) lane group by xor shuffles. Divide and
// reciprocal are the correctly rounded ones (__fdiv_rn / __frcp_rn never lower to v_rcp_f32 + a
// multiply), the product is a single fp32 multiply: the CPU formula's bits.
template <int LPK>
__device__ __forceinline__ uint2 kv_quant8(const bf16x8& x, float* sc_out) {
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(bf2f(x[j])));
#pragma unroll
  for (int o = LPK / 2; o >= 1; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
  const float sc = fmaxf(__fdiv_rn(am, 448.f), 1e-12f);
  const float inv = __frcp_rn(sc);
  auto q = [&](int j) { return fminf(fmaxf(bf2f(x[j]) * inv, -448.f), 448.f); };
  uint32_t w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q(0), q(1), 0u, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q(2), q(3), w0, true);
  uint32_t w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q(4), q(5), 0u, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q(6), q(7), w1, true);
  *sc_out = sc;
  return make_uint2(w0, w1);
}

// ---- 1. prefill fill. Row r = (b, outer, inner) with the two middle dims ordered by the
// destination's strides (host), so consecutive lane groups walk the code storage in memory order.
// A thread issues kQuantRows independent 16-byte loads before the first use; a lane group stores
// 8 bytes per lane and one scale. No LDS, no atomics: one read of the slab, one write at half size.
constexpr int kQuantRows = 4;

struct KvQuantGeom {
  int64_t s_a, s_b, c_a, c_b, z_a, z_b;  // strides of the outer / inner middle dim
  int na, nb;
  int64_t rows;
};

template <int LPK>
__global__ __launch_bounds__(256) void kv_quant_f8_kernel(KvQuantParams p, KvQuantGeom g) {
  constexpr int RPB = 256 / LPK;  // rows per block per pass
  const int sub = threadIdx.x / LPK, dl = (threadIdx.x % LPK) * 8;
  const int64_t r0 = (int64_t)blockIdx.x * RPB * kQuantRows + sub;
  bf16x8 x[kQuantRows];
  int64_t coff[kQuantRows], zoff[kQuantRows];
  bool ok[kQuantRows];
#pragma unroll
  for (int i = 0; i < kQuantRows; ++i) {
    const int64_t r = r0 + (int64_t)i * RPB;
    ok[i] = r < g.rows;
    const int64_t rc = ok[i] ? r : g.rows - 1;  // (a whole lane group is in or out together)
    const int ib = (int)(rc % g.nb);
    const int ia = (int)((rc / g.nb) % g.na);
    const int b = (int)(rc / ((int64_t)g.nb * g.na));
    x[i] = load_bf16x8(p.src + (int64_t)b * p.s_sb + ia * g.s_a + ib * g.s_b + dl);
    coff[i] = (int64_t)b * p.c_sb + ia * g.c_a + ib * g.c_b + dl;
    zoff[i] = (int64_t)b * p.z_sb + ia * g.z_a + ib * g.z_b;
  }
#pragma unroll
  for (int i = 0; i < kQuantRows; ++i) {
    float sc;
    const uint2 w = kv_quant8<LPK>(x[i], &sc);
    if (ok[i]) {
      *reinterpret_cast<uint2*>(p.codes + coff[i]) = w;
      if (dl == 0) p.scale[zoff[i]] = sc;
    }
  }
}

void launch_kv_quant_f8(const KvQuantParams& p, hipStream_t st) {
  if (p.B == 0 || p.T == 0 || p.Hkv == 0) return;
  KvQuantParams q = p;  // token t0 folded into the destination bases
  q.codes += (int64_t)p.t0 * p.c_st;
  q.scale += (int64_t)p.t0 * p.z_st;
  KvQuantGeom g;
  if (p.c_sh > p.c_st) {  // head-major storage: a head's tokens contiguous, walk (h, t)
    g = KvQuantGeom{p.s_sh, p.s_st, p.c_sh, p.c_st, p.z_sh, p.z_st, p.Hkv, p.T, 0};
  } else {
    g = KvQuantGeom{p.s_st, p.s_sh, p.c_st, p.c_sh, p.z_st, p.z_sh, p.T, p.Hkv, 0};
  }
  g.rows = (int64_t)p.B * p.T * p.Hkv;
  const int lpk = p.D / 8;
  const int64_t per_block = (int64_t)(256 / lpk) * kQuantRows;
  const unsigned grid = (unsigned)((g.rows + per_block - 1) / per_block);
  if (p.D == 128) kv_quant_f8_kernel<16><<<grid, 256, 0, st>>>(q, g);
  else kv_quant_f8_kernel<8><<<grid, 256, 0, st>>>(q, g);
}

// ---- 2. decode-step prologue: rope_cache_kernel with a quantising write. LPK lanes own one head
// row, a wave 64 / LPK of them. Waves [0, nqw) take the B * Hq query rows (rotated into q_out by
// dec_rope8: the rounding of rope_cache_kernel and of the fused prologue, nothing else); the waves
// after them take the B * 2 Hkv key / value rows (k rotated and rounded to bf16, v as it is), which
// alone pay for the quantiser (amax shuffles, the divide and the reciprocal); codes and the scale go
// to cache slot *slot. The branch is uniform per wave, so the shuffles see whole waves.
template <int LPK>
__global__ __launch_bounds__(256) void rope_cache_f8_kernel(RopeCacheF8Params p, int nqw, int nwaves) {
  constexpr int D = LPK * 8, RPW = 64 / LPK;
  const int half = p.rot >> 1;
  const int lane = threadIdx.x & 63, sub = lane / LPK, dl = (lane % LPK) * 8;
  const int64_t t_slot = p.slot[0];
  for (int gw = blockIdx.x * 4 + (threadIdx.x >> 6); gw < nwaves; gw += gridDim.x * 4) {
    if (gw < nqw) {
      const int64_t r = (int64_t)gw * RPW + sub;
      if (r >= (int64_t)p.B * p.Hq) continue;
      const int h = (int)(r % p.Hq), b = (int)(r / p.Hq);
      const float* cs = p.cos_t + (int64_t)p.pos[b] * half;
      const float* sn = p.sin_t + (int64_t)p.pos[b] * half;
      store_bf16x8(p.q_out + r * D + dl, dec_rope8(p.qkv + (int64_t)b * p.ld + (int64_t)h * D, dl, p.rot, cs, sn));
      continue;
    }
    const int64_t total = (int64_t)p.B * 2 * p.Hkv;
    const int64_t r = (int64_t)(gw - nqw) * RPW + sub;
    const bool ok = r < total;
    const int64_t rc = ok ? r : total - 1;  // (a whole lane group is in or out together)
    const int h2 = (int)(rc % (2 * p.Hkv)), b = (int)(rc / (2 * p.Hkv));
    const bool isv = h2 >= p.Hkv;
    const int hk = h2 - (isv ? p.Hkv : 0);
    const bf16_t* s = p.qkv + (int64_t)b * p.ld + (int64_t)(p.Hq + h2) * D;
    const float* cs = p.cos_t + (int64_t)p.pos[b] * half;
    const float* sn = p.sin_t + (int64_t)p.pos[b] * half;
    const bf16x8 x = isv ? load_bf16x8(s + dl) : dec_rope8(s, dl, p.rot, cs, sn);
    float sc;
    const uint2 w = kv_quant8<LPK>(x, &sc);  // (every lane of the wave: the shuffles want it whole)
    if (!ok) continue;
    uint8_t* codes = (isv ? p.c.v8 : p.c.k8) + (int64_t)b * p.c.c_sb + t_slot * p.c.c_st + (int64_t)hk * p.c.c_sh;
    *reinterpret_cast<uint2*>(codes + dl) = w;
    if (dl == 0) (isv ? p.c.vs : p.c.ks)[(int64_t)b * p.c.z_sb + t_slot * p.c.z_st + (int64_t)hk * p.c.z_sh] = sc;
  }
}

void launch_rope_cache_f8(const RopeCacheF8Params& p, hipStream_t st) {
  const int rpw = 64 / (p.D / 8);
  const int64_t nqw = ((int64_t)p.B * p.Hq + rpw - 1) / rpw;
  const int64_t nkw = ((int64_t)p.B * 2 * p.Hkv + rpw - 1) / rpw;
  const int64_t nwaves = nqw + nkw;
  const unsigned grid = (unsigned)std::min<int64_t>((nwaves + 3) / 4, 1024);
  if (grid == 0) return;
  if (p.D == 128) rope_cache_f8_kernel<16><<<grid, 256, 0, st>>>(p, (int)nqw, (int)nwaves);
  else rope_cache_f8_kernel<8><<<grid, 256, 0, st>>>(p, (int)nqw, (int)nwaves);
}

// ---- 3. decode attention over codes.
//
// Work split as decode.hip's loop kernel: a block owns one kv head, all G = Hq / Hkv query heads
// and `cpb` consecutive 128-key chunks; a wave takes 32 keys of each chunk and keeps its own
// online softmax across chunks; the 4 waves merge once at the end.
//
// Data path (per wave and chunk):
//   K   lane (r16 = key in a 16-key tile, kg) loads 16 bytes = dims [64 j + 16 kg, + 16) of its
//       key: TWO k-steps of v_mfma_f32_16x16x32_bf16 per load (the bf16 kernel gets one). The k
//       index of the MFMA is permuted (k-step 2 j + e, lane group kg <-> dims 64 j + 16 kg + 8 e +
//       [0, 8)); the bf16 q fragment is loaded with the same permutation, so S^T = K q^T is the
//       plain dot product. Codes become bf16 in registers (f8x8_to_bf16, exact).
//   ks  the key's scale multiplies the fp32 score together with scale_log2, before mask and max.
//   V   a row is D bytes: D / 16 lanes cover it, a wave instruction covers 128 / (D / 8) rows
//       (twice the bf16 kernel's). The codes wait in a register ring, are converted to bf16 in
//       registers and stored into the wave-private swizzled LDS image (dec_swz of decode.hip) that
//       ds_read_b64_tr_b16 reads back as the B operand of the P.V MFMA. ONE image per wave (the
//       ring is in registers): 32 KB of LDS per block against the bf16 kernel's 64 KB.
//   vs  folded into the probability as it is packed to bf16 (bf16(p * vs[t])); the row sum l
//       accumulates the unscaled p in fp32.
//   scales: lanes 0..31 load the wave's 32 K scales and lanes 32..63 its 32 V scales in one
//       instruction (two 128-byte runs in the head-major layout) issued with the chunk's K / V
//       loads; each lane fetches the 8 + 8 values of its own keys by ds_bpermute.
// Ring: chunk c + 2's loads are issued when chunk c has been consumed (2 slots of K codes, V codes
// and scales in registers); the compiler's vmcnt tracking orders them (no LDS-DMA here).
// Reads: the split's first chunk of K is loaded speculatively, before kv_len has arrived, with rows
// clamped only into the cache capacity: in that one chunk rows at or beyond kv_len (inside the
// tensor, possibly uninitialised bytes) ARE read and DO enter the QK MFMA. A garbage or NaN code
// touches only its own key's row of S^T, and that score is replaced by -inf by a select before
// the max, so it is discarded per key. Every later K row, every V row and every scale is clamped
// into the visible range [k0, k1) of its chunk: a masked key has p = 0 exactly, a finite V row
// and a finite V scale, so nothing from beyond kv_len reaches the softmax or P.V.
template <int D>
__device__ __forceinline__ int f8_swz(int row, int ch) {  // decode.hip dec_swz
  constexpr int NCH = D / 8;
  const int f = (((row & 3) << 2) | ((row >> 2) & 3)) & (NCH - 1);
  return row * D + ((ch ^ f) << 3);
}

typedef __attribute__((address_space(3))) s16x4 f8_lds_s16x4;

// ds_read_b64_tr_b16 of 4 key rows x 16 columns (decode.hip dec_tr_read); EXEC must be all ones
template <int D>
__device__ __forceinline__ s16x4 f8_tr_read(const bf16_t* img, int r0, int c0, int lane) {
  const int i = lane & 15, q = i >> 2, pp = i & 3;
  const int ch = (c0 >> 3) + (pp >> 1), sub = (pp & 1) * 4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((f8_lds_s16x4*)(img + f8_swz<D>(r0 + q, ch) + sub));
}

template <int D, int G>
__global__ __launch_bounds__(256, 2) void decode_attn_f8_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh,
    const uint8_t* __restrict__ k8, const uint8_t* __restrict__ v8, int64_t c_sb, int64_t c_st, int64_t c_sh,
    const float* __restrict__ ksc, const float* __restrict__ vsc, int64_t z_sb, int64_t z_st, int64_t z_sh,
    const int* __restrict__ kv_len, const int* __restrict__ kv_start, int window, float scale_log2,
    int nsplit, int cpb, float* __restrict__ part_o, float* __restrict__ part_ml, int Hq,
    bf16_t* __restrict__ out, int64_t o_sb, int64_t o_sh, int Tcap) {
  constexpr int KPW = kDecChunk / 4;         // keys per wave and chunk
  constexpr int KLD = D / 64;                // 16-byte K loads per key tile (2 k-steps each)
  constexpr int KST = D / 32;                // MFMA k-steps over the head dim
  constexpr int LPV = D / 16, RPI = 64 / LPV, NIV = KPW / RPI;  // V: lanes per row, rows / instruction
  constexpr int RD = 2;
  static_assert(G <= 16 && KPW == 32, "decode tile geometry");
  static_assert(G * D * 4 <= KPW * D * 2, "the wave's partial O aliases its V image");
  __shared__ __attribute__((aligned(16))) bf16_t vimg[4][KPW * D];
  __shared__ float mls[4][G][2];
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kg = lane >> 4;   // MFMA fragment layout
  const int vsub = lane / LPV, vl = lane % LPV;  // V row layout: row vsub of the pass, bytes 16 vl ..
  const int len = min(kv_len[0], Tcap);  // (never past the cache, whatever the device value says)
  int lo = kv_start ? max(kv_start[b], 0) : 0;
  const int cfirst = split * cpb;
  const uint8_t* kb0 = k8 + (int64_t)b * c_sb + (int64_t)hk * c_sh + 16 * kg;
  const uint8_t* vb0 = v8 + (int64_t)b * c_sb + (int64_t)hk * c_sh + 16 * vl;
  // lanes 0..31: K scales, 32..63: V scales of key (lane & 31) of the wave
  const float* zb0 = (lane < 32 ? ksc : vsc) + (int64_t)b * z_sb + (int64_t)hk * z_sh;
  uint4 kf[RD][2][KLD];
  uint4 vf[RD][NIV];
  float zf[RD];
  // rows clamped into [klo, khi]
  auto loadK = [&](auto J, int c, int klo, int khi) {
    constexpr int j = decltype(J)::value;
    const int kw0 = c * kDecChunk + wv * KPW;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = min(max(kw0 + 16 * t + r16, klo), khi);
#pragma unroll
      for (int s = 0; s < KLD; ++s)
        kf[j][t][s] = *reinterpret_cast<const uint4*>(kb0 + (int64_t)key * c_st + 64 * s);
    }
  };
  loadK(std::integral_constant<int, 0>{}, cfirst, 0, Tcap - 1);  // speculative: the split's first chunk
  if (window > 0) lo = max(lo, len - window);
  const int cbeg = max(cfirst, lo / kDecChunk);
  const int cend = min(cfirst + cpb, (len + kDecChunk - 1) / kDecChunk);
  const int64_t pbase = ((int64_t)b * Hq + (int64_t)hk * G) * nsplit + split;
  if (cbeg >= cend || max(cbeg * kDecChunk, lo) >= len) {  // no visible key in this split
    if (out != nullptr) {  // one split per sequence: zeros, as the combine writes for an all-empty row
      for (int i = tid; i < G * D; i += 256)
        out[(int64_t)b * o_sb + (int64_t)(hk * G + i / D) * o_sh + i % D] = 0;
      return;
    }
    if (tid < G) {
      part_ml[(pbase + (int64_t)tid * nsplit) * 2 + 0] = -INFINITY;
      part_ml[(pbase + (int64_t)tid * nsplit) * 2 + 1] = 0.f;
    }
    return;
  }
  // q fragments in the permuted k order of the K loads
  s16x8 qf[KST];
#pragma unroll
  for (int s = 0; s < KST; ++s) {
    qf[s] = s16x8{};
    if (r16 < G)
      qf[s] = __builtin_bit_cast(s16x8, load_bf16x8(q + (int64_t)b * q_sb + (int64_t)(hk * G + r16) * q_sh +
                                                    64 * (s >> 1) + 16 * kg + 8 * (s & 1)));
  }
  auto loadVZ = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int base = c * kDecChunk, k0 = max(base, lo), k1 = min(base + kDecChunk, len);
    const int kw0 = base + wv * KPW;
    zf[j] = zb0[(int64_t)min(max(kw0 + (lane & 31), k0), k1 - 1) * z_st];
#pragma unroll
    for (int it = 0; it < NIV; ++it) {
      const int key = min(max(kw0 + it * RPI + vsub, k0), k1 - 1);
      vf[j][it] = *reinterpret_cast<const uint4*>(vb0 + (int64_t)key * c_st);
    }
  };
  auto load = [&](auto J, int c) {  // issue order per chunk: K, scales, V
    const int base = c * kDecChunk;
    loadK(J, c, max(base, lo), min(base + kDecChunk, len) - 1);
    loadVZ(J, c);
  };
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 oacc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16_t* vw = &vimg[wv][0];
  auto step = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int base = c * kDecChunk, k0 = max(base, lo), k1 = min(base + kDecChunk, len);
    const int kw0 = base + wv * KPW;
    // ---- S^T[key][g]: lane holds keys kw0 + 16 t + 4 kg + i (i < 4) of head g = r16
    f32x4 sacc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KLD; ++s) {
        const uint4 w = kf[j][t][s];
        sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f8x8_to_bf16(w.x, w.y), qf[2 * s], sacc[t], 0, 0, 0);
        sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f8x8_to_bf16(w.z, w.w), qf[2 * s + 1], sacc[t], 0, 0, 0);
      }
    }
    float sc[2][4], vs[2][4];
    float mc = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kl = 16 * t + 4 * kg + i, key = kw0 + kl;
        const float ks = __shfl(zf[j], kl, 64);
        vs[t][i] = __shfl(zf[j], 32 + kl, 64);
        sc[t][i] = (key >= k0 && key < k1) ? sacc[t][i] * (ks * scale_log2) : -INFINITY;
        mc = fmaxf(mc, sc[t][i]);
      }
    mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    const float mnew = fmaxf(m_run, mc);
    const float alpha = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - mnew);
    const float muse = mnew == -INFINITY ? 0.f : mnew;
    float pv8[8], ls = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(sc[t][i] - muse);  // exp2(-inf) = 0 for masked keys
        ls += p;
        pv8[4 * t + i] = r16 < G ? p * vs[t][i] : 0.f;
      }
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    l_run = l_run * alpha + ls;
    m_run = mnew;
    // A operand: k-slot e < 4 <-> key 4 kg + e, e >= 4 <-> key 16 + 4 kg + e - 4
    const s16x8 pa = __builtin_bit_cast(s16x8, pack_bf16x8(pv8));
    float ai[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ai[i] = __shfl(alpha, 4 * kg + i, 64);
    // ---- V codes -> bf16 -> the wave's swizzled image (the previous chunk's transposed reads were
    // issued earlier by this wave; LDS operations of one wave execute in order)
#pragma unroll
    for (int it = 0; it < NIV; ++it) {
      const uint4 w = vf[j][it];
      const int row = it * RPI + vsub;
      store_bf16x8(vw + f8_swz<D>(row, 2 * vl), __builtin_bit_cast(bf16x8, f8x8_to_bf16(w.x, w.y)));
      store_bf16x8(vw + f8_swz<D>(row, 2 * vl + 1), __builtin_bit_cast(bf16x8, f8x8_to_bf16(w.z, w.w)));
    }
    if (c + RD < cend) load(J, c + RD);  // slot j is consumed: refill it two chunks ahead
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      const s16x4 v0 = f8_tr_read<D>(vw, 4 * kg, 16 * dt, lane);
      const s16x4 v1 = f8_tr_read<D>(vw, 16 + 4 * kg, 16 * dt, lane);
      const s16x8 vb = s16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      f32x4 o = oacc[dt];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] *= ai[i];
      oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, o, 0, 0, 0);
    }
    // WAR on the image: the transposed reads have returned before the next chunk's stores
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  };
  if (cbeg != cfirst)  // left padding: the guess was wrong
    loadK(std::integral_constant<int, 0>{}, cbeg, max(cbeg * kDecChunk, lo), min((cbeg + 1) * kDecChunk, len) - 1);
  loadVZ(std::integral_constant<int, 0>{}, cbeg);
  if (cbeg + 1 < cend) load(std::integral_constant<int, 1>{}, cbeg + 1);
  for (int c = cbeg; c < cend; c += RD) {
    step(std::integral_constant<int, 0>{}, c);
    if (c + 1 < cend) step(std::integral_constant<int, 1>{}, c + 1);
  }
  // ---- this wave's partial O into its own (dead) image, then the 4 waves merge in a fixed order
  float* acc_w = reinterpret_cast<float*>(vw);
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4 * kg + i < G) acc_w[(4 * kg + i) * D + 16 * dt + r16] = oacc[dt][i];
  if (kg == 0 && r16 < G) {
    mls[wv][r16][0] = m_run;
    mls[wv][r16][1] = l_run;
  }
  __syncthreads();
  for (int i = tid; i < G * D; i += 256) {
    const int g = i / D, d = i % D;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mm = fmaxf(mm, mls[w][g][0]);
    float v = 0.f, ll = 0.f;
    if (mm != -INFINITY) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float mw = mls[w][g][0];
        const float cc = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mm);
        v += cc * reinterpret_cast<const float*>(&vimg[w][0])[g * D + d];
        ll += cc * mls[w][g][1];
      }
    }
    if (out != nullptr) {
      out[(int64_t)b * o_sb + (int64_t)(hk * G + g) * o_sh + d] = f2bf(ll > 0.f ? v * (1.f / ll) : 0.f);
      continue;
    }
    part_o[(pbase + (int64_t)g * nsplit) * D + d] = v;
    if (d == 0) {
      part_ml[(pbase + (int64_t)g * nsplit) * 2 + 0] = mm;
      part_ml[(pbase + (int64_t)g * nsplit) * 2 + 1] = ll;
    }
  }
}

// ---- host side. Split geometry of decode_geom.h; where it asks for the one-chunk kernel (cpb 0)
// the loop kernel runs with one chunk per block: the same grid and partial layout.
static int f8_cpb(const DecodeF8Params& p) { return std::max(decode_cpb(p.c.Tmax, p.B, p.Hkv), 1); }

int decode_f8_splits(const DecodeF8Params& p) {
  const int nch = (p.c.Tmax + kDecChunk - 1) / kDecChunk, cpb = f8_cpb(p);
  return (nch + cpb - 1) / cpb;
}

template <int D, int G>
static void launch_decode_f8_t(const DecodeF8Params& p, hipStream_t st) {
  const int cpb = f8_cpb(p), nsplit = decode_f8_splits(p);
  bf16_t* fin = nsplit == 1 ? p.out : nullptr;  // one split per sequence: no combine launch
  decode_attn_f8_kernel<D, G><<<dim3(nsplit, p.Hkv, p.B), 256, 0, st>>>(
      p.q, p.q_sb, p.q_sh, p.c.k8, p.c.v8, p.c.c_sb, p.c.c_st, p.c.c_sh, p.c.ks, p.c.vs, p.c.z_sb, p.c.z_st,
      p.c.z_sh, p.kv_len, p.kv_start, p.window, p.scale_log2, nsplit, cpb, p.part_o, p.part_ml, p.Hq, fin,
      p.o_sb, p.o_sh, p.c.Tmax);
  if (fin == nullptr) launch_decode_combine_parts(p.part_o, p.part_ml, nsplit, p.out, p.o_sb, p.o_sh, p.B, p.Hq, D, st);
}

void launch_decode_f8(const DecodeF8Params& p, hipStream_t st) {
  auto heads = [&](auto d) {
    constexpr int D = decltype(d)::value;
    switch (p.Hq / p.Hkv) {
      case 1: launch_decode_f8_t<D, 1>(p, st); break;
      case 2: launch_decode_f8_t<D, 2>(p, st); break;
      case 4: launch_decode_f8_t<D, 4>(p, st); break;
      case 8: launch_decode_f8_t<D, 8>(p, st); break;
      default: break;  // (validated by the binding)
    }
  };
  if (p.D == 128) heads(std::integral_constant<int, 128>{});
  else heads(std::integral_constant<int, 64>{});
}

}  // namespace dla
