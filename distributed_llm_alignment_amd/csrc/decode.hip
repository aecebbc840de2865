// Single-token decode attention over a KV cache (RLHF rollouts, teacher generation,
// eval — reference src/training/train_rlhf.py:123-124 / generate_teacher_data.py:72-79 via HF
// `generate`).
//
// Decode is bandwidth bound: each step streams the whole KV cache once. Design:
//   * split-KV (flash-decoding): grid = (splits, Hkv, B); a block owns one KV head, ALL its
//     G = Hq/Hkv query heads (GQA: the K/V rows are read once, not G times) and a 128-key chunk;
//   * each wave takes 32 keys of the chunk: S^T = K q^T on MFMA (K rows as A fragments), a
//     wave-local softmax, P.V on the VALU over V rows read coalesced (D/8 lanes x 16 B per row);
//     the 4 waves merge once at the end (see decode_attn_kernel);
//   * partial (m, l, o) per split in fp32, merged by `decode_combine_kernel`.
// Lengths are DEVICE values (kv_len scalar, per-row kv_start for left padding), so the same
// launch replays inside a captured hipGraph while the cache grows; splits beyond kv_len exit.
// Group rollouts whose rows share a prompt prefix have a two-launch form that reads the prefix once
// per group (DecGroup, decode_prefix_kernel, launch_decode below).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "decode_geom.h"
#include "decode_params.h"

namespace dla {

// Lanes cooperate on rows: LPK = D/8 lanes x 16 B cover one K/V row (coalesced 256-byte rows
// for D = 128), KPI = 64/LPK rows per wave instruction.

// 8 rotated dims [d0, d0 + 8) of one head (rotate-half over the first `rot` dims), rounded to bf16
__device__ __forceinline__ bf16x8 dec_rope8(const bf16_t* src, int d0, int rot, const float* cs,
                                            const float* sn) {
  const bf16x8 x = load_bf16x8(src + d0);
  if (d0 >= rot) return x;
  const int half = rot >> 1;
  const bool lo = d0 < half;
  const bf16x8 y = load_bf16x8(src + (lo ? d0 + half : d0 - half));
  const int c0 = lo ? d0 : d0 - half;
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float c = cs[c0 + j], s = sn[c0 + j], a = bf2f(x[j]), bb = bf2f(y[j]);
    o[j] = f2bf(lo ? a * c - bb * s : a * c + bb * s);
  }
  return o;
}

// Element offset of 16-byte chunk `ch` of key row `row` in a wave's [32 keys][D] bf16 V image;
// the XOR keeps the ds_read_b64_tr_b16 column reads of the P.V MFMA spread over banks (cdna
// guide T10 layout (b)).
template <int D>
__device__ __forceinline__ int dec_swz(int row, int ch) {
  constexpr int NCH = D / 8;
  const int f = (((row & 3) << 2) | ((row >> 2) & 3)) & (NCH - 1);
  return row * D + ((ch ^ f) << 3);
}

typedef __attribute__((address_space(3))) s16x4 dec_lds_s16x4;

// ds_read_b64_tr_b16 of 4 key rows x 16 columns, column-major per 16-lane group: lane 4q + p of
// the group addresses row r0 + q, columns c0 + 4p .. +3; lane i receives column c0 + i of the 4
// rows (row q in element q). Every lane of the wave must execute it (EXEC all ones).
template <int D>
__device__ __forceinline__ s16x4 dec_tr_read(const bf16_t* img, int r0, int c0, int lane) {
  const int i = lane & 15, q = i >> 2, pp = i & 3;
  const int ch = (c0 >> 3) + (pp >> 1), sub = (pp & 1) * 4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((dec_lds_s16x4*)(img + dec_swz<D>(r0 + q, ch) + sub));
}

// The four waves of a block work independently until one final merge.
//   * every load is issued up front, one memory round trip: the wave's 32 K rows as MFMA A
//     fragments (lane = key, 16 B of its row per k-step), its 32 V rows in the coalesced row
//     layout, and q as the B fragment (lane = query head);
//   * S^T = K q^T with v_mfma_f32_16x16x32_bf16 (no cross-lane dot-product reductions); the
//     lane holding (head g, 8 keys) runs a wave-local online softmax with 2 cross-lane steps;
//   * P^T goes to the V row layout through a wave-private LDS slice, P.V on the VALU, and the 4
//     waves' (m, l, o) are merged after the block's single barrier.
// The previous version (one block-wide softmax: 6 barriers, the V loads behind the scores):
// 17.3 -> 16.4 us per layer in a Llama-3-8B B=8 decode step. Neither the grid order (kv head
// fastest) nor a head-major cache layout changed the time (tools/decode_attn_bench.py).
// P.V on MFMA: the exponentiated scores stay in the S^T accumulator layout (lane = head g,
// keys {4kg .. 4kg+3, 16+4kg .. 16+4kg+3}), which IS the A operand of v_mfma_f32_16x16x32_bf16
// once packed to bf16 (k permuted the same way on both operands); V goes through a wave-private
// swizzled LDS image and comes back as the B operand by ds_read_b64_tr_b16 (cdna guide T10). The
// (The VALU P.V form it replaced -- P through LDS, 8 x G FMAs per key and lane -- was deleted in
// round 6; git history has it.)
template <int D, int G, bool ROPE>
__global__ __launch_bounds__(256, 3) void decode_attn_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh,     // q [B, Hq, D]
    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,              // [B, Tmax, Hkv, D]
    int64_t c_sb, int64_t c_st, int64_t c_sh, const int* __restrict__ kv_len,
    const int* __restrict__ kv_start, int window, float scale_log2, int nsplit,
    float* __restrict__ part_o,  // [B, Hq, nsplit, D]
    float* __restrict__ part_ml, // [B, Hq, nsplit, 2]
    int Hq, DecRope rp, int Tcap) {
  constexpr int LPK = D / 8, KPI = 64 / LPK, KPW = kDecChunk / 4, NIT = KPW / KPI;
  constexpr int KST = D / 32;  // MFMA k-steps over the head dim
  static_assert(G <= 16 && KPW == 32, "decode tile geometry");
  __shared__ __attribute__((aligned(16))) bf16_t vimg[4][KPW * D];
  __shared__ float acc_s[4][G][D];
  __shared__ float mls[4][G][2];
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int len = kv_len[0];
  // the row's first visible key, loaded together with kv_len ahead of the newest-token prologue
  // (one scalar round trip before the bulk K / V loads; measured neutral vs after the prologue)
  int lo = kv_start ? kv_start[b] : 0;
  const int sub = lane / LPK, dl = (lane % LPK) * 8;  // V row layout
  const int r16 = lane & 15, kg = lane >> 4;           // MFMA fragment layout
  bf16x8 vnew = {};
  int newest = -1;
  const bf16_t* qrow = nullptr;
  const float *cs = nullptr, *sn = nullptr;
  if constexpr (ROPE) {
    newest = static_cast<int>(rp.slot[0]);
    qrow = rp.qkv + (int64_t)b * rp.ld;
    const int half = rp.rot >> 1;
    cs = rp.cos_t + (int64_t)rp.pos[b] * half;
    sn = rp.sin_t + (int64_t)rp.pos[b] * half;
    vnew = load_bf16x8(qrow + (int64_t)(Hq + rp.Hkv + hk) * D + dl);
    if (split == newest / kDecChunk && wv == 0 && lane < LPK) {  // cache write for later steps
      const bf16x8 knew = dec_rope8(qrow + (int64_t)(Hq + hk) * D, dl, rp.rot, cs, sn);
      store_bf16x8(kc + (int64_t)b * c_sb + (int64_t)newest * c_st + (int64_t)hk * c_sh + dl, knew);
      store_bf16x8(vc + (int64_t)b * c_sb + (int64_t)newest * c_st + (int64_t)hk * c_sh + dl, vnew);
    }
  }
  const int base = split * kDecChunk;
  const int kw0 = base + wv * KPW;  // this wave's first key
  const bf16_t* kb0 = kc + (int64_t)b * c_sb + (int64_t)hk * c_sh;
  const bf16_t* vb0 = vc + (int64_t)b * c_sb + (int64_t)hk * c_sh + dl;
  // ---- all loads up front. K rows are clamped only into the cache capacity, so they leave at
  // kernel start without waiting for kv_len / kv_start (rows outside [k0, k1) are masked out of
  // the scores: whatever they hold is discarded); V rows are clamped into [k0, k1) (a masked
  // key's weight is 0 and its row must be finite). The newest key's rotated K / raw V (a
  // dependent chain through pos -> cos / sin) replace their registers only afterwards.
  s16x8 kf[2][KST];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int kcl = min(kw0 + 16 * t + r16, Tcap - 1);
#pragma unroll
    for (int s = 0; s < KST; ++s)
      kf[t][s] = __builtin_bit_cast(s16x8, load_bf16x8(kb0 + (int64_t)kcl * c_st + 32 * s + 8 * kg));
  }
  if (window > 0) lo = max(lo, len - window);
  const int k0 = max(base, lo), k1 = min(base + kDecChunk, len);
  const int64_t pbase = ((int64_t)b * Hq + (int64_t)hk * G) * nsplit + split;
  if (k0 >= k1) {  // empty split (beyond the current length or fully masked)
    if (tid < G) {
      part_ml[(pbase + (int64_t)tid * nsplit) * 2 + 0] = -INFINITY;
      part_ml[(pbase + (int64_t)tid * nsplit) * 2 + 1] = 0.f;
    }
    return;
  }
  bf16x8 vvr[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int key = min(max(kw0 + it * KPI + sub, k0), k1 - 1);
    vvr[it] = load_bf16x8(vb0 + (int64_t)key * c_st);
  }
  if constexpr (ROPE) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (min(kw0 + 16 * t + r16, Tcap - 1) == newest) {
#pragma unroll
        for (int s = 0; s < KST; ++s)
          kf[t][s] = __builtin_bit_cast(s16x8, dec_rope8(qrow + (int64_t)(Hq + hk) * D, 32 * s + 8 * kg, rp.rot, cs, sn));
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (min(max(kw0 + it * KPI + sub, k0), k1 - 1) == newest) vvr[it] = vnew;
  }
  s16x8 qf[KST];
#pragma unroll
  for (int s = 0; s < KST; ++s) {
    qf[s] = s16x8{};
    if (r16 < G) {
      if constexpr (ROPE)
        qf[s] = __builtin_bit_cast(s16x8, dec_rope8(qrow + (int64_t)(hk * G + r16) * D, 32 * s + 8 * kg, rp.rot, cs, sn));
      else
        qf[s] = __builtin_bit_cast(s16x8, load_bf16x8(q + (int64_t)b * q_sb + (int64_t)(hk * G + r16) * q_sh + 32 * s + 8 * kg));
    }
  }
  // ---- S^T[key][g]: lane holds keys kw0 + 16t + 4kg + i (i < 4) of head g = r16
  f32x4 sacc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    sacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KST; ++s) sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][s], qf[s], sacc[t], 0, 0, 0);
  }
  float sc[2][4];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = kw0 + 16 * t + 4 * kg + i;
      sc[t][i] = (key >= k0 && key < k1) ? sacc[t][i] * scale_log2 : -INFINITY;
      m = fmaxf(m, sc[t][i]);
    }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float muse = m == -INFINITY ? 0.f : m;
  float l = 0.f;
  // V rows -> this wave's LDS image (row = key within the wave, swizzled 16-byte chunks)
  bf16_t* vw = &vimg[wv][0];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    store_bf16x8(vw + dec_swz<D>(it * KPI + sub, dl >> 3), vvr[it]);
  float pf[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = __builtin_amdgcn_exp2f(sc[t][i] - muse);  // exp2(-inf) = 0 for masked keys
      l += p;
      pf[t][i] = r16 < G ? p : 0.f;
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  // A operand: k-slot e < 4 <-> key 4kg + e, e >= 4 <-> key 16 + 4kg + e - 4
  const float pv8[8] = {pf[0][0], pf[0][1], pf[0][2], pf[0][3], pf[1][0], pf[1][1], pf[1][2], pf[1][3]};
  const s16x8 pa = __builtin_bit_cast(s16x8, pack_bf16x8(pv8));
  // wave-private image: this wave's LDS writes complete before its transposed reads
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  f32x4 oacc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const s16x4 v0 = dec_tr_read<D>(vw, 4 * kg, 16 * dt, lane);
    const s16x4 v1 = dec_tr_read<D>(vw, 16 + 4 * kg, 16 * dt, lane);
    const s16x8 vb = s16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
  // lane (d = 16 dt + r16, heads 4kg + i) -> this wave's partial O
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4 * kg + i < G) acc_s[wv][4 * kg + i][16 * dt + r16] = oacc[dt][i];
  if (kg == 0 && r16 < G) {
    mls[wv][r16][0] = m;
    mls[wv][r16][1] = l;
  }
  __syncthreads();
  // ---- merge the 4 waves (fixed order) into this split's partial
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
        const float c = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mm);
        v += c * acc_s[w][g][d];
        ll += c * mls[w][g][1];
      }
    }
    part_o[(pbase + (int64_t)g * nsplit) * D + d] = v;
    if (d == 0) {
      part_ml[(pbase + (int64_t)g * nsplit) * 2 + 0] = mm;
      part_ml[(pbase + (int64_t)g * nsplit) * 2 + 1] = ll;
    }
  }
}

// In-kernel split combine (decode_attn_loop_kernel with `cnt`): every block publishes its
// partial (m, l, o) with write-through (sc1) stores, waits for them (vmcnt(0) in every wave), and
// one lane adds to the (b, kv head) arrival counter; the block whose add returns nsplit - 1 re-arms
// the counter, takes ONE agent-scope acquire and merges the nsplit partials into the normalised
// bf16 output -- the decode_combine_kernel launch and its kernel boundary are gone. No block waits
// on another (no polling), so a late or empty split cannot stall the grid. Hand-off form:
// MI355X_MICROARCH "Valid forms" (sc1 stores + drained vmcnt + agent atomic; consumer acquire).
__device__ __forceinline__ void dec_pub(float* p, float v, bool wt) {
  if (wt) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// Group-structured decode step (GRPO rollouts: rows p * G .. p * G + G - 1 share prompt p's keys
// [0, Tp), bitwise identical copies). The prefix part [lo, Tp) is attended once per (prompt, kv
// head) for all of the group's queries (decode_prefix_kernel, K / V of row p * G only) and lands in
// split slots [0, npre) of every (row, q head) partial; the loop kernel then runs per row over
// chunks >= c0 with Tp as its lower bound, fills slots [npre, npre + nsuf) and merges all of them.
// Everything here is a host constant of the captured graph; the lengths stay device values.
struct DecGroup {
  int G;     // rows per prompt
  int Tp;    // shared prefix length (keys)
  int npre;  // prefix split slots per (row, q head)
  int nsuf;  // suffix splits = arrivals per (row, kv head) counter
  int c0;    // first suffix chunk
};

// GRP: `nsplit` partial slots are merged, `narrive` of them (the suffix splits of this launch)
// arrive at the counter; the others were complete before the launch (decode_prefix_kernel).
template <int D, int G, bool GRP = false>
__device__ __forceinline__ void dec_arrive_combine(int* __restrict__ cnt, const float* part_o,
                                                   const float* part_ml, int64_t pbase0, int nsplit,
                                                   bf16_t* __restrict__ out, int64_t o_base,
                                                   int64_t o_sh, int narrive = 0) {
  __shared__ int last_s;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == (GRP ? narrive : nsplit) - 1;
    if (last) {
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    last_s = last;
  }
  __syncthreads();
  if (!last_s) return;
  // same merge as decode_combine_kernel (log2-domain running max, splits in ascending order),
  // every load of the (<= kDecMaxFuse) splits issued before any use: one round trip after the acquire
  constexpr int EPT = (G * D + 255) / 256;
  float mv[EPT][kDecMaxFuse], lv[EPT][kDecMaxFuse], ov[EPT][kDecMaxFuse];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = threadIdx.x + 256 * e;
    const int g = min(i, G * D - 1) / D, d = i % D;
    const float* ml = part_ml + (pbase0 + (int64_t)g * nsplit) * 2;
    const float* po = part_o + (pbase0 + (int64_t)g * nsplit) * D + d;
#pragma unroll
    for (int s = 0; s < kDecMaxFuse; ++s) {
      if (s < nsplit) {
        mv[e][s] = ml[2 * s];
        lv[e][s] = ml[2 * s + 1];
        ov[e][s] = po[(int64_t)s * D];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = threadIdx.x + 256 * e;
    if (i >= G * D) break;
    const int g = i / D, d = i % D;
    float m = -INFINITY;
#pragma unroll
    for (int s = 0; s < kDecMaxFuse; ++s)
      if (s < nsplit) m = fmaxf(m, mv[e][s]);
    float acc = 0.f, l = 0.f;
    if (m != -INFINITY) {
#pragma unroll
      for (int s = 0; s < kDecMaxFuse; ++s) {
        if (s < nsplit) {
          const float c = mv[e][s] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mv[e][s] - m);
          l += c * lv[e][s];
          acc += c == 0.f ? 0.f : c * ov[e][s];  // an empty split never wrote its o row
        }
      }
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
    out[o_base + (int64_t)g * o_sh + d] = f2bf(acc * inv);
  }
}

// Multi-chunk form (the default): grid (nsplit, Hkv, B) with each block looping over `cpb`
// consecutive 128-key chunks of its (b, kv head), chunk c + 2's K / V loads in flight while chunk
// c is computed (a 2-slot register ring), and a per-wave online softmax across the chunks. The
// host picks cpb so the grid fits in ~one round of resident blocks: at B = 64 (the reference's
// RLHF rollout batch) the one-chunk-per-block grid ran 2560 blocks in ~3.3 rounds, each block
// paying its own dependent round trips (scalars -> K/V -> merge); here 512 blocks stream ~4.5
// chunks each and the per-block prologue / merge is paid once. Numerics: the same masked
// exp2-domain softmax and P.V MFMA as decode_attn_kernel, with the running max rescale
// applied between chunks; partials (m, l, o) per split as before.
__device__ __forceinline__ void dec_glds16(const void* src, void* lds_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
}

// The loop kernel's body: a block streams chunks [cbeg, cend) of one (split, kv head, sequence)
// through a 2-deep K / V ring.
template <int D, int G, bool ROPE, bool GRP = false>
__device__ __forceinline__ void dec_loop_body(
    const int split, const int hk, const int b, const int Hkv_grid,
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh,
    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    int64_t c_sb, int64_t c_st, int64_t c_sh, const int* __restrict__ kv_len,
    const int* __restrict__ kv_start, int window, float scale_log2, int nsplit, int cpb,
    float* __restrict__ part_o, float* __restrict__ part_ml, int Hq, const DecRope& rp,
    bf16_t* __restrict__ out, int64_t o_sb, int64_t o_sh, int* __restrict__ cnt, int Tcap,
    const DecGroup& gp = DecGroup{}) {
  // GRP (the suffix part of a group-structured step, see DecGroup): `split` counts from chunk
  // gp.c0, keys below gp.Tp are masked, the partials go to slots gp.npre + split of `nsplit`, and
  // the host always asks for partials (+ the in-kernel combine when `cnt` is given).
  // out != nullptr, cnt == nullptr (one split per sequence): the block writes the normalised bf16
  // output itself; out and cnt (nsplit > 1): partials + in-kernel combine (dec_arrive_combine).
  // Either way the combine launch is skipped.
  constexpr int LPK = D / 8, KPI = 64 / LPK, KPW = kDecChunk / 4, NIT = KPW / KPI;
  constexpr int KST = D / 32;
  static_assert(G <= 16 && KPW == 32, "decode tile geometry");
  static_assert(G * D * 4 <= KPW * D * 2, "acc_s aliases one V image slot");
  // per wave: 2 V image slots (LDS-DMA ring), the first re-used for the wave's partial O
  constexpr int RD = 2;
  __shared__ __attribute__((aligned(16))) bf16_t vimg[4][RD][KPW * D];
  __shared__ float mls[4][G][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int len = kv_len[0];
  int lo = kv_start ? kv_start[b] : 0;
  const int sub = lane / LPK, dl = (lane % LPK) * 8;
  const int r16 = lane & 15, kg = lane >> 4;
  int newest = -1;
  // this block's q heads, k and v of the newest token: a row of the qkv projection
  const bf16_t *qh = nullptr, *kh = nullptr, *vh = nullptr;
  const float *cs = nullptr, *sn = nullptr;
  const int cfirst = (GRP ? gp.c0 : 0) + split * cpb;
  auto cache_write = [&]() {  // the newest key's rotated K / raw V into its cache slot
    if constexpr (ROPE) {
      const int cn = newest / kDecChunk;
      if (cn >= cfirst && cn < cfirst + cpb && wv == 0 && lane < LPK) {
        const bf16x8 vnew = load_bf16x8(vh + dl);
        const bf16x8 knew = dec_rope8(kh, dl, rp.rot, cs, sn);
        store_bf16x8(kc + (int64_t)b * c_sb + (int64_t)newest * c_st + (int64_t)hk * c_sh + dl, knew);
        store_bf16x8(vc + (int64_t)b * c_sb + (int64_t)newest * c_st + (int64_t)hk * c_sh + dl, vnew);
      }
    }
  };
  if constexpr (ROPE) {
    newest = static_cast<int>(rp.slot[0]);
    const bf16_t* qrow = rp.qkv + (int64_t)b * rp.ld;
    qh = qrow + (int64_t)(hk * G) * D;
    kh = qrow + (int64_t)(Hq + hk) * D;
    vh = qrow + (int64_t)(Hq + rp.Hkv + hk) * D;
    const int half = rp.rot >> 1;
    cs = rp.cos_t + (int64_t)rp.pos[b] * half;
    sn = rp.sin_t + (int64_t)rp.pos[b] * half;
    cache_write();
  }
  const bf16_t* kb0 = kc + (int64_t)b * c_sb + (int64_t)hk * c_sh;
  const bf16_t* vb0 = vc + (int64_t)b * c_sb + (int64_t)hk * c_sh;
  // 2-slot ring: K as MFMA A fragments in registers, V by LDS-DMA straight into the wave's
  // swizzled image (lane-linear destination, the swizzle applied on the per-lane SOURCE chunk:
  // image row it * KPI + sub, position dl / 8 holds logical chunk (dl / 8) ^ f(row)). K rows are
  // clamped only into the chunk and the cache capacity (no kv_len / kv_start dependence: the
  // first chunk's K loads leave at kernel start, beside the scalar length loads; rows outside
  // the visible range are masked out of the scores, so whatever they hold is discarded); V rows
  // are clamped into the visible range (a masked key's weight is 0 and its V row must be finite).
  s16x8 kf[RD][2][KST];
  auto loadK = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int kw0 = c * kDecChunk + wv * KPW;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kcl = min(kw0 + 16 * t + r16, Tcap - 1);
#pragma unroll
      for (int s = 0; s < KST; ++s)
        kf[j][t][s] = __builtin_bit_cast(s16x8, load_bf16x8(kb0 + (int64_t)kcl * c_st + 32 * s + 8 * kg));
    }
  };
  loadK(std::integral_constant<int, 0>{}, cfirst);  // speculative: the split's first chunk
  if (window > 0) lo = max(lo, len - window);
  if constexpr (GRP) lo = max(lo, gp.Tp);
  // chunks [cbeg, cend) of this split that hold visible keys
  const int cbeg = max(cfirst, lo / kDecChunk);
  const int cend = min(cfirst + cpb, (len + kDecChunk - 1) / kDecChunk);
  const int64_t pbase = ((int64_t)b * Hq + (int64_t)hk * G) * nsplit + (GRP ? gp.npre : 0) + split;
  const bool fuse = cnt != nullptr;
  int* const cslot = fuse ? cnt + (int64_t)b * Hkv_grid + hk : nullptr;
  const int64_t pbase0 = ((int64_t)b * Hq + (int64_t)hk * G) * nsplit;
  const int64_t obase = (int64_t)b * o_sb + (int64_t)hk * G * o_sh;
  if (cbeg >= cend || max(cbeg * kDecChunk, lo) >= len) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the speculative K loads
    if (out != nullptr && !fuse) {  // no visible key: zeros, as the combine writes for an all-empty row
      for (int i = tid; i < G * D; i += 256)
        out[(int64_t)b * o_sb + (int64_t)(hk * G + i / D) * o_sh + i % D] = 0;
      return;
    }
    if (tid < G) {
      dec_pub(&part_ml[(pbase + (int64_t)tid * nsplit) * 2 + 0], -INFINITY, fuse);
      dec_pub(&part_ml[(pbase + (int64_t)tid * nsplit) * 2 + 1], 0.f, fuse);
    }
    if (fuse) dec_arrive_combine<D, G, GRP>(cslot, part_o, part_ml, pbase0, nsplit, out, obase, o_sh, gp.nsuf);
    return;
  }
  // q fragments first, the oldest loads: S of chunk 0 waits for them and K(0) only
  s16x8 qf[KST];
#pragma unroll
  for (int s = 0; s < KST; ++s) {
    qf[s] = s16x8{};
    if (r16 < G) {
      if constexpr (ROPE)
        qf[s] = __builtin_bit_cast(s16x8, dec_rope8(qh + (int64_t)r16 * D, 32 * s + 8 * kg, rp.rot, cs, sn));
      else
        qf[s] = __builtin_bit_cast(s16x8, load_bf16x8(q + (int64_t)b * q_sb + (int64_t)(hk * G + r16) * q_sh + 32 * s + 8 * kg));
    }
  }
  auto loadV = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int base = c * kDecChunk, k0 = max(base, lo), k1 = min(base + kDecChunk, len);
    const int kw0 = base + wv * KPW;
    bf16_t* img = &vimg[wv][j][0];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * KPI + sub;
      const int key = min(max(kw0 + row, k0), k1 - 1);
      const int ch = (dec_swz<D>(row, dl >> 3) - row * D) >> 3;  // position dl/8 <-> chunk ch
      dec_glds16(vb0 + (int64_t)key * c_st + ch * 8, img + it * 512);
    }
  };
  auto load = [&](auto J, int c) {  // issue order per chunk: K then V
    loadK(J, c);
    loadV(J, c);
  };
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 oacc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int base = c * kDecChunk, k0 = max(base, lo), k1 = min(base + kDecChunk, len);
    const int kw0 = base + wv * KPW;
    const bool newest_here = ROPE && newest >= kw0 && newest < kw0 + KPW;
    if constexpr (ROPE) {  // the newest key's K comes from registers (its cache row is being written)
      if (newest_here) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (min(kw0 + 16 * t + r16, Tcap - 1) == newest) {
#pragma unroll
            for (int s = 0; s < KST; ++s)
              kf[j][t][s] = __builtin_bit_cast(s16x8, dec_rope8(kh, 32 * s + 8 * kg, rp.rot, cs, sn));
          }
        }
      }
    }
    f32x4 sacc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KST; ++s) sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[j][t][s], qf[s], sacc[t], 0, 0, 0);
    }
    float sc[2][4];
    float mc = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kw0 + 16 * t + 4 * kg + i;
        sc[t][i] = (key >= k0 && key < k1) ? sacc[t][i] * scale_log2 : -INFINITY;
        mc = fmaxf(mc, sc[t][i]);
      }
    mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    const float mnew = fmaxf(m_run, mc);
    const float alpha = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - mnew);
    const float muse = mnew == -INFINITY ? 0.f : mnew;
    float pf[2][4], ls = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(sc[t][i] - muse);
        ls += p;
        pf[t][i] = r16 < G ? p : 0.f;
      }
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    l_run = l_run * alpha + ls;
    m_run = mnew;
    const float pv8[8] = {pf[0][0], pf[0][1], pf[0][2], pf[0][3], pf[1][0], pf[1][1], pf[1][2], pf[1][3]};
    const s16x8 pa = __builtin_bit_cast(s16x8, pack_bf16x8(pv8));
    float ai[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ai[i] = __shfl(alpha, 4 * kg + i, 64);
    // V(c) has landed once every VMEM op but the next chunk's (2 KST K loads + NIT V pieces,
    // issued after it) is done; the compiler does not see the DMA -> LDS dependence
    // (chunks issued after c: min(RD - 1, cend - 1 - c); the refill of c + RD comes after this)
    constexpr int PER = 2 * KST + NIT;
    const int nlater = min(RD - 1, cend - 1 - c);
    if (nlater == 1) {
      if constexpr (PER == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else if constexpr (PER == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bf16_t* vw = &vimg[wv][j][0];
    if constexpr (ROPE) {
      // Every image row whose clamped key is the newest one -- its own row, and the rows past
      // the visible range that loadV clamped onto it (a wave beyond kv_len has only those) --
      // takes the V row from the qkv row: the cache slot is written by this launch, so the DMA
      // read stale or never-written bytes there, and a NaN in a masked row still poisons P.V.
      if (newest >= k0 && newest < k1) {
        const bf16x8 vn = load_bf16x8(vh + dl);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int row = it * KPI + sub;
          if (min(max(kw0 + row, k0), k1 - 1) == newest) store_bf16x8(vw + dec_swz<D>(row, dl >> 3), vn);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      const s16x4 v0 = dec_tr_read<D>(vw, 4 * kg, 16 * dt, lane);
      const s16x4 v1 = dec_tr_read<D>(vw, 16 + 4 * kg, 16 * dt, lane);
      const s16x8 vb = s16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      f32x4 o = oacc[dt];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] *= ai[i];
      oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, o, 0, 0, 0);
    }
    if (c + RD < cend) {
      // WAR: this slot's transposed reads are complete before the DMA refill is issued
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      load(J, c + RD);
    }
  };
  if (cbeg != cfirst) loadK(std::integral_constant<int, 0>{}, cbeg);  // left padding: the guess was wrong
  loadV(std::integral_constant<int, 0>{}, cbeg);
  if (cbeg + 1 < cend) load(std::integral_constant<int, 1>{}, cbeg + 1);
  for (int c = cbeg; c < cend; c += RD) {
    step(std::integral_constant<int, 0>{}, c);
    if (c + 1 < cend) step(std::integral_constant<int, 1>{}, c + 1);
  }
  // this wave's partial O into its own (dead) first image slot
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float* acc_w = reinterpret_cast<float*>(&vimg[wv][0][0]);
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
        v += cc * reinterpret_cast<const float*>(&vimg[w][0][0])[g * D + d];
        ll += cc * mls[w][g][1];
      }
    }
    if (out != nullptr && !fuse) {
      out[(int64_t)b * o_sb + (int64_t)(hk * G + g) * o_sh + d] = f2bf(ll > 0.f ? v * (1.f / ll) : 0.f);
      continue;
    }
    dec_pub(&part_o[(pbase + (int64_t)g * nsplit) * D + d], v, fuse);
    if (d == 0) {
      dec_pub(&part_ml[(pbase + (int64_t)g * nsplit) * 2 + 0], mm, fuse);
      dec_pub(&part_ml[(pbase + (int64_t)g * nsplit) * 2 + 1], ll, fuse);
    }
  }
  if (fuse) dec_arrive_combine<D, G, GRP>(cslot, part_o, part_ml, pbase0, nsplit, out, obase, o_sh, gp.nsuf);
}

template <int D, int G, bool ROPE>
__global__ __launch_bounds__(256, 2) void decode_attn_loop_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh,
    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    int64_t c_sb, int64_t c_st, int64_t c_sh, const int* __restrict__ kv_len,
    const int* __restrict__ kv_start, int window, float scale_log2, int nsplit, int cpb,
    float* __restrict__ part_o, float* __restrict__ part_ml, int Hq, DecRope rp,
    bf16_t* __restrict__ out, int64_t o_sb, int64_t o_sh, int* __restrict__ cnt, int Tcap) {
  dec_loop_body<D, G, ROPE>(blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, q, q_sb, q_sh, kc, vc, c_sb, c_st,
                            c_sh, kv_len, kv_start, window, scale_log2, nsplit, cpb, part_o, part_ml, Hq, rp,
                            out, o_sb, o_sh, cnt, Tcap);
}

// The suffix part of a group-structured step: the loop kernel with GRP set (see dec_loop_body).
template <int D, int G, bool ROPE>
__global__ __launch_bounds__(256, 2) void decode_attn_loop_group_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh,
    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    int64_t c_sb, int64_t c_st, int64_t c_sh, const int* __restrict__ kv_len,
    const int* __restrict__ kv_start, int window, float scale_log2, int nsplit, int cpb,
    float* __restrict__ part_o, float* __restrict__ part_ml, int Hq, DecRope rp,
    bf16_t* __restrict__ out, int64_t o_sb, int64_t o_sh, int* __restrict__ cnt, int Tcap, DecGroup gp) {
  dec_loop_body<D, G, ROPE, true>(blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, q, q_sb, q_sh, kc, vc, c_sb,
                                  c_st, c_sh, kv_len, kv_start, window, scale_log2, nsplit, cpb, part_o,
                                  part_ml, Hq, rp, out, o_sb, o_sh, cnt, Tcap, gp);
}

// The prefix part of a group-structured step (see DecGroup): grid (npre, Hkv, P * ntile). A block
// streams chunks [split * cpb, +cpb) of keys [lo, min(Tp, kv_len)) of ONE cache row, p * G, with the
// loop kernel's machinery (K rows as MFMA A fragments in a 2-slot register ring, V by LDS-DMA into
// the wave's swizzled image, read back transposed, exp2-domain online softmax per wave), but against
// NT 16-column query tiles at once: column c of row tile `tg` is q head hk * GQ + c % GQ of group
// row tg * rpt + c / GQ. Every K fragment and every V image read feeds NT MFMAs; each tile keeps
// its own (m, l, o). Columns past rpt * GQ or rows past G are padding: zero queries, never stored.
// The 4 waves merge in a fixed tree ((0 + 1) + (2 + 3)) through the dead V images, lane for lane
// in the accumulator layout, and the block stores the fp32 partial of slot `split` for each of
// its (row, q head) columns. An empty range stores m = -inf, l = 0 and no o row.
template <int D, int NT, bool ROPE>
__global__ __launch_bounds__(256, NT > 2 ? 1 : 2) void decode_prefix_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh,
    const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    int64_t c_sb, int64_t c_st, int64_t c_sh, const int* __restrict__ kv_len,
    const int* __restrict__ kv_start, int window, float scale_log2, int ntot, int cpb,
    float* __restrict__ part_o, float* __restrict__ part_ml, int Hq, int GQ, DecRope rp,
    DecGroup gp, int rpt, int ntile, int Tcap) {
  constexpr int LPK = D / 8, KPI = 64 / LPK, KPW = kDecChunk / 4, NIT = KPW / KPI;
  constexpr int KST = D / 32, NDT = D / 16, RD = 2;
  constexpr int WSZ = NT * 16 * D;  // floats of one wave's partial O
  static_assert(NT >= 1 && NT <= 4 && KPW == 32, "prefix tile geometry");
  static_assert(2 * WSZ * 4 <= 4 * RD * KPW * D * 2, "two waves' partial O alias the V images");
  __shared__ __attribute__((aligned(16))) bf16_t vimg[4][RD][KPW * D];
  __shared__ float mls[2][NT][2][64];
  __shared__ float mlf[NT * 16][2];
  const int split = blockIdx.x, hk = blockIdx.y;
  const int p = blockIdx.z / ntile, tg = blockIdx.z % ntile;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sub = lane / LPK, dl = (lane % LPK) * 8;
  const int r16 = lane & 15, kg = lane >> 4;
  const int b0 = p * gp.G;  // the row whose prefix K / V the whole group reads
  const int len = kv_len[0];
  int lo = kv_start ? kv_start[b0] : 0;
  const bf16_t* kb0 = kc + (int64_t)b0 * c_sb + (int64_t)hk * c_sh;
  const bf16_t* vb0 = vc + (int64_t)b0 * c_sb + (int64_t)hk * c_sh;
  const int cfirst = split * cpb;
  s16x8 kf[RD][2][KST];
  auto loadK = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int kw0 = c * kDecChunk + wv * KPW;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kcl = min(kw0 + 16 * t + r16, Tcap - 1);
#pragma unroll
      for (int s = 0; s < KST; ++s)
        kf[j][t][s] = __builtin_bit_cast(s16x8, load_bf16x8(kb0 + (int64_t)kcl * c_st + 32 * s + 8 * kg));
    }
  };
  loadK(std::integral_constant<int, 0>{}, cfirst);  // speculative, as in dec_loop_body
  if (window > 0) lo = max(lo, len - window);
  const int hi = min(gp.Tp, len);
  const int cbeg = max(cfirst, lo / kDecChunk);
  const int cend = min(cfirst + cpb, (hi + kDecChunk - 1) / kDecChunk);
  // column c = 16 n + r16 of this row tile (S layout: the lane's own column of tile n)
  const int ncol = rpt * GQ;
  auto col_row = [&](int c) { return tg * rpt + c / GQ; };
  auto col_ok = [&](int c) { return c < ncol && col_row(c) < gp.G; };
  auto col_pbase = [&](int c) {  // partial slot `split` of the column's (row, q head)
    return ((int64_t)(b0 + col_row(c)) * Hq + (int64_t)hk * GQ + c % GQ) * ntot + split;
  };
  if (cbeg >= cend || max(cbeg * kDecChunk, lo) >= hi) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the speculative K loads
    if (tid < NT * 16 && col_ok(tid)) {
      part_ml[col_pbase(tid) * 2 + 0] = -INFINITY;
      part_ml[col_pbase(tid) * 2 + 1] = 0.f;
    }
    return;
  }
  s16x8 qf[NT][KST];
  bool cok[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int c = 16 * n + r16;
    cok[n] = col_ok(c);
    const int b = b0 + col_row(c), h = hk * GQ + c % GQ;
#pragma unroll
    for (int s = 0; s < KST; ++s) {
      qf[n][s] = s16x8{};
      if (cok[n]) {
        if constexpr (ROPE) {
          const int half = rp.rot >> 1;
          const float* cs = rp.cos_t + (int64_t)rp.pos[b] * half;
          const float* sn = rp.sin_t + (int64_t)rp.pos[b] * half;
          qf[n][s] = __builtin_bit_cast(s16x8, dec_rope8(rp.qkv + (int64_t)b * rp.ld + (int64_t)h * D, 32 * s + 8 * kg, rp.rot, cs, sn));
        } else {
          qf[n][s] = __builtin_bit_cast(s16x8, load_bf16x8(q + (int64_t)b * q_sb + (int64_t)h * q_sh + 32 * s + 8 * kg));
        }
      }
    }
  }
  auto loadV = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int base = c * kDecChunk, k0 = max(base, lo), k1 = min(base + kDecChunk, hi);
    const int kw0 = base + wv * KPW;
    bf16_t* img = &vimg[wv][j][0];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * KPI + sub;
      const int key = min(max(kw0 + row, k0), k1 - 1);
      const int ch = (dec_swz<D>(row, dl >> 3) - row * D) >> 3;  // position dl/8 <-> chunk ch
      dec_glds16(vb0 + (int64_t)key * c_st + ch * 8, img + it * 512);
    }
  };
  auto load = [&](auto J, int c) {  // issue order per chunk: K then V
    loadK(J, c);
    loadV(J, c);
  };
  float m_run[NT], l_run[NT];
  f32x4 oacc[NT][NDT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    m_run[n] = -INFINITY;
    l_run[n] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) oacc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto step = [&](auto J, int c) {
    constexpr int j = decltype(J)::value;
    const int base = c * kDecChunk, k0 = max(base, lo), k1 = min(base + kDecChunk, hi);
    const int kw0 = base + wv * KPW;
    s16x8 pa[NT];
    float ai[NT][4];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      f32x4 sacc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KST; ++s) sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[j][t][s], qf[n][s], sacc[t], 0, 0, 0);
      }
      float sc[2][4];
      float mc = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = kw0 + 16 * t + 4 * kg + i;
          sc[t][i] = (key >= k0 && key < k1) ? sacc[t][i] * scale_log2 : -INFINITY;
          mc = fmaxf(mc, sc[t][i]);
        }
      mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
      mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
      const float mnew = fmaxf(m_run[n], mc);
      const float alpha = m_run[n] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run[n] - mnew);
      const float muse = mnew == -INFINITY ? 0.f : mnew;
      float pv8[8], ls = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pe = __builtin_amdgcn_exp2f(sc[t][i] - muse);
          ls += pe;
          pv8[4 * t + i] = cok[n] ? pe : 0.f;
        }
      ls += __shfl_xor(ls, 16, 64);
      ls += __shfl_xor(ls, 32, 64);
      l_run[n] = l_run[n] * alpha + ls;
      m_run[n] = mnew;
      pa[n] = __builtin_bit_cast(s16x8, pack_bf16x8(pv8));
#pragma unroll
      for (int i = 0; i < 4; ++i) ai[n][i] = __shfl(alpha, 4 * kg + i, 64);
    }
    // V(c) has landed once every VMEM op but the next chunk's is done (see dec_loop_body)
    constexpr int PER = 2 * KST + NIT;
    const int nlater = min(RD - 1, cend - 1 - c);
    if (nlater == 1) {
      if constexpr (PER == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else if constexpr (PER == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bf16_t* vw = &vimg[wv][j][0];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const s16x4 v0 = dec_tr_read<D>(vw, 4 * kg, 16 * dt, lane);
      const s16x4 v1 = dec_tr_read<D>(vw, 16 + 4 * kg, 16 * dt, lane);
      const s16x8 vb = s16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        f32x4 o = oacc[n][dt];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] *= ai[n][i];
        oacc[n][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[n], vb, o, 0, 0, 0);
      }
    }
    if (c + RD < cend) {
      // WAR: this slot's transposed reads are complete before the DMA refill is issued
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      load(J, c + RD);
    }
  };
  if (cbeg != cfirst) loadK(std::integral_constant<int, 0>{}, cbeg);  // the guess was wrong
  loadV(std::integral_constant<int, 0>{}, cbeg);
  if (cbeg + 1 < cend) load(std::integral_constant<int, 1>{}, cbeg + 1);
  for (int c = cbeg; c < cend; c += RD) {
    step(std::integral_constant<int, 0>{}, c);
    if (c + 1 < cend) step(std::integral_constant<int, 1>{}, c + 1);
  }
  // ---- merge the 4 waves: 1 -> 0 and 3 -> 2, then 2 -> 0, through the (dead) V images
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  float* mb = reinterpret_cast<float*>(&vimg[0][0][0]);
  auto put = [&](int slot) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      mls[slot][n][0][lane] = m_run[n];
      mls[slot][n][1][lane] = l_run[n];
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) mb[slot * WSZ + ((n * NDT + dt) * 4 + i) * 64 + lane] = oacc[n][dt][i];
    }
  };
  auto take = [&](int slot) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float m2 = mls[slot][n][0][lane], l2 = mls[slot][n][1][lane];
      const float mm = fmaxf(m_run[n], m2);
      const float c1 = m_run[n] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run[n] - mm);
      const float c2 = m2 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m2 - mm);
      l_run[n] = c1 * l_run[n] + c2 * l2;
      m_run[n] = mm;
      float a1[4], a2[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a1[i] = __shfl(c1, 4 * kg + i, 64);
        a2[i] = __shfl(c2, 4 * kg + i, 64);
      }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          oacc[n][dt][i] = a1[i] * oacc[n][dt][i] + a2[i] * mb[slot * WSZ + ((n * NDT + dt) * 4 + i) * 64 + lane];
    }
  };
  if (wv & 1) put(wv >> 1);
  __syncthreads();
  if (!(wv & 1)) take(wv >> 1);
  __syncthreads();
  if (wv == 2) put(0);
  __syncthreads();
  if (wv == 0) {
    take(0);
    // the block's partial as [column][d] in slot 1 (slot 0 is being read by this wave)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) mb[WSZ + (16 * n + 4 * kg + i) * D + 16 * dt + r16] = oacc[n][dt][i];
      if (kg == 0) {
        mlf[16 * n + r16][0] = m_run[n];
        mlf[16 * n + r16][1] = l_run[n];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < NT * 16 * D; i += 256) {
    const int c = i / D, d = i % D;
    if (!col_ok(c)) continue;
    const int64_t pb = col_pbase(c);
    part_o[pb * D + d] = mb[WSZ + i];
    if (d == 0) {
      part_ml[pb * 2 + 0] = mlf[c][0];
      part_ml[pb * 2 + 1] = mlf[c][1];
    }
  }
}

// Decode-step prologue: rotate q (-> q_out [B, Hq, D]) and k of the newest token and write k and
// v straight into the cache slot `*slot` (device value), replacing rope + two index_copy
// launches. qkv [B, (Hq + 2 Hkv) * D] rows; same rotate-half math as rope.hip.
__global__ __launch_bounds__(256) void rope_cache_kernel(
    const bf16_t* __restrict__ qkv, int64_t ld, bf16_t* __restrict__ q_out,
    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, int64_t c_sb, int64_t c_st, int64_t c_sh,
    const int64_t* __restrict__ slot, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, const int* __restrict__ pos, int B, int Hq, int Hkv, int D,
    int rot) {
  const int dv = D >> 3, heads = Hq + 2 * Hkv, half = rot >> 1, hv = half >> 3;
  const int64_t total = (int64_t)B * heads * dv;
  const int64_t t_slot = slot[0];
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int v = (int)(i % dv);
    const int h = (int)((i / dv) % heads);
    const int b = (int)(i / ((int64_t)dv * heads));
    const bf16_t* s = qkv + (int64_t)b * ld + (int64_t)h * D;
    bf16_t* d;
    if (h < Hq) d = q_out + ((int64_t)b * Hq + h) * D;
    else if (h < Hq + Hkv) d = kc + (int64_t)b * c_sb + t_slot * c_st + (int64_t)(h - Hq) * c_sh;
    else d = vc + (int64_t)b * c_sb + t_slot * c_st + (int64_t)(h - Hq - Hkv) * c_sh;
    if (h < Hq + Hkv && v < hv) {
      const int p = pos[b];
      const float* cp = cos_t + (int64_t)p * half + v * 8;
      const float* sp = sin_t + (int64_t)p * half + v * 8;
      bf16x8 lo = load_bf16x8(s + v * 8), hi = load_bf16x8(s + half + v * 8), olo, ohi;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = cp[j], sn = sp[j], a = bf2f(lo[j]), bb = bf2f(hi[j]);
        olo[j] = f2bf(a * c - bb * sn);
        ohi[j] = f2bf(bb * c + a * sn);
      }
      store_bf16x8(d + v * 8, olo);
      store_bf16x8(d + half + v * 8, ohi);
    } else if (h >= Hq + Hkv || v >= 2 * hv) {
      store_bf16x8(d + v * 8, load_bf16x8(s + v * 8));
    }
  }
}

void launch_rope_cache(const bf16_t* qkv, int64_t ld, bf16_t* q_out, bf16_t* kc, bf16_t* vc,
                       int64_t c_sb, int64_t c_st, int64_t c_sh, const int64_t* slot,
                       const float* cos_t, const float* sin_t, const int* pos, int B, int Hq,
                       int Hkv, int D, int rot, hipStream_t st) {
  const int64_t work = (int64_t)B * (Hq + 2 * Hkv) * (D / 8);
  const int grid = (int)std::min<int64_t>((work + 255) / 256, 1024);
  rope_cache_kernel<<<grid, 256, 0, st>>>(qkv, ld, q_out, kc, vc, c_sb, c_st, c_sh, slot, cos_t,
                                          sin_t, pos, B, Hq, Hkv, D, rot);
}

// one 64-thread block per (b, h): merge the splits (log2-domain running max). The split
// statistics are read in parallel (one split per lane, 64 at a time) and the per-split weights
// go through LDS, so the output pass issues its part_o loads 8 splits at a time instead of one
// dependent load chain per split (which made this launch grow by ~0.5 us per split).
template <int D>
__global__ __launch_bounds__(64) void decode_combine_kernel(const float* __restrict__ part_o,
                                                             const float* __restrict__ part_ml,
                                                             int nsplit, bf16_t* __restrict__ out,
                                                             int64_t o_sb, int64_t o_sh, int Hq) {
  __shared__ float wsp[64];
  const int bh = blockIdx.x, lane = threadIdx.x;
  const int b = bh / Hq, h = bh % Hq;
  const float* ml = part_ml + (int64_t)bh * nsplit * 2;
  const float* po = part_o + (int64_t)bh * nsplit * D;
  float m = -INFINITY;
  for (int s = lane; s < nsplit; s += 64) m = fmaxf(m, ml[2 * s]);
  m = wave_max(m);
  constexpr int DPT = D / 64;
  float acc[DPT] = {};
  float l = 0.f;
  if (m != -INFINITY) {
    for (int s0 = 0; s0 < nsplit; s0 += 64) {
      const int s = s0 + lane;
      float c = 0.f;
      if (s < nsplit) {
        const float ms = ml[2 * s];
        c = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - m);
        l += c * ml[2 * s + 1];
      }
      wsp[lane] = c;
      __syncthreads();
      const int n = min(64, nsplit - s0);
      int j = 0;
      for (; j + 8 <= n; j += 8) {
        float v[8][DPT];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int t = 0; t < DPT; ++t) v[u][t] = po[(int64_t)(s0 + j + u) * D + lane * DPT + t];
        // an empty split never wrote its part_o row (uninitialised memory): weight 0 selects 0
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float w = wsp[j + u];
#pragma unroll
          for (int t = 0; t < DPT; ++t) acc[t] += w == 0.f ? 0.f : w * v[u][t];
        }
      }
      for (; j < n; ++j) {
        const float w = wsp[j];
#pragma unroll
        for (int t = 0; t < DPT; ++t)
          acc[t] += w == 0.f ? 0.f : w * po[(int64_t)(s0 + j) * D + lane * DPT + t];
      }
      __syncthreads();
    }
    l = wave_sum(l);
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
  for (int j = 0; j < DPT; ++j)
    out[(int64_t)b * o_sb + (int64_t)h * o_sh + lane * DPT + j] = f2bf(acc[j] * inv);
}

// ---- host side: one launch path for the four forms (per-row / group-structured step, rotated q /
// fused rope + cache write); split geometry in decode_geom.h
template <int N>
using dec_int = std::integral_constant<int, N>;

// f(D, GQ, ROPE) with the launch's head dim, q heads per kv head and form as integral constants
// (head dim and GQA ratio validated on the host)
template <class F>
static void decode_dispatch(const DecodeParams& p, F f) {
  auto form = [&](auto d, auto gq) {
    if (p.rope.qkv != nullptr) f(d, gq, std::true_type{});
    else f(d, gq, std::false_type{});
  };
  auto heads = [&](auto d) {
    switch (p.Hq / p.Hkv) {
      case 1: form(d, dec_int<1>{}); break;
      case 2: form(d, dec_int<2>{}); break;
      case 4: form(d, dec_int<4>{}); break;
      case 8: form(d, dec_int<8>{}); break;
      default: break;
    }
  };
  if (p.D == 128) heads(dec_int<128>{});
  else heads(dec_int<64>{});
}

template <int D>
static void launch_decode_combine(const DecodeParams& p, int nsplit, hipStream_t st) {
  decode_combine_kernel<D><<<p.B * p.Hq, 64, 0, st>>>(p.part_o, p.part_ml, nsplit, p.out, p.o_sb, p.o_sh, p.Hq);
}

template <int D, int GQ, bool ROPE>
static void launch_decode_rows(const DecodeParams& p, hipStream_t st) {
  const int cpb = decode_cpb(p.Tmax, p.B, p.Hkv);
  const int nsplit = decode_num_splits(p.Tmax, p.B, p.Hkv);
  dim3 grid(nsplit, p.Hkv, p.B);
  if (cpb > 0) {
    // one split per sequence, or the in-kernel combine (arrival counters given): no combine launch
    int* const cn = (nsplit > 1 && nsplit <= kDecMaxFuse) ? p.cnt : nullptr;
    bf16_t* fin = (nsplit == 1 || cn != nullptr) ? p.out : nullptr;
    decode_attn_loop_kernel<D, GQ, ROPE><<<grid, 256, 0, st>>>(
        p.q, p.q_sb, p.q_sh, p.kc, p.vc, p.c_sb, p.c_st, p.c_sh, p.kv_len, p.kv_start, p.window,
        p.scale_log2, nsplit, cpb, p.part_o, p.part_ml, p.Hq, p.rope, fin, p.o_sb, p.o_sh, cn, p.Tmax);
    if (fin == nullptr) launch_decode_combine<D>(p, nsplit, st);
    return;
  }
  decode_attn_kernel<D, GQ, ROPE><<<grid, 256, 0, st>>>(
      p.q, p.q_sb, p.q_sh, p.kc, p.vc, p.c_sb, p.c_st, p.c_sh, p.kv_len, p.kv_start, p.window,
      p.scale_log2, nsplit, p.part_o, p.part_ml, p.Hq, p.rope, p.Tmax);
  launch_decode_combine<D>(p, nsplit, st);
}

// Group-structured decode step (DecGroup); ROPE: rope + cache write of the newest token in the
// suffix launch
template <int D, int GQ, bool ROPE>
static void launch_decode_group(const DecodeParams& p, hipStream_t st) {
  const int P = p.B / p.G;
  const DecGroupGeom g = decode_group_geom(p.Tmax, p.B, p.Hq, p.Hkv, p.G, p.Tp);
  const DecGroup gp{p.G, p.Tp, g.npre, g.nsuf, g.c0};
  const int ntot = g.npre + g.nsuf;
  // prefix launch first: its partials are complete at the kernel boundary, ahead of the suffix
  // launch's merge (same stream)
  dim3 pgrid(g.npre, p.Hkv, P * g.ntile);
  auto prefix = [&](auto nt) {
    decode_prefix_kernel<D, decltype(nt)::value, ROPE><<<pgrid, 256, 0, st>>>(
        p.q, p.q_sb, p.q_sh, p.kc, p.vc, p.c_sb, p.c_st, p.c_sh, p.kv_len, p.kv_start, p.window,
        p.scale_log2, ntot, g.cpb_p, p.part_o, p.part_ml, p.Hq, GQ, p.rope, gp, g.rpt, g.ntile, p.Tmax);
  };
  switch (g.nt) {
    case 1: prefix(dec_int<1>{}); break;
    case 2: prefix(dec_int<2>{}); break;
    default: prefix(dec_int<4>{}); break;  // 3 tiles run as 4, the last one padding
  }
  int* const cn = (g.fuse && p.cnt != nullptr) ? p.cnt : nullptr;
  bf16_t* const fin = cn != nullptr ? p.out : nullptr;
  dim3 sgrid(g.nsuf, p.Hkv, p.B);
  decode_attn_loop_group_kernel<D, GQ, ROPE><<<sgrid, 256, 0, st>>>(
      p.q, p.q_sb, p.q_sh, p.kc, p.vc, p.c_sb, p.c_st, p.c_sh, p.kv_len, p.kv_start, p.window,
      p.scale_log2, ntot, g.cpb_s, p.part_o, p.part_ml, p.Hq, p.rope, fin, p.o_sb, p.o_sh, cn, p.Tmax, gp);
  if (fin == nullptr) launch_decode_combine<D>(p, ntot, st);
}

// partial slots per (row, q head); a group-structured step: prefix splits, then suffix splits
int decode_splits(const DecodeParams& p) {
  if (p.G == 0) return decode_num_splits(p.Tmax, p.B, p.Hkv);
  const DecGroupGeom g = decode_group_geom(p.Tmax, p.B, p.Hq, p.Hkv, p.G, p.Tp);
  return g.npre + g.nsuf;
}

void launch_decode(const DecodeParams& p, hipStream_t st) {
  decode_dispatch(p, [&](auto d, auto gq, auto rope) {
    constexpr int D = decltype(d)::value, GQ = decltype(gq)::value;
    constexpr bool ROPE = decltype(rope)::value;
    if (p.G > 0) launch_decode_group<D, GQ, ROPE>(p, st);
    else launch_decode_rows<D, GQ, ROPE>(p, st);
  });
}

}  // namespace dla
