// Launch geometry of the decode projection GEMMs (skinny.hip, skinny64.hip): split counts, kernel
// family choice, waves per workgroup, ring depths and LDS sizes, with every DLA_* switch they read
// (once per process). Pure host C++ (no HIP, no torch), so the choice is testable without a GPU
// (tests/test_skinny_geom_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace dla {

constexpr int kSkWaves = 8;             // waves per workgroup; each owns 16 output columns
constexpr int kSkCols = 16 * kSkWaves;  // output columns (weight rows) per workgroup
constexpr int kSkUnroll = 8;            // k-steps (32 each) of weight loads in flight per wave
constexpr int kSkChunk = 32 * kSkUnroll;
constexpr int kKsUnroll = 4;  // k-steps per chunk (one 16-byte W and x load per lane each)
constexpr int kKsChunk = 32 * kKsUnroll;
constexpr int kM64Waves = 8;
constexpr int kM64Ck = 256;         // k per x chunk and per weight ring slot
constexpr int kM64Ld = kM64Ck + 8;  // LDS row stride in bf16 (16-byte pad)

// Dynamic LDS limits: what hipFuncSetAttribute raises the kernels to and what the ops check x against
constexpr int64_t kSkLdsMax = 160 * 1024;     // skinny_gemm_kernel, plain and swiglu input
// the GLU variant also holds an 8 KB static exchange tile: dynamic + static <= 160 KB
constexpr int64_t kSkLdsGluMax = 152 * 1024;
constexpr int64_t kSkLdsNormMax = 150 * 1024;  // norm-on-input GLU kernels (skinny_gemm NPRE, skinny_glu_il)
constexpr int64_t kSkLdsNormX = 148 * 1024;    // the x image the ops admit to those
constexpr int64_t kM64LdsMax = 80 * 1024;      // m64_gemm_kernel

inline int skinny_env(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// skinny_gemm_kernel / skinny_glu_il_kernel: M rows of a kc-deep slice, 16-byte row pad
inline int64_t skinny_lds_bytes(int M, int kc) { return static_cast<int64_t>(M) * (kc + 8) * 2; }

// m64_gemm_kernel: a 2-slot ring of 16 mt rows x kM64Ld bf16
inline int m64_row_tiles(int M) { return M <= 32 ? 2 : 4; }
inline int64_t m64_lds_bytes(int mt) { return static_cast<int64_t>(2 * 16 * mt * kM64Ld) * 2; }

inline int skinny_splits(int M, int N, int K) {
  // Column blocks >= 128 (8 waves each: >= 4 waves per CU): no split (an in-kernel split-K combine costs each
  // workgroup an agent-scope release, measured 1.5-2x slower at 900-4000 workgroups). Otherwise
  // the smallest split count (K-slices a multiple of kSkChunk) giving >= `target` workgroups
  // (DLA_SKINNY_WG, default 256: one 8-wave workgroup per CU).
  static const int target = skinny_env("DLA_SKINNY_WG", 256);
  const int nb = (N + kSkCols - 1) / kSkCols;
  if (nb >= 128) return 1;
  const int chunks = K / kSkChunk;
  int best = chunks;
  for (int s = 1; s <= chunks; ++s) {
    if (chunks % s) continue;
    const int kc = K / s;
    if (static_cast<int64_t>(M) * (kc + 8) * 2 > 65536) continue;
    best = s;
    if (static_cast<int64_t>(nb) * s >= target) break;
  }
  return best;
}

inline bool skinny_use_ksplit(int N, int K) {
  return (N + kSkCols - 1) / kSkCols < 128 && (K % (8 * kKsChunk)) == 0 && N % 16 == 0;
}

inline bool skinny_glu_ks_ok(int N, int K) { return (K % (4 * kKsChunk)) == 0 && N % 32 == 0; }

// In-workgroup split-K ring depth at M <= 16: a 2-deep ring (84 VGPRs: 5-6 waves per SIMD, every
// qkv block resident in one round); a 4-deep ring (152 VGPRs) measured slower at qkv (16.0 vs 14.8
// us in a decode step). Long K (the 14336-deep down projection: 14 ring slots per wave, one
// workgroup per CU) keeps a 4-deep ring in flight (DLA_SKINNY_DEEP_K, default 8192: K at or above it)
inline int skinny_ks_depth(int K) {
  static const int deep_k = skinny_env("DLA_SKINNY_DEEP_K", 8192);
  return K >= deep_k ? 4 : 2;
}

// DLA_KS_F8_DEPTH (2 or 4): ring depth. Graph decode, Llama-3-8B B=8, same box: 2.62 ms/token
// at depth 2 vs 2.73 at 4 (fewer VGPRs, more resident waves beat more bytes in flight per wave)
inline int skinny_ks_f8_depth() {
  static const int depth = skinny_env("DLA_KS_F8_DEPTH", 2) == 4 ? 4 : 2;
  return depth;
}

// skinny_glu_il_kernel ring depth: DLA_GLU_IL_DEPTH (2, 3 or 4) for A/B runs; fp8:
// DLA_GLU_IL_F8_DEPTH (2, 3 or 4), same A/B: 2.712 / 2.710 / 2.729 ms/token
inline int glu_il_depth(bool f8) {
  static const int d16 = std::min(std::max(skinny_env("DLA_GLU_IL_DEPTH", 2), 2), 4);
  static const int d8 = std::min(std::max(skinny_env("DLA_GLU_IL_F8_DEPTH", 3), 2), 4);
  return f8 ? d8 : d16;
}

// skinny_glu_il_kernel waves per workgroup: the largest of 8..4 dividing the tile count with
// >= 256 workgroups, else 8. DLA_GLU_IL_WAVES (0 = auto) overrides it on the bf16 weight for A/B runs
inline int glu_il_waves(int ntiles, int M, bool f8) {
  static const int waves = [] {
    const int v = skinny_env("DLA_GLU_IL_WAVES", 0);
    return (v >= 1 && v <= 8) ? v : 0;
  }();
  int w = 8;
  for (int c : {8, 7, 6, 5, 4}) {
    if (ntiles % c == 0 && ntiles / c >= 256) { w = c; break; }
  }
  if (!f8 && waves > 0 && M <= 4 * waves) w = waves;  // the rstd waves cover 4 rows each
  return w;
}

inline bool m64_shape_ok(int N, int K) { return K % kM64Ck == 0 && N % 128 == 0; }

// Split-K count: the most splits that keep the grid within one workgroup per CU. A grid of 1.5
// workgroups per CU (the qkv projection at Llama-3-8B: 48 column blocks x 8 splits = 384) leaves
// half the CUs streaming twice the bytes of the rest; 48 x 4 = 192 workgroups ran the same GEMM +
// reduce in 21.4 vs 26.9 us (B = 64, a round-4 probe since removed). DLA_M64_WG=n (A/B) restores the
// round-3 rule: the fewest splits whose grid reaches n workgroups.
inline int m64_splits(int N, int K, int cus) {
  static const int target = skinny_env("DLA_M64_WG", 0);
  const int nb = N / (16 * kM64Waves);
  const int chunks = K / kM64Ck;
  // split counts the reduce kernel is instantiated for
  if (target > 0) {
    for (int s : {1, 2, 4, 7, 8, 14, 16}) {
      if (chunks % s) continue;
      if (nb * s >= target) return s;
    }
    for (int s : {16, 14, 8, 7, 4, 2}) if (chunks % s == 0) return s;
    return 1;
  }
  // (a grid of fewer column blocks than CUs always splits at least once, as the round-3 rule did:
  // the residual / norm epilogues live in the reduce launch)
  int best = 1;
  for (int s : {2, 4, 7, 8, 14, 16})
    if (chunks % s == 0 && (nb * s <= cus || (best == 1 && nb < cus))) best = s;
  return best;
}

// fp8 weights (tiled, nt): DLA_M64_F8_DEPTH = weight chunks in flight per wave (2, 3 or 4; a chunk
// is half the bf16 bytes, so the same bytes in flight take twice the chunks)
inline int m64_f8_depth() {
  static const int depth = [] {
    const int d = skinny_env("DLA_M64_F8_DEPTH", 3);
    return d >= 2 && d <= 4 ? d : 3;
  }();
  return depth;
}

}  // namespace dla
