// Split geometry of the decode attention launches (decode.hip): how many 128-key chunks a block
// takes and how many partial slots a (row, q head) gets. Pure host C++ (no HIP, no torch), so the
// choice is testable without a GPU (tests/test_decode_geom_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace dla {

constexpr int kDecChunk = 128;  // keys per block (4 waves x 32)
constexpr int kDecMaxFuse = 8;  // most splits the in-kernel combine merges

// Target block count of a decode launch: DLA_DECODE_BLOCKS (default 256); 0 with DLA_DECODE_LOOP=0
// (one chunk per block). Read per call (cheap next to a launch) so a test can force the loop
// kernel at small shapes.
inline int decode_block_target() {
  const char* e = getenv("DLA_DECODE_LOOP");
  const char* tb = getenv("DLA_DECODE_BLOCKS");
  return (e != nullptr && atoi(e) == 0) ? 0 : (tb ? atoi(tb) : 256);
}

// DLA_DECODE_LOOP=0: one 128-key chunk per block (decode_attn_kernel); otherwise blocks loop over
// chunks so that B x Hkv x splits stays near DLA_DECODE_BLOCKS (default 256; same-box graph decode:
// B = 8 / 1152 keys 3 chunks per block 3.98-4.00 vs 4.02 ms/token one-chunk, 2 chunks 4.03-4.06,
// 9 chunks (no combine) 4.25; B = 64 / ~576 keys: one split per sequence)
inline int decode_cpb(int Tmax, int B, int Hkv) {
  const int target = decode_block_target();
  const int nch = (Tmax + kDecChunk - 1) / kDecChunk;
  if (target <= 0) return 0;
  const int64_t blocks = static_cast<int64_t>(B) * Hkv * nch;
  const int cpb = static_cast<int>((blocks + target - 1) / target);
  // Below DLA_DECODE_LOOP_MIN chunks per block the one-chunk kernel (3 blocks per CU) + the combine
  // launch. Round 3 measured that faster under 3 chunks (B = 8, 1152 keys: 4.05 vs 4.12 ms/token);
  // with the in-kernel combine the loop kernel now wins at 2 chunks and at 1 chunk whenever the
  // splits fit the fused combine (B = 8, 512 + 256 tokens: 3.466-3.473 at 2, 3.485-3.497 at 1 vs
  // 3.542-3.548 ms/token, same box, tools/gpu_passes.py r6-decode-combine)
  const char* mn = getenv("DLA_DECODE_LOOP_MIN");
  const int min_cpb = mn ? atoi(mn) : 2;
  if (cpb < min_cpb) return (mn == nullptr && cpb == 1 && nch <= kDecMaxFuse) ? 1 : 0;
  return std::min(cpb, nch);
}

inline int decode_num_splits(int Tmax, int B, int Hkv) {
  const int nch = (Tmax + kDecChunk - 1) / kDecChunk;
  const int cpb = decode_cpb(Tmax, B, Hkv);
  return cpb == 0 ? nch : (nch + cpb - 1) / cpb;
}

// ---- group-structured step (DecGroup): split geometry
// Row tiles of at most 64 query columns (rpt rows x GQ heads), prefix chunks [0, ceil(Tp / 128))
// and suffix chunks [Tp / 128, ceil(Tmax / 128)) each cut so that the grid stays near
// DLA_DECODE_BLOCKS (default 256) blocks, as decode_cpb does for the per-row kernel; the prefix
// cut is coarsened until prefix + suffix slots fit the in-kernel combine when they can.
// When the suffix alone takes kDecMaxFuse splits there is no slot left for the prefix: the step
// then runs the separate combine launch (a third launch) where the per-row op at that shape still
// fuses. DLA_DECODE_LOOP=0: one chunk per block on both sides and the separate combine launch.
struct DecGroupGeom {
  int rpt, ntile, nt, cpb_p, cpb_s, npre, nsuf, c0;
  bool fuse;
};

inline DecGroupGeom decode_group_geom(int Tmax, int B, int Hq, int Hkv, int G, int Tp) {
  const int target = decode_block_target();
  const int GQ = Hq / Hkv, P = B / G;
  DecGroupGeom g{};
  g.rpt = std::min(G, 64 / GQ);
  g.ntile = (G + g.rpt - 1) / g.rpt;
  g.nt = (g.rpt * GQ + 15) / 16;
  const int nch = (Tmax + kDecChunk - 1) / kDecChunk;
  const int nchp = (Tp + kDecChunk - 1) / kDecChunk;
  g.c0 = std::min(Tp / kDecChunk, nch - 1);
  const int nchs = nch - g.c0;
  g.fuse = target > 0;
  if (target <= 0) {
    g.cpb_p = g.cpb_s = 1;
  } else {
    const int64_t bp = static_cast<int64_t>(P) * g.ntile * Hkv * nchp;
    const int64_t bs = static_cast<int64_t>(B) * Hkv * nchs;
    g.cpb_p = static_cast<int>(std::min<int64_t>(std::max<int64_t>((bp + target - 1) / target, 1), nchp));
    g.cpb_s = static_cast<int>(std::min<int64_t>(std::max<int64_t>((bs + target - 1) / target, 1), nchs));
  }
  g.nsuf = (nchs + g.cpb_s - 1) / g.cpb_s;
  g.npre = (nchp + g.cpb_p - 1) / g.cpb_p;
  if (g.fuse && g.nsuf < kDecMaxFuse && g.npre + g.nsuf > kDecMaxFuse) {
    g.cpb_p = (nchp + (kDecMaxFuse - g.nsuf) - 1) / (kDecMaxFuse - g.nsuf);
    g.npre = (nchp + g.cpb_p - 1) / g.cpb_p;
  }
  g.fuse = g.fuse && g.npre + g.nsuf <= kDecMaxFuse;
  return g;
}

}  // namespace dla
