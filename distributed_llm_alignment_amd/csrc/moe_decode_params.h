// Launch contract of the decode-shaped MoE expert block, shared by moe_decode.hip (kernels and
// launchers) and bindings_moe.cpp (torch ops, every host check). Two launches take route_topk's
// outputs to the block's output: no sort, no offsets, no dispatch copy, no combine launch.
// Trusted, not checked on the device (a host check would need a sync): 0 <= topi < E and a
// token's k experts are distinct, both guaranteed by route_topk.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dla {

using bf16_t = uint16_t;

constexpr int kMdMaxRows = 64;   // token rows M: an expert sees at most M slots, four 16-row tiles
constexpr int kMdMaxTopK = 8;    // so at most 512 slots, 8 per lane of one wave
constexpr int kMdGluWaves = 4;   // waves splitting K = H in moe_decode_glu_kernel
constexpr int kMdDownWaves = 8;  // waves splitting K = F in moe_decode_down_kernel

struct MoeDecodeParams {
  const bf16_t* h2;      // [M, H] token rows, row stride ldh
  int64_t ldh;
  const int* topi;       // [M, k] expert of slot s = t k + j
  const float* topv;     // [M, k] routing weight of the slot (down only)
  const bf16_t* w_up;    // [E, 2F, H] = [gate; up], as the parameter is stored
  const bf16_t* w_down;  // [E, H, F]
  bf16_t* a;             // [M k, F] silu(gate) * up, indexed by slot: written by glu, read by down
  bf16_t* out;           // [M, H] (down only)
  int M, k, E, H, F;     // H % 32 == 0, F % 32 == 0
};

// moe_decode_glu_kernel, grid (F / 16, E): a[slot] for every slot, unrouted experts exit at once
void launch_moe_decode_glu(const MoeDecodeParams& p, hipStream_t st);
// moe_decode_down_kernel, grid (H / 16): out = sum over a token's experts in index order
void launch_moe_decode_down(const MoeDecodeParams& p, hipStream_t st);

}  // namespace dla
