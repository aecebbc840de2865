// Launch contract of the decode attention step, shared by decode.hip (launchers) and
// bindings_decode.cpp (torch ops). DecodeParams is host-side only: the kernels keep their own
// `const ... __restrict__` pointer parameters; DecRope is a kernel argument as it stands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dla {

using bf16_t = uint16_t;

// Fused decode-step prologue (ROPE = true): instead of a separate rope + cache-write launch, the
// kernel reads the raw qkv row of the newest token: every block rotates its G query heads while
// filling `qs`; the newest key's K/V (rotated k, plain v) come from registers rather than the
// cache, and the block whose split holds that key writes them into the cache slot for the next
// steps. Rounding matches rope_cache_kernel + the unfused kernel (q and k rounded to bf16 after
// the rotation), so fused and unfused decode agree bitwise.
struct DecRope {
  const bf16_t* qkv;  // [B, (Hq + 2 Hkv) * D] rows of the newest token
  int64_t ld;
  const float* cos_t;  // [P, rot/2]
  const float* sin_t;
  const int* pos;      // [B] rope position of the newest token
  const int64_t* slot; // cache slot of the newest token (== kv_len - 1)
  int rot;
  int Hkv;
};

struct DecodeParams {
  const bf16_t* q;  // [B, Hq, D] rotated queries, or null: the fused form, `rope` set
  int64_t q_sb, q_sh;
  DecRope rope;     // rope.qkv != null: raw qkv rows, rope + cache write of the newest token fused in
  bf16_t* kc;       // caches [B, Tmax, Hkv, D], k and v sharing strides
  bf16_t* vc;
  int64_t c_sb, c_st, c_sh;
  const int* kv_len;    // device scalar
  const int* kv_start;  // [B] or null
  int window;
  float scale_log2;  // softmax scale * log2(e)
  int B, Hq, Hkv, D, Tmax;
  int G;   // rows per prompt of a group-structured step (decode.hip DecGroup); 0: per-row
  int Tp;  // shared prefix length (keys), G > 0 only
  float* part_o;   // [B, Hq, decode_splits, D]
  float* part_ml;  // [B, Hq, decode_splits, 2]
  bf16_t* out;     // [B, Hq, D]
  int64_t o_sb, o_sh;
  int* cnt;  // arrival counters of the in-kernel split combine, or null: the combine launch
};

// partial slots per (row, q head): part_o / part_ml are sized by this
int decode_splits(const DecodeParams& p);
void launch_decode(const DecodeParams& p, hipStream_t st);

// qkv rows of the newest token -> rotated q_out [B, Hq, D], rotated k / plain v into cache row *slot
void launch_rope_cache(const bf16_t* qkv, int64_t ld, bf16_t* q_out, bf16_t* kc, bf16_t* vc,
                       int64_t c_sb, int64_t c_st, int64_t c_sh, const int64_t* slot,
                       const float* cos_t, const float* sin_t, const int* pos, int B, int Hq,
                       int Hkv, int D, int rot, hipStream_t st);

}  // namespace dla
