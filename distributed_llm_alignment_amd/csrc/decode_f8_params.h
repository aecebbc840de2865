// Launch contract of the e4m3 KV cache (decode_f8.hip launchers, bindings_decode_f8.cpp torch ops).
//
// Format of record: per (cache row b, token t, kv head h) one fp32 scale for K and one for V,
//   sc = max(amax / 448, 1e-12),  code = e4m3fn_rne(clamp(x * (1 / sc), -448, 448)),  deq = code * sc
// with every operation one correctly rounded fp32 operation (ops.decode.quantize_kv_f8 is the CPU
// formula). Codes are bytes [B, Tmax, Hkv, D] (D contiguous), scales fp32 [B, Tmax, Hkv]; both are
// strided views, K and V sharing strides. All structs are host-side only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dla {

using bf16_t = uint16_t;

// One layer's e4m3 cache. Code strides in bytes (multiples of 16), scale strides in floats.
struct KvF8 {
  uint8_t* k8;
  uint8_t* v8;
  int64_t c_sb, c_st, c_sh;
  float* ks;
  float* vs;
  int64_t z_sb, z_st, z_sh;
  int Tmax;
};

// Prefill fill: src [B, T, Hkv, D] bf16 (strides in elements) -> codes / scales of tokens [t0, t0 + T)
struct KvQuantParams {
  const bf16_t* src;
  int64_t s_sb, s_st, s_sh;
  uint8_t* codes;
  int64_t c_sb, c_st, c_sh;
  float* scale;
  int64_t z_sb, z_st, z_sh;
  int B, T, Hkv, D, t0;
};
void launch_kv_quant_f8(const KvQuantParams& p, hipStream_t st);

// Decode-step prologue: qkv rows of the newest token -> rotated q_out [B, Hq, D] (bitwise
// launch_rope_cache's), rotated k / plain v quantised into cache slot *slot.
struct RopeCacheF8Params {
  const bf16_t* qkv;
  int64_t ld;
  bf16_t* q_out;
  KvF8 c;
  const int64_t* slot;
  const float* cos_t;
  const float* sin_t;
  const int* pos;
  int B, Hq, Hkv, D, rot;
};
void launch_rope_cache_f8(const RopeCacheF8Params& p, hipStream_t st);

// Split-KV decode attention over the e4m3 cache; partials in the layout of DecodeParams
// (part_o [B, Hq, nsplit, D], part_ml [B, Hq, nsplit, 2]), nsplit = decode_f8_splits().
struct DecodeF8Params {
  const bf16_t* q;  // [B, Hq, D] rotated queries
  int64_t q_sb, q_sh;
  KvF8 c;
  const int* kv_len;    // device scalar
  const int* kv_start;  // [B] or null
  int window;
  float scale_log2;  // softmax scale * log2(e)
  int B, Hq, Hkv, D;
  float* part_o;
  float* part_ml;
  bf16_t* out;  // [B, Hq, D]
  int64_t o_sb, o_sh;
};
int decode_f8_splits(const DecodeF8Params& p);
void launch_decode_f8(const DecodeF8Params& p, hipStream_t st);

}  // namespace dla
