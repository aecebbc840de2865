// The decode step's RoPE row helper, shared by decode.hip (fused prologue) and decode_f8.hip
// (quantising prologue): both must round q and k exactly alike.
#pragma once
#include "common.h"

namespace dla {

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

}  // namespace dla
