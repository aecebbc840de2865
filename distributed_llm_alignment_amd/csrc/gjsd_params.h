// Launch contract of the JSD(beta) row kernels, shared by gjsd.hip (kernels, launcher) and
// bindings.cpp (torch ops). The struct is the kernel argument as it stands.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dla {

using bf16_t = uint16_t;

constexpr int kGjsdMaxTeachers = 8;

struct GjsdParams {
  const bf16_t* s;   // student logits [N, V], row stride s_ld (elements)
  const bf16_t* t;   // teacher logits [K, N, V], strides t_sk, t_ld (elements)
  int64_t s_ld, t_sk, t_ld, N;
  int K, V;
  const void* mask;  // row mask [N], float or uint8 (mask_u8); nullptr: every row is live
  int mask_u8;
  float beta, c;     // c = 1 - beta, and 1 at beta = 1
  float it;          // inverse temperature
  float lb, l1b;     // log beta, log(1 - beta): formed in double by the host (unused at the end points)
  float logK, invK;
  float* loss;       // [N]  forward out
  float* aux;        // [N]  forward out / backward in: A (0 at beta = 0)
  float* s_lse;      // [N]  forward out / backward in
  float* t_lse;      // [K, N]
  const float* g;    // backward: dL/dloss [N]
  bf16_t* ds;        // backward out: [N, V] contiguous
};

// forward (bwd = false) or backward on stream st; N == 0 launches nothing. The 16 B path needs
// V % 8 == 0, every stride a multiple of 8 and 16-byte-aligned bases; otherwise the scalar loop runs.
void launch_gjsd(const GjsdParams& p, bool bwd, hipStream_t st);

}  // namespace dla
