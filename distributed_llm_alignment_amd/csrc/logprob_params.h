// Launch contract of the LM-head row kernels, shared by logprob.hip (launchers) and
// bindings_logprob.cpp (torch ops). LogprobParams is host-side only: the kernels keep their scalar
// argument lists, the launchers unpack the struct at the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dla {

using bf16_t = uint16_t;

// One struct for the forward, the in-place backward and the transposing backward. The launchers
// pick the instantiation from it: VEC = V % 8 == 0 && ld % 8 == 0, TEMP = temp, MASK = keep != null,
// ENT = ent != null (forward) or ge != null (backwards).
struct LogprobParams {
  bf16_t* logits;  // [rows, V], row stride ld; read by the forward, rewritten in place by the backwards
  int64_t ld;
  int V;
  int64_t rows;
  int64_t off;  // first vocabulary entry of this shard (0: the unsharded head)
  const int64_t* tgt;  // [rows]
  // TEMP: softmax(inv_temp * logits). A flag of its own, not inv_temp != 1: the tempered
  // instantiations at inv_temp = 1 are other kernels than the plain ones (with the same bits).
  bool temp;
  float inv_temp;
  const uint8_t* keep;       // [M, V / 8] packed keep mask, or null
  const int64_t* keep_rows;  // [rows] mask row of every logits row (< 0: none)
  float* logp;  // [rows] forward output
  float* lse;   // [rows] forward output, backward input
  float* ent;   // [rows] forward output (null: no entropy), backward input with ge
  const float* g;   // [rows] dL/dlogp
  const float* ge;  // [rows] dL/dent, or null: the non-entropy backward
  bf16_t* outT;     // [V, rows] second output of the transposing backward
};

// No kernel exists for a keep mask without temp, with the entropy, with V % 8 or ld % 8 nonzero or
// with a vocabulary shard (off != 0): these throw std::invalid_argument, nothing is launched.
void launch_logprob_fwd(const LogprobParams& p, hipStream_t st);
void launch_logprob_bwd(const LogprobParams& p, hipStream_t st);
// false (nothing launched) when rows, V or ld is not a multiple of 8: run launch_logprob_bwd
bool launch_logprob_bwd_t(const LogprobParams& p, hipStream_t st);

void launch_row_lse(const bf16_t* logits, int64_t ld, int V, int64_t rows, float* lse, hipStream_t st);
void launch_ensemble_kl(bf16_t* s_logits, const bf16_t* t_logits, int64_t ld, int64_t t_stride, int K, int V,
                        const float* s_lse, const float* t_lse, int64_t rows, const float* g, float* kl,
                        bool write_grad, hipStream_t st);

}  // namespace dla
