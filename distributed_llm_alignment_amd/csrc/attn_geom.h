// Launch plan of the training / prefill flash attention (attention.hip): every decision the host
// takes between an attn_fwd / attn_bwd call and its kernel launches -- which kernel, how many
// workgroups, how large the scratch buffers, in which dtype. bindings_attention.cpp plans once per
// call, allocates from the plan and hands it to the launchers, which decide nothing. Pure host C++
// (no HIP, no torch), so the choice is testable without a GPU (tests/test_attn_geom_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace dla {

// Backward geometry: one workgroup per (256-key block, GQA head subset, kv head, batch);
// queries are swept in 32-row tiles.
constexpr int kAttnBwdKeys = 256;
constexpr int kAttnBwdQRows = 32;

// ---- forward
// 8 waves (256 queries) per workgroup. A 4-wave / 128-query variant (two independent
// workgroups per CU, unaligned barriers) measured 31-35 % slower at T = 1024 and 4096.
struct AttnFwdPlan {
  int D;
  bool causal, prefix;
  int hp;        // GQA heads sharing a workgroup (and every K/V tile in LDS): 4, 2 or 1
  int bq;        // query rows of each head per workgroup: 256 / hp
  int64_t nblk;  // (query block, head set, batch) work items
  bool persist;  // attn_fwd_persist_kernel: `grid` workgroups loop over the nblk items
  int64_t grid;
};

// DLA_ATTN_FWD_HP=1|2|4 caps the heads per workgroup for A/B runs; read once per process.
inline int attn_fwd_hp_cap() {
  static const int forced = [] {
    const char* e = getenv("DLA_ATTN_FWD_HP");
    return e ? atoi(e) : 0;
  }();
  return forced > 0 ? forced : 4;
}

// Persistent forward: DLA_ATTN_FWD_PERSIST=1 always, =0 never, unset = for key ranges of at most
// 512 (<= 8 tiles per block), where it measured faster: graph-timed, B*T = 8192, Hq 32 / Hkv 8 /
// D 128 (profiles/r5_attention_fwd.md) causal 240 -> 290-318 TF/s at T 256 and 413 -> 469-472 at
// T 512, equal at 1024, 5 % slower at 2048-4096. Read per call so one process can A/B both
// (tools/attn_fwd_sweep.py --cfg, tests/test_kernels_gpu.py).
inline bool attn_fwd_persist(int64_t Tk) {
  const char* e = getenv("DLA_ATTN_FWD_PERSIST");
  if (e == nullptr || *e == '\0') return Tk <= 512;
  return atoi(e) != 0;
}

// hp: 4 (64-query blocks, 2 waves per head) when the group size allows it, else 2, else 1. Same-box
// A/B (B8 T1024 Hq32 Hkv8 D128, tools/gpu_attn_env_ab.sh): causal 140-148 / 131-133 / 124-129 us
// for HP 1 / 2 / 4, non-causal 217 -> 205-209 us, T = 4096 unchanged (366-379 us).
inline AttnFwdPlan attn_fwd_plan(int64_t B, int64_t Hq, int64_t Hkv, int64_t Tq, int64_t Tk, int D, bool causal,
                                 bool has_prefix, int cus) {
  AttnFwdPlan g{};
  g.D = D;
  g.causal = causal;
  g.prefix = has_prefix;
  const int64_t group = Hq / Hkv;
  const int want = attn_fwd_hp_cap();
  g.hp = (want >= 4 && group % 4 == 0) ? 4 : (want >= 2 && group % 2 == 0) ? 2 : 1;
  g.bq = 256 / g.hp;
  g.nblk = (Tq + g.bq - 1) / g.bq * (Hq / g.hp) * B;
  // the shared prefix runs on attn_fwd_kernel only (the persistent one has no second key range);
  // the persistent kernel counts its work items in an int
  g.persist = !has_prefix && attn_fwd_persist(Tk) && g.nblk < (int64_t(1) << 30);
  // persistent: one 8-wave workgroup per CU (230 VGPRs: two waves per SIMD), never more than the blocks
  g.grid = g.persist ? std::min<int64_t>(g.nblk, cus) : g.nblk;
  return g;
}

// ---- backward
struct AttnBwdPlan {
  int D;
  bool causal;
  int waves;           // main kernel: attn_bwd8_kernel (8) or attn_bwd_kernel (4)
  int64_t nkb;         // 256-key blocks
  int64_t slab_rows;   // Tq rounded up to a multiple of kAttnBwdQRows (dq_slab row count)
  bool slab16;         // dQ slabs in bf16
  int hsplit;          // GQA group split across workgroups
  bool part16;         // dK / dV head-split partials in bf16 (hsplit > 1 only)
  int64_t delta_grid;  // attn_bwd_delta_kernel
  int64_t grid;        // main kernel
  int64_t dq_grid;     // attn_dq_reduce_kernel
  int64_t dkv_grid;    // attn_dkv_reduce_kernel (hsplit > 1 only)
};

// Main kernel: 8 waves by default, 4 with DLA_ATTN_BWD_WAVES=4. Same-box A/B, B8 T1024 Hq32 Hkv8
// D128 causal, all backward passes: 489 -> 410 us; non-causal 624 -> 549 us
// (profiles/r3_attention_bwd.md). Read per call (not cached) so one process can A/B both.
inline int attn_bwd_waves() {
  const char* e = getenv("DLA_ATTN_BWD_WAVES");
  return (e && atoi(e) == 4) ? 4 : 8;
}

// bf16 dQ slabs (DLA_ATTN_DQ_BF16=0 keeps fp32) and bf16 dK / dV head-split partials
// (DLA_ATTN_DKV_BF16=0 keeps fp32): the 8-wave kernel only. Read per call, like the wave count.
inline bool attn_bwd_bf16_scratch(const char* name, int waves) {
  const char* e = getenv(name);
  return waves == 8 && !(e && atoi(e) == 0);
}

// GQA heads of one kv head split across `hs` backward workgroups when the (key block x kv head x
// batch) grid alone would under-fill the chip: causal key blocks carry unequal work (block 0
// sees every query), so target two workgroups per CU there and let the heaviest-first dispatch
// balance them. Partial dK/dV of the splits are summed by a reduce pass.
inline int attn_bwd_hsplit(int64_t nkb, int64_t Hkv, int64_t B, int64_t group, bool causal, int cus) {
  const int64_t base = nkb * Hkv * B;
  const int64_t target = causal ? 2 * static_cast<int64_t>(cus) : cus;
  int hs = 1;
  while (base * hs < target && group % (2 * hs) == 0) hs *= 2;
  return hs;
}

// Grid of a grid-stride reduce pass over `work` 16-byte items, 256 threads per block; 0 = no launch.
inline int64_t attn_stream_grid(int64_t work) {
  // grid-stride cap of the reduce passes: 1024 / 8192 / 32768 measured as noise against 2048
  constexpr int64_t cap = 2048;
  return work <= 0 ? 0 : std::min((work + 255) / 256, cap);
}

inline AttnBwdPlan attn_bwd_plan(int64_t B, int64_t Hq, int64_t Hkv, int64_t Tq, int64_t Tk, int D, bool causal,
                                 bool has_rope, int rope_rot, int cus) {
  AttnBwdPlan g{};
  g.D = D;
  g.causal = causal;
  g.waves = attn_bwd_waves();
  g.nkb = (Tk + kAttnBwdKeys - 1) / kAttnBwdKeys;
  g.slab_rows = (Tq + kAttnBwdQRows - 1) / kAttnBwdQRows * kAttnBwdQRows;
  g.slab16 = attn_bwd_bf16_scratch("DLA_ATTN_DQ_BF16", g.waves);
  g.hsplit = attn_bwd_hsplit(g.nkb, Hkv, B, Hq / Hkv, causal, cus);
  g.part16 = g.hsplit > 1 && attn_bwd_bf16_scratch("DLA_ATTN_DKV_BF16", g.waves);
  const int64_t rows_per_block = 4 * (64 / (D <= 64 ? 8 : 16));  // as attn_bwd_delta_kernel
  g.delta_grid = (B * Hq * Tq + rows_per_block - 1) / rows_per_block;
  g.grid = Tq == 0 ? 0 : g.nkb * Hkv * B * g.hsplit;
  // work items per row of the reduce passes: a rotary pair of 8-column chunks, or one chunk
  const int64_t items = has_rope ? rope_rot / 16 + (D - rope_rot) / 8 : D / 8;
  g.dq_grid = attn_stream_grid(B * Tq * Hq * items);
  g.dkv_grid = g.hsplit > 1 ? attn_stream_grid(B * Tk * Hkv * items) : 0;
  return g;
}

}  // namespace dla
