// Torch ops of the training / prefill flash attention (csrc/attention.hip): attn_fwd, attn_bwd,
// attn_stamps, attn_fwd_switch. Host-only. Each op checks every operand, builds the launch plan
// (attn_geom.h) once, refuses a plan whose grids do not fit, and only then allocates from the plan
// and calls the direction's one launcher on the current stream: a refused call has written nothing.
//
// Every tensor operand goes through a helper that also holds it to q's device; B, Hq, Hkv, Tq, Tk
// go through to_int() because the kernels index with int.
#include <ATen/ATen.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>

#include "attn_params.h"
#include "bind_util.h"

namespace dla {

using OptT = c10::optional<at::Tensor>;

static bool given(const OptT& t) { return t && t->defined(); }

// ---- shared operand rules
// [B, T, H, D] bf16, unit D stride, the other strides multiples of 8 elements, 16-byte aligned
static void check_bthd(const at::Tensor& t, const at::Tensor& q, const char* name) {
  check_bf16(t, name);
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1, name, " must be [B, T, H, D] with unit d stride");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 && t.stride(2) % 8 == 0, name,
              " strides must be multiples of 8 elements");
  check_aligned16(t, name);
  same_device(q, t);
}

static void set_strides(const at::Tensor& t, int64_t& sb, int64_t& st, int64_t& sh) {
  sb = t.stride(0);
  st = t.stride(1);
  sh = t.stride(2);
}

static int to_int(int64_t v, const char* what) {
  TORCH_CHECK(v >= 0 && v <= INT_MAX, "attention: ", what, " = ", v, " does not fit the kernels' int index");
  return static_cast<int>(v);
}

static void check_grid(int64_t grid, const char* what) {
  TORCH_CHECK(grid <= INT_MAX, "attention: the ", what, " grid of ", grid, " workgroups does not fit a launch");
}

template <class P>
static void set_sizes(P& p, int64_t B, int64_t Hq, int64_t Hkv, int64_t Tq, int64_t Tk) {
  p.B = to_int(B, "B");
  p.Hq = to_int(Hq, "Hq");
  p.Hkv = to_int(Hkv, "Hkv");
  p.Tq = to_int(Tq, "Tq");
  p.Tk = to_int(Tk, "Tk");
}

static const int* kv_range(const OptT& r, const at::Tensor& q, const char* name) {
  if (!given(r)) return nullptr;
  TORCH_CHECK(r->scalar_type() == at::kInt && r->is_contiguous() && r->numel() == q.size(0) && r->is_cuda(), name,
              " must be int32 [B] on GPU");
  same_device(q, *r);
  return r->data_ptr<int>();
}

// The mask and rotary fields both params structs share: per-batch key ranges; packed-sequence
// bounds `segs` [2, B, T] int32 (seg_start; seg_end: `seg` receives row `seg_row`), causal
// self-attention only; rotary tables for the fused RoPE paths: contiguous fp32 [max_pos, D/2]
// cos / sin, optional int32 [B*T] positions (else position = t), full rotary or (backward only:
// `partial_ok`) phi-2's partial rotary, 32 of D = 80 dims; self-attention only. Returns the rotary
// dims (0 without tables).
template <class P>
static int set_mask_rope(P& p, const int*& seg, int seg_row, bool partial_ok, const at::Tensor& q, int64_t Tk,
                         bool causal, int64_t causal_off, const OptT& kv_start, const OptT& kv_end, const OptT& segs,
                         const OptT& rope_cos, const OptT& rope_sin, const OptT& rope_pos) {
  const int64_t B = q.size(0), Tq = q.size(1), D = q.size(3);
  p.kv_start = kv_range(kv_start, q, "kv_start");
  p.kv_end = kv_range(kv_end, q, "kv_end");
  if (given(segs)) {
    TORCH_CHECK(segs->scalar_type() == at::kInt && segs->is_contiguous() && segs->dim() == 3 &&
                    segs->size(0) == 2 && segs->size(1) == B && segs->size(2) == Tq,
                "segs must be contiguous int32 [2, B, T]");
    TORCH_CHECK(causal && causal_off == 0 && Tq == Tk, "packed sequences need causal self-attention");
    same_device(q, *segs);
    seg = segs->data_ptr<int>() + seg_row * B * Tq;
  }
  if (!given(rope_cos)) return 0;
  TORCH_CHECK(given(rope_sin), "rope_sin missing");
  const int64_t half = rope_cos->dim() == 2 ? rope_cos->size(1) : -1;
  partial_ok = partial_ok && D == 80 && half == 16;
  for (const at::Tensor* t : {&*rope_cos, &*rope_sin}) {
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 2 &&
                    (t->size(1) == D / 2 || (partial_ok && t->size(1) == 16)),
                "rope cos/sin must be contiguous fp32 [max_pos, head_dim/2] (or [max_pos, 16] at "
                "head_dim 80 in the backward)");
    same_device(q, *t);
  }
  TORCH_CHECK(Tq == Tk && causal_off == 0, "fused RoPE needs self-attention");
  if (given(rope_pos)) {
    TORCH_CHECK(rope_pos->scalar_type() == at::kInt && rope_pos->is_contiguous() &&
                    rope_pos->numel() == B * Tq, "rope_pos must be contiguous int32 [B*T]");
    same_device(q, *rope_pos);
    p.rope_pos = rope_pos->data_ptr<int>();
  } else {
    TORCH_CHECK(Tq <= rope_cos->size(0), "positions exceed the rotary table");
  }
  p.rope_cos = rope_cos->data_ptr<float>();
  p.rope_sin = rope_sin->data_ptr<float>();
  return static_cast<int>(2 * half);
}

static int device_cus(int dev) {
  static int cache[64] = {0};
  if (dev < 0 || dev >= 64) return 256;
  if (cache[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
  }
  return cache[dev];
}

// ---- forward structure switches
struct AttnFwdSwitches {
  int prio, sgpr, pro, ostage, msub;
};

// Read from the environment ONCE per process (every switch defaults to its measured winner, the
// others exist for same-binary A/B runs); tests flip a switch through attn_fwd_switch instead of
// re-reading the environment on every launch.
//   prio 1: s_setprio 1 around each MFMA chain, so the matrix chain of one wave issues ahead
//     of its SIMD partner's softmax VALU (cdna guide T5). Same box, graph-timed, B*T 8192:
//     causal T1024 654 vs 613 TF/s, T4096 937 vs 897; non-causal +4-6 %. 2 (static priority
//     for waves 4-7) measured +0-7 % and below 1 everywhere; 0 = off.
//   msub (D = 128): same box, graph-timed, interleaved: causal T1024 701 vs 668 TF/s, T2048
//     898 vs 865, non-causal +3-7 % (gpurun_out/r5/attn13); outputs within one bf16 ulp
static AttnFwdSwitches& attn_fwd_switches() {
  static AttnFwdSwitches sw = [] {
    auto env = [](const char* name, int dflt) {
      const char* e = std::getenv(name);
      return e ? std::atoi(e) : dflt;
    };
    return AttnFwdSwitches{env("DLA_ATTN_FWD_PRIO", 1), env("DLA_ATTN_FWD_SGPR", 1), env("DLA_ATTN_FWD_PRO", 1),
                           env("DLA_ATTN_FWD_OSTAGE", 1), env("DLA_ATTN_FWD_MSUB", 1)};
  }();
  return sw;
}

// Flip one switch ("prio", "sgpr", "pro", "ostage", "msub") for this process (tests / same-binary
// A/B); returns the previous value.
int64_t attn_fwd_switch(c10::string_view name, int64_t value) {
  const std::string n(name.data(), name.size());
  AttnFwdSwitches& sw = attn_fwd_switches();
  int* f = n == "prio" ? &sw.prio : n == "sgpr" ? &sw.sgpr : n == "pro" ? &sw.pro : n == "ostage" ? &sw.ostage
           : n == "msub" ? &sw.msub : nullptr;
  TORCH_CHECK(f != nullptr, "attn_fwd_switch: unknown switch ", n);
  const int prev = *f;
  *f = static_cast<int>(value);
  return prev;
}

static at::Tensor& attn_stamp_buffer() {
  static at::Tensor buf;
  return buf;
}

at::Tensor attn_stamps(const at::Tensor& like) {
  (void)like;
  return attn_stamp_buffer().defined() ? attn_stamp_buffer().clone() : at::Tensor();
}

// ================================= forward ====================================================
std::tuple<at::Tensor, at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                            double scale, bool causal, int64_t causal_off, int64_t window,
                                            const OptT& kv_start, const OptT& kv_end, const OptT& segs,
                                            const OptT& rope_cos, const OptT& rope_sin, const OptT& rope_pos,
                                            const OptT& q_rot, bool rope_k, const OptT& prefix) {
  check_bthd(q, q, "q");
  check_bthd(k, q, "k");
  check_bthd(v, q, "v");
  const int64_t B = q.size(0), Tq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int64_t Tk = k.size(1), Hkv = k.size(2);
  TORCH_CHECK(D == 64 || D == 80 || D == 128, "head_dim must be 64, 80 or 128 (pad others)");
  TORCH_CHECK(k.size(0) == B && v.size(0) == B && k.size(3) == D && v.size(3) == D &&
                  v.size(1) == Tk && v.size(2) == Hkv,
              "k/v shapes");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  AttnParams p{};
  set_sizes(p, B, Hq, Hkv, Tq, Tk);
  p.q = cbp(q);
  p.k = cbp(k);
  p.v = cbp(v);
  set_strides(q, p.q_sb, p.q_st, p.q_sh);
  set_strides(k, p.k_sb, p.k_st, p.k_sh);
  set_strides(v, p.v_sb, p.v_st, p.v_sh);
  p.scale2 = static_cast<float>(scale * 1.4426950408889634);
  p.causal_off = static_cast<int>(causal_off);
  p.window = static_cast<int>(window);
  set_mask_rope(p, p.seg_start, 0, false, q, Tk, causal, causal_off, kv_start, kv_end, segs, rope_cos, rope_sin,
                rope_pos);
  if (given(prefix)) {  // shared prefix (ps, pe, qe) per batch row
    TORCH_CHECK(prefix->scalar_type() == at::kInt && prefix->is_contiguous() && prefix->dim() == 2 &&
                    prefix->size(0) == B && prefix->size(1) == 3,
                "prefix must be contiguous int32 [B, 3]");
    TORCH_CHECK(p.seg_start != nullptr && causal && causal_off == 0 && Tq == Tk && window <= 0,
                "prefix needs segs and causal self-attention without a window");
    same_device(q, *prefix);
    p.prefix = prefix->data_ptr<int>();
  }
  TORCH_CHECK(p.rope_cos == nullptr || D != 80, "RoPE on load: full-rotary head dims 64 / 128 only");
  p.rope_k = rope_k ? 1 : 0;
  if (given(q_rot)) {
    TORCH_CHECK(p.rope_cos != nullptr, "q_rot needs the rotary tables");
    check_bthd(*q_rot, q, "q_rot");
    TORCH_CHECK(q_rot->sizes() == q.sizes(), "q_rot shape");
    p.q_rot = bp(*q_rot);
    set_strides(*q_rot, p.qr_sb, p.qr_st, p.qr_sh);
  }
  const AttnFwdSwitches& sw = attn_fwd_switches();
  p.fwd_prio = sw.prio;
  p.fwd_sgpr = sw.sgpr;
  p.fwd_pro = sw.pro;
  p.fwd_ostage = sw.ostage;
  p.fwd_msub = sw.msub;
  const AttnFwdPlan plan = attn_fwd_plan(B, Hq, Hkv, Tq, Tk, static_cast<int>(D), causal, p.prefix != nullptr,
                                         device_cus(q.get_device()));
  check_grid(plan.grid, "forward");

  c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
  auto o = at::empty({B, Tq, Hq, D}, q.options());
  auto lse2 = at::empty({B, Hq, Tq}, q.options().dtype(at::kFloat));
  p.o = bp(o);
  p.lse2 = lse2.data_ptr<float>();
  set_strides(o, p.o_sb, p.o_st, p.o_sh);
  static const bool stamps = [] {
    const char* e = std::getenv("DLA_ATTN_STAMPS");
    return e != nullptr && std::atoi(e) == 1;
  }();
  if (stamps) {  // debug: read back with attn_stamps()
    auto& buf = attn_stamp_buffer();
    if (!buf.defined() || buf.device() != q.device())
      buf = at::zeros({1024 * 8 * 4}, q.options().dtype(at::kLong));
    p.stamps = reinterpret_cast<unsigned long long*>(buf.data_ptr<int64_t>());
  }
  launch_attn_fwd(p, plan, cur_stream(q));
  return {o, lse2};
}

// ================================= backward ===================================================
// dq / dk / dv are written into the given (possibly strided, e.g. fused-dqkv) bf16 outputs
void attn_bwd(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
              const at::Tensor& o, const at::Tensor& lse2, at::Tensor& dq, at::Tensor& dk, at::Tensor& dv,
              double scale, bool causal, int64_t causal_off, int64_t window, const OptT& kv_start,
              const OptT& kv_end, const OptT& segs, const OptT& rope_cos, const OptT& rope_sin,
              const OptT& rope_pos, bool rope_inputs) {
  check_bthd(dout, q, "dout");
  check_bthd(q, q, "q");
  check_bthd(k, q, "k");
  check_bthd(v, q, "v");
  check_bthd(o, q, "o");
  check_bthd(dq, q, "dq");
  check_bthd(dk, q, "dk");
  check_bthd(dv, q, "dv");
  check_f32(lse2, "lse2");
  same_device(q, lse2);
  const int64_t B = q.size(0), Tq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int64_t Tk = k.size(1), Hkv = k.size(2);
  TORCH_CHECK(D == 64 || D == 80 || D == 128, "head_dim must be 64, 80 or 128");
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() && dq.sizes() == q.sizes(),
              "dout/o/dq shape");
  TORCH_CHECK(k.size(0) == B && k.size(3) == D && v.sizes() == k.sizes(), "k/v shapes");
  TORCH_CHECK(dk.sizes() == k.sizes() && dv.sizes() == v.sizes(), "dk/dv shape");
  TORCH_CHECK(lse2.is_contiguous() && lse2.numel() == B * Hq * Tq, "lse2 shape");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "GQA ratio");
  AttnBwdParams p{};
  set_sizes(p, B, Hq, Hkv, Tq, Tk);
  p.q = cbp(q); p.k = cbp(k); p.v = cbp(v); p.dout = cbp(dout);
  p.lse2 = lse2.data_ptr<float>();
  p.dk = bp(dk); p.dv = bp(dv);
  set_strides(q, p.q_sb, p.q_st, p.q_sh);
  set_strides(k, p.k_sb, p.k_st, p.k_sh);
  set_strides(v, p.v_sb, p.v_st, p.v_sh);
  set_strides(dout, p.do_sb, p.do_st, p.do_sh);
  set_strides(dk, p.dk_sb, p.dk_st, p.dk_sh);
  set_strides(dv, p.dv_sb, p.dv_st, p.dv_sh);
  AttnBwdHostArgs h{};
  h.o = cbp(o);
  set_strides(o, h.o_sb, h.o_st, h.o_sh);
  h.dq = bp(dq);
  set_strides(dq, h.dq_sb, h.dq_st, h.dq_sh);
  p.scale = static_cast<float>(scale);
  p.scale2 = static_cast<float>(scale * 1.4426950408889634);
  p.causal_off = static_cast<int>(causal_off);
  p.window = static_cast<int>(window);
  // fused RoPE backward: dq / dk receive the un-rotated gradients; with rope_inputs (full rotary
  // only) q / k are also un-rotated and get rotated as they are staged
  p.rope_rot = set_mask_rope(p, p.seg_end, 1, true, q, Tk, causal, causal_off, kv_start, kv_end, segs, rope_cos,
                             rope_sin, rope_pos);
  TORCH_CHECK(!rope_inputs || p.rope_cos != nullptr, "rope_inputs needs the rotary tables");
  TORCH_CHECK(!rope_inputs || p.rope_rot == D, "rope_inputs (RoPE on load): full rotary only");
  p.rope_inputs = rope_inputs ? 1 : 0;
  const AttnBwdPlan plan = attn_bwd_plan(B, Hq, Hkv, Tq, Tk, static_cast<int>(D), causal, p.rope_cos != nullptr,
                                         p.rope_rot, device_cus(q.get_device()));
  check_grid(plan.delta_grid, "backward delta");
  check_grid(plan.grid, "backward");
  to_int(plan.slab_rows, "the dQ slab row count");

  c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
  auto fopt = q.options().dtype(at::kFloat);
  auto delta = at::empty({B, Hq, Tq}, fopt);
  // one dQ partial per key block (no zero fill: the reduce pass reads exactly the rows each key
  // block's workgroups wrote)
  auto slab = at::empty({std::max<int64_t>(plan.nkb, 1), B, plan.slab_rows, Hq, D}, plan.slab16 ? q.options() : fopt);
  at::Tensor dkp, dvp;
  if (plan.hsplit > 1) {
    dkp = at::empty({plan.hsplit, B, Tk, Hkv, D}, plan.part16 ? q.options() : fopt);
    dvp = at::empty({plan.hsplit, B, Tk, Hkv, D}, plan.part16 ? q.options() : fopt);
  }
  p.delta = delta.data_ptr<float>();
  p.dq_slab = plan.slab16 ? nullptr : slab.data_ptr<float>();
  p.dq_slab16 = plan.slab16 ? bp(slab) : nullptr;
  p.dk_part = plan.hsplit > 1 && !plan.part16 ? dkp.data_ptr<float>() : nullptr;
  p.dv_part = plan.hsplit > 1 && !plan.part16 ? dvp.data_ptr<float>() : nullptr;
  p.dk_part16 = plan.part16 ? bp(dkp) : nullptr;
  p.dv_part16 = plan.part16 ? bp(dvp) : nullptr;
  p.hsplit = plan.hsplit;
  p.slab_rows = static_cast<int>(plan.slab_rows);
  launch_attn_bwd(p, h, plan, cur_stream(q));
}

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("attn_fwd(Tensor q, Tensor k, Tensor v, float scale, bool causal, int causal_off, int window, Tensor? kv_start, Tensor? kv_end, Tensor? segs=None, Tensor? rope_cos=None, Tensor? rope_sin=None, Tensor? rope_pos=None, Tensor(a!)? q_rot=None, bool rope_k=True, Tensor? prefix=None) -> (Tensor, Tensor)");
  m.def("attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse2, Tensor(a!) dq, Tensor(b!) dk, Tensor(c!) dv, float scale, bool causal, int causal_off, int window, Tensor? kv_start, Tensor? kv_end, Tensor? segs=None, Tensor? rope_cos=None, Tensor? rope_sin=None, Tensor? rope_pos=None, bool rope_inputs=False) -> ()");
  m.def("attn_stamps(Tensor like) -> Tensor");
  m.def("attn_fwd_switch(str name, int value) -> int", &dla::attn_fwd_switch);
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("attn_fwd", &dla::attn_fwd);
  m.impl("attn_bwd", &dla::attn_bwd);
  m.impl("attn_stamps", &dla::attn_stamps);
}
