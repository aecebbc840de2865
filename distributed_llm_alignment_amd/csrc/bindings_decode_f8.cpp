// Torch ops of the e4m3 KV cache (csrc/decode_f8.hip): kv_quant_f8, rope_cache_write_f8,
// decode_attn_f8. Host-only: argument checks, output allocation, launch on the current stream.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "bind_util.h"
#include "decode_f8_params.h"

namespace dla {

// One layer's cache: codes uint8 [B, Tmax, Hkv, D] (D contiguous, 16-byte aligned rows), scales
// fp32 [B, Tmax, Hkv]; K and V share strides (any layout behind the view)
static KvF8 check_kv_f8(const at::Tensor& k8, const at::Tensor& v8, const at::Tensor& ks, const at::Tensor& vs,
                        int64_t B, int64_t Hkv, int64_t D) {
  check_cuda(k8, "k8");
  check_cuda(v8, "v8");
  check_f32(ks, "k_scale");
  check_f32(vs, "v_scale");
  TORCH_CHECK(k8.scalar_type() == at::kByte && v8.scalar_type() == at::kByte, "k8 / v8 must be uint8 e4m3 codes");
  TORCH_CHECK(D == 64 || D == 128, "the e4m3 KV cache supports head_dim 64 or 128");
  TORCH_CHECK(k8.dim() == 4 && k8.size(0) == B && k8.size(2) == Hkv && k8.size(3) == D &&
                  k8.sizes() == v8.sizes() && k8.strides() == v8.strides() && k8.stride(3) == 1,
              "codes [B, Tmax, Hkv, D]: cache batch / head dim, k8 / v8 must share strides");
  TORCH_CHECK(k8.stride(0) % 16 == 0 && k8.stride(1) % 16 == 0 && k8.stride(2) % 16 == 0, "16-byte aligned code rows");
  check_aligned16(k8, "k8");
  check_aligned16(v8, "v8");
  TORCH_CHECK(ks.dim() == 3 && ks.size(0) == B && ks.size(1) == k8.size(1) && ks.size(2) == Hkv &&
                  ks.sizes() == vs.sizes() && ks.strides() == vs.strides(),
              "scales [B, Tmax, Hkv], k_scale / v_scale must share strides");
  TORCH_CHECK(k8.size(1) >= 1, "empty cache");
  same_device(k8, v8);
  same_device(k8, ks);
  same_device(k8, vs);
  KvF8 c;
  c.k8 = k8.data_ptr<uint8_t>();
  c.v8 = v8.data_ptr<uint8_t>();
  c.c_sb = k8.stride(0), c.c_st = k8.stride(1), c.c_sh = k8.stride(2);
  c.ks = ks.data_ptr<float>();
  c.vs = vs.data_ptr<float>();
  c.z_sb = ks.stride(0), c.z_st = ks.stride(1), c.z_sh = ks.stride(2);
  c.Tmax = static_cast<int>(k8.size(1));
  return c;
}

// src [B, T, Hkv, D] bf16 (a layer's rotated prompt K, or V) -> tokens [t0, t0 + T) of dst_codes
// uint8 [B, Tmax, Hkv, D] and dst_scale fp32 [B, Tmax, Hkv]
void kv_quant_f8(const at::Tensor& src, at::Tensor& dst_codes, at::Tensor& dst_scale, int64_t t0) {
  check_bf16(src, "src");
  TORCH_CHECK(src.dim() == 4 && src.stride(3) == 1, "src [B, T, Hkv, D] with the head dim contiguous");
  const int64_t B = src.size(0), T = src.size(1), Hkv = src.size(2), D = src.size(3);
  const KvF8 c = check_kv_f8(dst_codes, dst_codes, dst_scale, dst_scale, B, Hkv, D);
  TORCH_CHECK(t0 >= 0 && t0 + T <= c.Tmax, "tokens [t0, t0 + T) must lie inside the cache");
  TORCH_CHECK(src.stride(0) % 8 == 0 && src.stride(1) % 8 == 0 && src.stride(2) % 8 == 0, "16-byte aligned src rows");
  check_aligned16(src, "src");
  same_device(src, dst_codes);
  c10::hip::HIPGuardMasqueradingAsCUDA g(src.device());
  KvQuantParams p{};
  p.src = cbp(src);
  p.s_sb = src.stride(0), p.s_st = src.stride(1), p.s_sh = src.stride(2);
  p.codes = c.k8;
  p.c_sb = c.c_sb, p.c_st = c.c_st, p.c_sh = c.c_sh;
  p.scale = c.ks;
  p.z_sb = c.z_sb, p.z_st = c.z_st, p.z_sh = c.z_sh;
  p.B = static_cast<int>(B), p.T = static_cast<int>(T), p.Hkv = static_cast<int>(Hkv), p.D = static_cast<int>(D);
  p.t0 = static_cast<int>(t0);
  launch_kv_quant_f8(p, cur_stream(src));
}

// rope_cache_write with a quantising write: qkv [B, 1, (Hq + 2 Hkv) D] of the newest token ->
// rotated q [B, Hq, D] (bitwise rope_cache_write's); rotated k / plain v as codes + scales into
// row `slot` (int64 [1] on the device) of the caches
at::Tensor rope_cache_write_f8(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin,
                               const at::Tensor& pos, at::Tensor& k8, at::Tensor& v8, at::Tensor& k_scale,
                               at::Tensor& v_scale, const at::Tensor& slot, int64_t Hq, int64_t Hkv, int64_t D,
                               int64_t rot) {
  check_bf16(qkv, "qkv");
  check_f32(cos, "cos");
  check_f32(sin, "sin");
  check_i32(pos, "pos");
  check_cuda(slot, "slot");
  TORCH_CHECK(slot.scalar_type() == at::kLong && slot.numel() >= 1, "slot int64");
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(1) == 1 && qkv.size(2) == (Hq + 2 * Hkv) * D && qkv.stride(2) == 1 &&
                  qkv.stride(0) % 8 == 0,
              "qkv [B, 1, (Hq+2Hkv)D] with 16-byte aligned rows");
  TORCH_CHECK(rot >= 0 && rot % 16 == 0 && rot <= D, "rot % 16 == 0, rot <= D");
  TORCH_CHECK(cos.is_contiguous() && sin.is_contiguous() && cos.size(-1) == rot / 2 && sin.sizes() == cos.sizes(),
              "rope tables");
  TORCH_CHECK(pos.numel() == qkv.size(0) && pos.is_contiguous(), "pos [B]");
  check_aligned16(qkv, "qkv");
  const int64_t B = qkv.size(0);
  const KvF8 c = check_kv_f8(k8, v8, k_scale, v_scale, B, Hkv, D);
  same_device(qkv, k8);
  c10::hip::HIPGuardMasqueradingAsCUDA g(qkv.device());
  auto q = at::empty({B, Hq, D}, qkv.options());
  RopeCacheF8Params p{};
  p.qkv = cbp(qkv);
  p.ld = qkv.stride(0);
  p.q_out = bp(q);
  p.c = c;
  p.slot = slot.data_ptr<int64_t>();
  p.cos_t = cos.data_ptr<float>();
  p.sin_t = sin.data_ptr<float>();
  p.pos = pos.data_ptr<int>();
  p.B = static_cast<int>(B), p.Hq = static_cast<int>(Hq), p.Hkv = static_cast<int>(Hkv);
  p.D = static_cast<int>(D), p.rot = static_cast<int>(rot);
  launch_rope_cache_f8(p, cur_stream(qkv));
  return q;
}

// q [B, Hq, D] already rotated, the newest token already in the caches; keys [kv_start, kv_len)
at::Tensor decode_attn_f8(const at::Tensor& q, const at::Tensor& k8, const at::Tensor& v8,
                          const at::Tensor& k_scale, const at::Tensor& v_scale, const at::Tensor& kv_len,
                          const c10::optional<at::Tensor>& kv_start, int64_t window, double scale) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 3 && q.stride(2) == 1 && q.stride(0) % 8 == 0 && q.stride(1) % 8 == 0,
              "q [B, Hq, D] with 16-byte aligned rows");
  check_aligned16(q, "q");
  TORCH_CHECK(k8.dim() == 4, "codes [B, Tmax, Hkv, D]");
  const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2), Hkv = k8.size(2);
  const KvF8 c = check_kv_f8(k8, v8, k_scale, v_scale, B, Hkv, D);
  same_device(q, k8);
  check_i32(kv_len, "kv_len");
  TORCH_CHECK(kv_len.numel() >= 1, "kv_len");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, "Hq % Hkv");
  const int64_t GQ = Hq / Hkv;
  TORCH_CHECK(GQ == 1 || GQ == 2 || GQ == 4 || GQ == 8, "GQA group size must be 1, 2, 4 or 8");
  DecodeF8Params p{};
  if (kv_start && kv_start->defined()) {
    check_i32(*kv_start, "kv_start");
    TORCH_CHECK(kv_start->numel() == B && kv_start->is_contiguous(), "kv_start [B]");
    p.kv_start = kv_start->data_ptr<int>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
  p.q = cbp(q);
  p.q_sb = q.stride(0), p.q_sh = q.stride(1);
  p.c = c;
  p.kv_len = kv_len.data_ptr<int>();
  p.window = static_cast<int>(window);
  p.scale_log2 = static_cast<float>(scale * 1.4426950408889634);
  p.B = static_cast<int>(B), p.Hq = static_cast<int>(Hq), p.Hkv = static_cast<int>(Hkv), p.D = static_cast<int>(D);
  const int nsplit = decode_f8_splits(p);
  auto fopt = q.options().dtype(at::kFloat);
  auto part_o = at::empty({B, Hq, nsplit, D}, fopt);
  auto part_ml = at::empty({B, Hq, nsplit, 2}, fopt);
  auto out = at::empty({B, Hq, D}, q.options());
  p.part_o = part_o.data_ptr<float>();
  p.part_ml = part_ml.data_ptr<float>();
  p.out = bp(out);
  p.o_sb = out.stride(0), p.o_sh = out.stride(1);
  launch_decode_f8(p, cur_stream(q));
  return out;
}

}  // namespace dla

TORCH_LIBRARY_FRAGMENT(dla, m) {
  m.def("kv_quant_f8(Tensor src, Tensor(a!) dst_codes, Tensor(b!) dst_scale, int t0) -> ()");
  m.def("rope_cache_write_f8(Tensor qkv, Tensor cos, Tensor sin, Tensor pos, Tensor(a!) k8, Tensor(b!) v8, Tensor(c!) k_scale, Tensor(d!) v_scale, Tensor slot, int Hq, int Hkv, int D, int rot) -> Tensor");
  m.def("decode_attn_f8(Tensor q, Tensor k8, Tensor v8, Tensor k_scale, Tensor v_scale, Tensor kv_len, Tensor? kv_start, int window, float scale) -> Tensor");
}

TORCH_LIBRARY_IMPL(dla, CUDA, m) {
  m.impl("kv_quant_f8", &dla::kv_quant_f8);
  m.impl("rope_cache_write_f8", &dla::rope_cache_write_f8);
  m.impl("decode_attn_f8", &dla::decode_attn_f8);
}
