"""Per-layer decode attention over the e4m3 KV cache against the bf16 cache (Llama-3-8B heads):
the fp8 arm is the quantising prologue + decode_attn_f8 (two launches), the bf16 arm the default
fused rope + attention op, each timed from a captured hipGraph of 50 calls, alternating, in one
process. One JSON line per (B, kv_len) with the bytes each arm streams.

    python tools/bench_kv_fp8.py [--shapes 8x768,64x768,8x4352]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x768,64x768,8x4352", help="BxL pairs")
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    a = ap.parse_args()
    from decode_attn_bench import _time_graph
    from distributed_llm_alignment_amd.ops import RotaryCache, _ext, decode

    C = _ext.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Hq, Hkv, D = a.Hq, a.Hkv, a.D
    for shape in a.shapes.split(","):
        B, L = (int(x) for x in shape.split("x"))
        Tmax = L + 1
        cos, sin = RotaryCache(D, 500000.0, Tmax + 8, None).tables(dev)
        # head-major storage behind the [B, Tmax, Hkv, D] view, as KVCache allocates it
        kc = torch.randn(B, Hkv, Tmax, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
        vc = torch.randn(B, Hkv, Tmax, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
        k8, v8 = (torch.empty(B, Hkv, Tmax, D, device=dev, dtype=torch.uint8).transpose(1, 2) for _ in range(2))
        ks, vs = (torch.empty(B, Hkv, Tmax, device=dev).transpose(1, 2) for _ in range(2))
        decode.kv_quant_f8(kc, k8, ks, 0)
        decode.kv_quant_f8(vc, v8, vs, 0)
        qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
        pos = torch.full((B,), L - 1, device=dev, dtype=torch.int32)
        slot = torch.tensor([L - 1], device=dev, dtype=torch.long)
        kv_len = torch.tensor([L], device=dev, dtype=torch.int32)

        def bf16():
            return C.decode_attn_rope(qkv, cos, sin, pos, kc, vc, slot, kv_len, None, 0, D ** -0.5, Hq, Hkv, D, D)

        def fp8():
            q = C.rope_cache_write_f8(qkv, cos, sin, pos, k8, v8, ks, vs, slot, Hq, Hkv, D, D)
            return C.decode_attn_f8(q, k8, v8, ks, vs, kv_len, None, 0, D ** -0.5)

        def fp8_attn_only():
            return C.decode_attn_f8(qkv[:, 0, :Hq * D].view(B, Hq, D), k8, v8, ks, vs, kv_len, None, 0, D ** -0.5)

        diff = (bf16().float() - fp8().float()).abs().max().item()
        arms = {"bf16": _time_graph(bf16), "fp8": _time_graph(fp8), "fp8_attn_only": _time_graph(fp8_attn_only)}
        us = {k: [] for k in arms}
        for _ in range(3):  # alternate the arms (best of 5 replays each time)
            for k, run in arms.items():
                us[k].append(round(run() * 1e3, 2))
        mb16 = 2 * B * L * Hkv * D * 2 / 1e6
        mb8 = 2 * B * L * Hkv * (D + 4) / 1e6
        print(json.dumps({"B": B, "kv_len": L, "us": us, "bf16_MB": round(mb16, 1), "fp8_MB": round(mb8, 1),
                          "bf16_TB_s": round(mb16 / 1e6 / (min(us["bf16"]) * 1e-6), 2),
                          "fp8_attn_TB_s": round(mb8 / 1e6 / (min(us["fp8_attn_only"]) * 1e-6), 2),
                          "max_abs_diff_vs_bf16_cache": diff}), flush=True)


if __name__ == "__main__":
    main()
