"""Decode-attention microbenchmark (Llama-3-8B heads, B=8): fused rope + split-KV attention +
combine per call, timed from a captured hipGraph of 50 calls (no host launch cost), for several
cache lengths, both kernel versions (DLA_DECODE_ATTN_V1 is read once per process: run twice).

    python tools/decode_attn_bench.py [--lens 128,512,1152,4096]

`--group G --prefix Tp`: a group-structured batch (rows p*G .. p*G+G-1 share keys [0, Tp)); each
length is timed with the per-row op and with the grouped op (`decode_attn_rope_group`) in this
process, alternating, and one JSON line per length reports both with the bytes each arm needs.

    python tools/decode_attn_bench.py --B 64 --group 8 --prefix 512 --lens 513,640,768"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_graph(call, reps=5, n=50):
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            call()
    graph.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        best = 1e9
        for _ in range(reps):
            s.record()
            graph.replay()
            e.record()
            torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / n)
        return best

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", default="128,512,1152,4096")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--headmajor", type=int, default=0, help="cache stored [B, Hkv, Tmax, D]")
    ap.add_argument("--group", type=int, default=1, help="rows per prompt (with --prefix)")
    ap.add_argument("--prefix", type=int, default=0, help="shared prefix length Tp of every group")
    ap.add_argument("--tmax", type=int, default=0, help="cache capacity (default: the length + 1)")
    a = ap.parse_args()
    from distributed_llm_alignment_amd.ops import RotaryCache, _ext

    C = _ext.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    B, Hq, Hkv, D = a.B, a.Hq, a.Hkv, a.D
    G, Tp = a.group, a.prefix
    for L in [int(x) for x in a.lens.split(",")]:
        Tmax = a.tmax if a.tmax else L + 1
        rope = RotaryCache(D, 500000.0, Tmax + 8, None)
        cos, sin = rope.tables(dev)
        if a.headmajor:  # same logical [B, Tmax, Hkv, D] tensor, head-major storage
            kc = torch.randn(B, Hkv, Tmax, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
            vc = torch.randn(B, Hkv, Tmax, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
        else:
            kc = torch.randn(B, Tmax, Hkv, D, device=dev, generator=g).to(torch.bfloat16)
            vc = torch.randn(B, Tmax, Hkv, D, device=dev, generator=g).to(torch.bfloat16)
        if G > 1:  # the group's rows share the prefix
            first = (torch.arange(B, device=dev) // G) * G
            kc[:, :Tp] = kc[first, :Tp]
            vc[:, :Tp] = vc[first, :Tp]
        qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
        pos = torch.full((B,), L - 1, device=dev, dtype=torch.int32)
        slot = torch.tensor([L - 1], device=dev, dtype=torch.long)
        kv_len = torch.tensor([L], device=dev, dtype=torch.int32)

        def call():
            return C.decode_attn_rope(qkv, cos, sin, pos, kc, vc, slot, kv_len, None, 0, D ** -0.5,
                                      Hq, Hkv, D, D)

        def call_group():
            return C.decode_attn_rope_group(qkv, cos, sin, pos, kc, vc, slot, kv_len, None, 0, D ** -0.5,
                                            Hq, Hkv, D, D, G, Tp)

        row = _time_graph(call)
        mb = 2 * B * L * Hkv * D * 2 / 1e6
        if G <= 1:
            best = row()
            print(json.dumps({"kv_len": L, "us": round(best * 1e3, 2), "kv_MB": round(mb, 1),
                              "TB_s": round(mb / 1e6 / (best * 1e-3), 2),
                              "v1": os.environ.get("DLA_DECODE_ATTN_V1", "0"),
                              "headmajor": a.headmajor}), flush=True)
            continue
        diff = (call().float() - call_group().float()).abs().max().item()
        grp = _time_graph(call_group)
        # alternate the arms: per-row, grouped, per-row, grouped (best of 5 replays each time)
        t_row, t_grp = [], []
        for _ in range(2):
            t_row.append(row())
            t_grp.append(grp())
        # the bytes the grouped arm needs: the prefix once per prompt, the suffix per row
        mbg = 2 * ((B // G) * Tp + B * (L - Tp)) * Hkv * D * 2 / 1e6
        print(json.dumps({"kv_len": L, "B": B, "group": G, "prefix": Tp, "tmax": Tmax,
                          "row_us": [round(t * 1e3, 2) for t in t_row],
                          "group_us": [round(t * 1e3, 2) for t in t_grp],
                          "row_MB": round(mb, 1), "group_MB": round(mbg, 1),
                          "row_TB_s": round(mb / 1e6 / (min(t_row) * 1e-3), 2),
                          "group_TB_s": round(mbg / 1e6 / (min(t_grp) * 1e-3), 2),
                          "max_abs_diff": diff, "headmajor": a.headmajor}), flush=True)


if __name__ == "__main__":
    main()
