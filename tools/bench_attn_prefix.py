#!/usr/bin/env python
"""Prefix-shared attention against the plain [S, T] grid it replaces (profiles/share_prefix_update.md).

One GRPO group of G rollouts (prompt P, n generated tokens) is G rows of T = P + n tokens in the
plain run and one packed row of L = P - 1 + G (n + 1) slots with `prefix=` (models.transformer.
shared_prefix_pack). Forward and forward + backward of `ops.attention_core` are timed with CUDA
events, the two arms interleaved round by round, medians reported. Also printed: the share of the
backward's (key block, 32-query tile) sweeps that are inactive in the packed layout (a key block
still loads Q / dO for every tile from its diagonal to the row end).

    python tools/bench_attn_prefix.py --groups 1 --group 8 --prompt 512 --new 256
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def swept_inactive_share(segs: torch.Tensor, L: int) -> float:
    """Share of the backward's (256-key block, 32-query tile) pairs swept (tile at or past the
    block's first key) in which no (query, key) pair is visible (j <= i < seg_end[j])."""
    se = segs[1, 0].long().cpu()
    swept = dead = 0
    for k0 in range(0, L, 256):
        keys = torch.arange(k0, min(k0 + 256, L))
        for q0 in range(k0 // 32 * 32, L, 32):
            qs = torch.arange(q0, min(q0 + 32, L))
            vis = (keys.view(1, -1) <= qs.view(-1, 1)) & (qs.view(-1, 1) < se[keys].view(1, -1))
            swept += 1
            dead += int(not vis.any())
    return dead / max(swept, 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--heads", type=int, nargs=2, default=(32, 8))
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from distributed_llm_alignment_amd import ops
    from distributed_llm_alignment_amd.models.transformer import shared_prefix_pack
    from distributed_llm_alignment_amd.ops import _ext

    _ext.require()
    dev = torch.device("cuda", 0)
    G, P, T = a.group, a.prompt, a.prompt + a.new
    S = a.groups * G
    Hq, Hkv = a.heads
    D = a.head_dim
    seqs = torch.zeros(S, T, dtype=torch.long, device=dev)
    _, _, segs, prefix, _ = shared_prefix_pack(seqs, None, P, G)
    L = segs.shape[2]
    gen = torch.Generator(device=dev).manual_seed(0)
    mk = lambda b, t, h: torch.randn(b, t, h, D, device=dev, dtype=torch.bfloat16, generator=gen).requires_grad_()
    arms = {"plain": (mk(S, T, Hq), mk(S, T, Hkv), mk(S, T, Hkv), {}),
            "prefix": (mk(a.groups, L, Hq), mk(a.groups, L, Hkv), mk(a.groups, L, Hkv), {"segs": segs, "prefix": prefix})}
    dos = {k: torch.randn_like(v[0]) for k, v in arms.items()}

    def fwd(name):
        q, k, v, kw = arms[name]
        with torch.no_grad():
            ops.attention_core(q, k, v, causal=True, **kw)

    def fwdbwd(name):
        q, k, v, kw = arms[name]
        o = ops.attention_core(q, k, v, causal=True, **kw)
        torch.autograd.grad(o, [q, k, v], dos[name])

    def timed(fn, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(name)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters  # us

    res = {f"{n}_{p}": [] for n in arms for p in ("fwd", "fwdbwd")}
    for r in range(a.rounds + 1):  # round 0 warms up
        for n in arms:
            for p, fn in (("fwd", fwd), ("fwdbwd", fwdbwd)):
                t = timed(fn, n)
                if r:
                    res[f"{n}_{p}"].append(t)
    out = {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
           for k, v in res.items()}
    print(json.dumps({"bench": "attn_prefix", "groups": a.groups, "group": G, "prompt": P, "new": a.new,
                      "plain_shape": [S, T], "packed_shape": [a.groups, L], "token_ratio": round(a.groups * L / (S * T), 4),
                      "heads": [Hq, Hkv], "head_dim": D,
                      "bwd_swept_inactive_share": round(swept_inactive_share(segs, L), 4), **out}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
