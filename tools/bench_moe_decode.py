"""The MoE block alone at Mixtral's shape (H 4096, F 14336, E 8, k 2): the grouped chain
(expert_positions .. combine) against the two decode kernels of csrc/moe_decode.hip, interleaved in
one process on the same tensors, weights rotated over three 2.8 GB sets between calls. Prints one
JSON line per row count: medians (and min / max) of per-call device-event times in microseconds
and the routed experts' weight bytes over them in TB/s.

    python tools/bench_moe_decode.py [rows ...]      (default 1 8 64)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_alignment_amd import ops  # noqa: E402
from distributed_llm_alignment_amd.ops import _ext  # noqa: E402

DEV = torch.device("cuda", 0)
H, Fd, E, K = 4096, 14336, 8, 2
NSETS, ROUNDS = 3, 7


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return out, (a, b)


def main():
    C = _ext.require()
    g = torch.Generator(device=DEV).manual_seed(0)
    sets = []
    for _ in range(NSETS):
        wu = torch.empty(E, 2 * Fd, H, device=DEV, dtype=torch.bfloat16).normal_(0, H ** -0.5, generator=g)
        wd = torch.empty(E, H, Fd, device=DEV, dtype=torch.bfloat16).normal_(0, Fd ** -0.5, generator=g)
        sets.append((wu, wd))
    for B in [int(x) for x in (sys.argv[1:] or ['1', '8', '64'])]:
        h2 = torch.randn(B, H, device=DEV, generator=g).to(torch.bfloat16)
        logits = torch.randn(B, E, device=DEV, generator=g).to(torch.bfloat16)
        topv, topi = ops.moe.route_topk(logits, K)
        routed = int(topi.unique().numel())
        wbytes = routed * 3 * Fd * H * 2

        def old(wu, wd):
            pos, counts = ops.moe.expert_positions(topi, E)
            xs = ops.moe.dispatch(h2, pos)
            ys = ops.moe.experts_swiglu(xs, wu, wd, counts)
            return ops.moe.combine(ys, pos, topv, permutation=True)

        ev = {"old": [], "new": [], "glu": [], "down": []}
        with torch.no_grad():
            for wu, wd in sets:  # warm both arms on every set
                o = old(wu, wd)
                n = C.moe_decode_down(C.moe_decode_glu(h2, topi, wu), topv, topi, wd)
            torch.cuda.synchronize()
            rel = ((n.float() - o.float()).norm() / o.float().norm()).item()
            for _ in range(ROUNDS):
                for wu, wd in sets:
                    _, e = timed(lambda: old(wu, wd))
                    ev["old"].append(e)
                for wu, wd in sets:
                    a, e1 = timed(lambda: C.moe_decode_glu(h2, topi, wu))
                    _, e2 = timed(lambda: C.moe_decode_down(a, topv, topi, wd))
                    ev["glu"].append(e1)
                    ev["down"].append(e2)
                    ev["new"].append((e1[0], e2[1]))
            torch.cuda.synchronize()
        us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ev.items()}
        row = {"B": B, "routed_experts": routed, "weight_GB": round(wbytes / 1e9, 3), "rel_new_vs_old": rel}
        for k, v in us.items():
            row[k + "_us"] = round(statistics.median(v), 1)
            row[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
        row["old_TBps"] = round(wbytes / (row["old_us"] * 1e-6) / 1e12, 3)
        row["new_TBps"] = round(wbytes / (row["new_us"] * 1e-6) / 1e12, 3)
        row["glu_TBps"] = round(wbytes * 2 / 3 / (row["glu_us"] * 1e-6) / 1e12, 3)
        row["down_TBps"] = round(wbytes / 3 / (row["down_us"] * 1e-6) / 1e12, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
