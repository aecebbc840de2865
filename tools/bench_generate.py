#!/usr/bin/env python
"""Rollout-generation throughput (the RLHF / teacher-generation hot loop):
prefill B prompts of length T, then decode N tokens, eager per-op loop vs the captured-hipGraph
decode step. Prints one JSON line per mode.

    python tools/bench_generate.py --model llama3-8b --batch 8 --prompt 1024 --new 256
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--modes", default="eager,graph")
    ap.add_argument("--weight-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="decode weight streams (generate(weight_dtype=...))")
    ap.add_argument("--group", type=int, default=1,
                    help="samples per prompt (generate(num_return_sequences=G)); --batch counts prompts")
    ap.add_argument("--group-attention", type=int, choices=(0, 1), default=0,
                    help="decode attention reads a group's prompt K/V once (generate(group_attention=...))")
    ap.add_argument("--logprobs", type=int, choices=(0, 1, 2, 3), default=0,
                    help="also return the sampler's token log-probs (generate(return_logprobs=...)): 1 at "
                         "temperature 1, 2 at the draw temperature (logprob_temperature=0.7), 3 the kept-set "
                         "log-probs and the sampling mask (return_keep_mask=True)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from distributed_llm_alignment_amd.models import build_model, generate, get_config
    from distributed_llm_alignment_amd.ops import _ext, decode
    from distributed_llm_alignment_amd.utils.tuning import enable_gemm_tuning

    dev = torch.device("cuda", 0)
    _ext.require()
    enable_gemm_tuning(0)
    cfg = get_config(a.model)
    m = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=0)
    g = torch.Generator(device=dev).manual_seed(0)
    ids = torch.randint(3, cfg.vocab_size, (a.batch, a.prompt), device=dev, generator=g)
    am = torch.ones_like(ids)
    # the sampler op alone at the decode step's shape, for its share of a token
    lg = torch.randn((a.batch * a.group, cfg.vocab_size), device=dev, generator=g).mul_(3).to(torch.bfloat16)
    rng = torch.tensor([1, 0], dtype=torch.long, device=dev)
    op = (decode.sample_tokens, decode.sample_tokens_logp, getattr(decode, "sample_tokens_logp_tempered", None),
          getattr(decode, "sample_tokens_keep", None))[a.logprobs]
    for _ in range(5):
        op(lg, 0.7, 0, 0.9, False, rng)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(50):
        op(lg, 0.7, 0, 0.9, False, rng)
    ev[1].record()
    torch.cuda.synchronize()
    sampler_ms = ev[0].elapsed_time(ev[1]) / 50
    for mode in a.modes.split(","):
        kw = dict(max_new_tokens=a.new, do_sample=True, temperature=0.7, top_p=0.9, eos_token_id=-1,
                  use_graph=(mode == "graph"), seed=1, weight_dtype=a.weight_dtype,
                  num_return_sequences=a.group, group_attention=bool(a.group_attention))
        if a.logprobs:  # (left out otherwise: the call an older build of the package takes)
            kw["return_logprobs"] = True
        if a.logprobs >= 2:
            kw["logprob_temperature"] = 0.7
        if a.logprobs == 3:
            kw["return_keep_mask"] = True
        generate(m, ids[:, :64], am[:, :64], **{**kw, "max_new_tokens": 8})  # warm
        generate(m, ids, am, **kw)  # warm at the timed shapes (graph mode: the capture is reused)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = generate(m, ids, am, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = out[0] if a.logprobs else out
        n = out.shape[1] - a.prompt
        # prefill alone, for the per-token decode latency
        t1 = time.perf_counter()
        generate(m, ids, am, **{**kw, "max_new_tokens": 1})
        torch.cuda.synchronize()
        tp = time.perf_counter() - t1
        print(json.dumps({"mode": mode, "model": cfg.name, "batch": a.batch, "prompt": a.prompt,
                          "weight_dtype": a.weight_dtype, "group": a.group,
                          "group_attention": bool(a.group_attention), "logprobs": bool(a.logprobs),
                          "logprob_temperature": 0.7 if a.logprobs >= 2 else 1.0,
                          "keep_mask": a.logprobs == 3,
                          "sampler_ms": round(sampler_ms, 4),
                          "new_tokens": n, "total_s": round(dt, 3), "prefill_s": round(tp, 3),
                          "decode_ms_per_token": round((dt - tp) / max(n - 1, 1) * 1e3, 3),
                          "decode_tokens_per_s": round(a.batch * a.group * (n - 1) / max(dt - tp, 1e-9), 1)}),
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
