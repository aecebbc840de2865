"""LoRA measurements on one MI355X (results: profiles/lora.md). Needs a GPU: no CPU fallback.

    python tools/bench_lora.py kernels [--rounds 7] [--iters 20]
    python tools/bench_lora.py step --mode full|lora|lora-shared [--steps 5] [--warmup 2]
    python tools/bench_lora.py refresh [--rounds 7] [--iters 10]          (results: profiles/lora_rollout.md)
    python tools/bench_lora.py decode [--rows 8 64] [--rounds 5]           (likewise)

kernels: lora_shrink and lora_expand_add_ against the torch composition of the same step
(the library GEMMs with the rounding of the formula of record, `ops.lora.shrink_library` = mm with
fp32 output, scale, one rounding, and `addmm_` for the expand: what an eligible call outside the
kernels' default gates runs) and against the fp32 composition of record that serves ineligible
calls, at the Llama-3-8B projection shapes (M = 8192; K = 4096 with N in {6144, 4096, 28672}, and
K = 14336 with N = 4096; r in {16, 32, 64}).
The arms alternate inside one process, `rounds` timed windows of `iters` launches each between
device events; the table gives the median and the min..max spread of the per-launch time, and the
achieved bytes/s of each kernel's minimal traffic (x read once for the shrink; y read and written
once for the expand). Inputs are uniform random (never zeros).

step: Llama-3-8B DPO at the headline shape (16 pairs x 1024 per optimizer step: 4 micro-batches
of 4 pairs, one GPU, ZeRO-1 engine as bench.py). `full` = full fine-tuning with a separate
reference (the default trainer), `lora` = r = 16 adapters (`--r`) with a separate reference model,
`lora-shared` = adapters with the reference taken from the policy (LoRAReference). Prints pairs/s
per step with its spread and the peak allocated memory. One mode per process: a fresh allocator.

refresh: building one decode weight copy from W + s B A at Llama-3-8B's four projections (qkv
6144 x 4096 and gate|up 28672 x 4096 with the norm weight folded, o 4096 x 4096, down 4096 x 14336),
r in {16, 64}, bf16 tiled and e4m3 tiled: (a) the one-pass op (`lora_tile_weight` /
`lora_quant_tile_f8`, its A^T copy included), (b) the three-launch composition on the same tensors
(clone, `lora_expand_add_(transposed=True)`, the existing `tile_weight` / `quant_tile_f8`), (c) the
existing op on W alone, the floor: a refresh without adapters. Interleaved rounds as `kernels`.

decode: graph decode ms/token of `generate(adapters="merged")` against the same model under
`lora_disabled` (the adapter-free kernels), from the difference of two generation lengths so the
prefill cancels; interleaved rounds, median and spread.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

KERNEL_SHAPES = [(8192, 4096, 6144), (8192, 4096, 4096), (8192, 4096, 28672), (8192, 14336, 4096)]
RANKS = (16, 32, 64)


def _need_gpu():
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py measures on the GPU; none is visible")
    from distributed_llm_alignment_amd.ops import _ext

    _ext.require()
    return torch.device("cuda", 0)


def _rand(shape, dev, gen, amp=1.0):
    return ((torch.rand(shape, generator=gen, device=dev, dtype=torch.float32) * 2 - 1) * amp).to(torch.bfloat16)


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per launch


def _ab(arms, rounds, iters):
    """Interleaved rounds of every arm; {name: [us per launch per round]}."""
    for fn in arms.values():  # warm every shape: code objects, library algorithm picks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            out[k].append(_timed(fn, iters))
    return out


def _fmt(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):.1f}..{max(ts):.1f})"


def bench_kernels(args):
    dev = _need_gpu()
    from distributed_llm_alignment_amd.ops import lora as L

    k = torch.ops.dla
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    print("| op | M | K | N | r | kernel us (min..max) | library us (min..max) | kernel / library | "
          "fp32 composition of record us | kernel GB/s of minimal traffic |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    done_shrink = set()
    for M, K, N in KERNEL_SHAPES:
        for r in RANKS:
            x = _rand((M, K), dev, gen)
            a = _rand((r, K), dev, gen, K ** -0.5)
            b = _rand((N, r), dev, gen, r ** -0.5)
            t = k.lora_shrink(x, a, 2.0)
            if (M, K, r) not in done_shrink:
                done_shrink.add((M, K, r))
                res = _ab({"kernel": lambda: k.lora_shrink(x, a, 2.0),
                           "comp": lambda: L.shrink_library(x, a, 2.0),
                           "record": lambda: L.shrink_composition(x, a, 2.0)}, args.rounds, args.iters)
                rows.append(("shrink", M, K, "-", r, res, M * K * 2))
            y = _rand((M, N), dev, gen)
            bt = b.t()
            res = _ab({"kernel": lambda: k.lora_expand_add_(y, t, b, 1.0, False),
                       "comp": lambda: y.addmm_(t, bt),
                       "record": lambda: y.copy_(L.expand_add_composition(y, t, b))}, args.rounds, args.iters)
            rows.append(("expand", M, "-", N, r, res, 2 * M * N * 2))
            btc = bt.contiguous()  # [r, N]
            res = _ab({"kernel": lambda: k.lora_expand_add_(y, t, btc, 1.0, True),
                       "comp": lambda: y.addmm_(t, bt)}, args.rounds, args.iters)
            rows.append(("expand [r,N]", M, "-", N, r, res, 2 * M * N * 2))
            del x, y
    for op, M, K, N, r, res, nbytes in rows:
        km, cm = statistics.median(res["kernel"]), statistics.median(res["comp"])
        rec = _fmt(res["record"]) if "record" in res else "-"
        print(f"| {op} | {M} | {K} | {N} | {r} | {_fmt(res['kernel'])} | {_fmt(res['comp'])} | {km / cm:.2f} | "
              f"{rec} | {nbytes / km / 1e3:.0f} |")
    print(json.dumps({"bench": "lora_kernels", "rows": [
        {"op": op, "M": M, "K": K, "N": N, "r": r, "kernel_us": res["kernel"], "comp_us": res["comp"],
         "record_us": res.get("record")}
        for op, M, K, N, r, res, _ in rows]}))


def bench_step(args):
    dev = _need_gpu()
    from distributed_llm_alignment_amd.data.synthetic import synthetic_preference_batch
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.models.lora import LoRAReference, apply_lora
    from distributed_llm_alignment_amd.objectives import dpo_step_loss
    from distributed_llm_alignment_amd.parallel.data_parallel import DataParallelEngine

    overrides = {"num_layers": args.layers} if args.layers else {}
    cfg = get_config(args.model, **overrides)
    policy = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=1234)
    ref = None
    if args.mode != "lora-shared":
        ref = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=1234).eval().requires_grad_(False)
    stats = None
    if args.mode != "full":
        stats = apply_lora(policy, r=args.r, alpha=2 * args.r, seed=0)
        for ad_site in policy.layers:  # B != 0: the backward runs every adapter product on real data
            for ad in (ad_site.attn.lora_qkv, ad_site.attn.lora_o, ad_site.mlp.lora_up, ad_site.mlp.lora_down):
                ad.B.data.normal_(0.0, 0.01)
        if ref is None:
            ref = LoRAReference(policy)
    lr = 1e-6 if args.mode == "full" else 1e-4
    engine = DataParallelEngine(policy, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                                max_grad_norm=1.0, zero_stage=1, bucket_mb=256.0)
    policy.train()
    gen = torch.Generator().manual_seed(17)
    batches = [synthetic_preference_batch(args.micro_pairs, args.seq_len, cfg.vocab_size, device=dev, generator=gen)
               for _ in range(4)]
    state = {"i": 0}

    def train_step():
        for a in range(args.accum):
            b = batches[state["i"] % 4]
            state["i"] += 1
            with (engine.no_sync() if a < args.accum - 1 else _Null()):
                loss, _ = dpo_step_loss(policy, ref, b, beta=0.1)
                (loss / args.accum).backward()
        engine.step()
        return loss

    for _ in range(args.warmup):
        train_step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        loss = train_step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    pairs = args.micro_pairs * args.accum
    rate = [pairs / t for t in times]
    print(json.dumps({"bench": "lora_step", "mode": args.mode, "model": args.model, "layers": cfg.num_layers,
                      "pairs_per_step": pairs, "seq_len": args.seq_len, "r": args.r if args.mode != "full" else None,
                      "pairs_per_s_median": statistics.median(rate), "pairs_per_s_min": min(rate),
                      "pairs_per_s_max": max(rate), "step_s": times,
                      "peak_allocated_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
                      "trainable": stats, "loss": float(loss.detach())}))


REFRESH_SHAPES = [("qkv", 6144, 4096, True), ("o", 4096, 4096, False), ("gate|up", 28672, 4096, True),
                  ("down", 4096, 14336, False)]


def bench_refresh(args):
    dev = _need_gpu()
    k = torch.ops.dla
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name, N, K, fold in REFRESH_SHAPES:
        w = _rand((N, K), dev, gen, K ** -0.5)
        nw = (1.0 + 0.1 * _rand((K,), dev, gen).float()).to(torch.bfloat16) if fold else None
        out = torch.empty((N // 16, K // 32, 4, 16, 8), dtype=torch.bfloat16, device=dev)
        o8 = torch.empty((N // 16, K // 64, 64, 16), dtype=torch.uint8, device=dev)
        sc = torch.empty(N, dtype=torch.float32, device=dev)
        for r in args.ranks:
            a = _rand((r, K), dev, gen, K ** -0.5)
            b = _rand((N, r), dev, gen, r ** -0.5)

            def comp(f8):
                tmp = w.clone()
                k.lora_expand_add_(tmp, b, a, 2.0, True)
                if f8:
                    k.quant_tile_f8(tmp, nw, o8, sc, False)
                else:
                    k.tile_weight(tmp, nw, out, False)

            for f8 in (False, True):
                if f8:
                    arms = {"fused": lambda: k.lora_quant_tile_f8(w, a, b, 2.0, nw, o8, sc, False),
                            "comp": lambda: comp(True), "floor": lambda: k.quant_tile_f8(w, nw, o8, sc, False)}
                else:
                    arms = {"fused": lambda: k.lora_tile_weight(w, a, b, 2.0, nw, out, False),
                            "comp": lambda: comp(False), "floor": lambda: k.tile_weight(w, nw, out, False)}
                rows.append((name, N, K, r, "fp8" if f8 else "bf16", _ab(arms, args.rounds, args.iters)))
        del w, out, o8
    print("| projection | N | K | r | copy | (a) one pass us (min..max) | (b) clone + expand + tile us | "
          "(c) existing op on W us | (a)/(b) | (a)/(c) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, N, K, r, dt, res in rows:
        fm, cm, fl = (statistics.median(res[x]) for x in ("fused", "comp", "floor"))
        print(f"| {name} | {N} | {K} | {r} | {dt} | {_fmt(res['fused'])} | {_fmt(res['comp'])} | {_fmt(res['floor'])} | "
              f"{fm / cm:.2f} | {fm / fl:.2f} |")
    print(json.dumps({"bench": "lora_refresh", "rows": [
        {"proj": name, "N": N, "K": K, "r": r, "copy": dt, **{f"{x}_us": res[x] for x in res}}
        for name, N, K, r, dt, res in rows]}))


def bench_decode(args):
    dev = _need_gpu()
    from distributed_llm_alignment_amd.models import build_model, generate, get_config
    from distributed_llm_alignment_amd.models.lora import apply_lora, lora_adapters, lora_disabled

    overrides = {"num_layers": args.layers} if args.layers else {}
    cfg = get_config(args.model, **overrides)
    m = build_model(cfg, device=dev, dtype=torch.bfloat16, seed=1234).eval()
    apply_lora(m, r=args.r, alpha=2 * args.r, seed=0)
    for ad in lora_adapters(m):
        ad.B.data.normal_(0.0, 0.01)
    n1, n2 = args.new_tokens
    out = []
    for rows in args.rows:
        ids = torch.randint(3, cfg.vocab_size, (rows, args.prompt), device=dev,
                            generator=torch.Generator(device=dev).manual_seed(rows))

        def run(n, merged):
            kw = dict(max_new_tokens=n, do_sample=True, temperature=0.7, top_p=0.9, eos_token_id=-1, seed=1,
                      weight_dtype=args.weight_dtype)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if merged:
                generate(m, ids, None, adapters="merged", **kw)
            else:
                with lora_disabled(m):
                    generate(m, ids, None, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        res = {"merged": [], "base": []}
        for merged in (True, False):  # warm: captures, derived copies, library picks
            run(n1, merged), run(n2, merged)
        for _ in range(args.rounds):
            for name, merged in (("merged", True), ("base", False)):
                res[name].append((run(n2, merged) - run(n1, merged)) / (n2 - n1) * 1e3)
        out.append({"rows": rows, **{f"{k}_ms_per_token": v for k, v in res.items()}})
        print(f"rows {rows}: merged {_fmt(res['merged'])} ms/token, adapter-free {_fmt(res['base'])} ms/token")
    print(json.dumps({"bench": "lora_decode", "model": args.model, "layers": cfg.num_layers, "r": args.r,
                      "weight_dtype": args.weight_dtype, "prompt": args.prompt, "results": out}))


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    pk = sub.add_parser("kernels")
    pk.add_argument("--rounds", type=int, default=7)
    pk.add_argument("--iters", type=int, default=20)
    ps = sub.add_parser("step")
    ps.add_argument("--mode", choices=("full", "lora", "lora-shared"), required=True)
    ps.add_argument("--model", default="llama3-8b")
    ps.add_argument("--layers", type=int, default=None, help="debug only: override the layer count")
    ps.add_argument("--r", type=int, default=16)
    ps.add_argument("--seq-len", type=int, default=1024)
    ps.add_argument("--micro-pairs", type=int, default=4)
    ps.add_argument("--accum", type=int, default=4)
    ps.add_argument("--steps", type=int, default=5)
    ps.add_argument("--warmup", type=int, default=2)
    pr = sub.add_parser("refresh")
    pr.add_argument("--rounds", type=int, default=7)
    pr.add_argument("--iters", type=int, default=10)
    pr.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
    pd = sub.add_parser("decode")
    pd.add_argument("--model", default="llama3-8b")
    pd.add_argument("--layers", type=int, default=None, help="debug only: override the layer count")
    pd.add_argument("--r", type=int, default=16)
    pd.add_argument("--rows", type=int, nargs="+", default=[8, 64])
    pd.add_argument("--prompt", type=int, default=512)
    pd.add_argument("--new-tokens", type=int, nargs=2, default=[64, 192])
    pd.add_argument("--weight-dtype", default="bf16", choices=("bf16", "fp8"))
    pd.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    {"kernels": bench_kernels, "step": bench_step, "refresh": bench_refresh, "decode": bench_decode}[args.cmd](args)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
