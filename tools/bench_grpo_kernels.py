#!/usr/bin/env python
"""Micro-benchmarks of the GRPO kernels on one GPU (device events around repeated launches):

  kv_replicate  the shared-prefill K/V replication at an RLHF shape (default Llama-3-8B: L 32,
                P 8, G 8, Tp 512, Hkv 8, D 128, head-major cache) vs the torch
                `repeat_interleave` + slice-copy fallback on the same tensors: time, effective
                GB/s over the bytes the copy needs (read once + written G times) and the transient
                memory each allocates.
  grpo_loss     the fused loss launch pair (fwd + bwd + metrics) at S = 64, T = 768 vs the composed
                torch formula + autograd backward on the GPU.
  logprob       the LM-head row kernels against their entropy twins at [6144, 128256] and
                [8192, 128256] bf16 logits (an update micro-batch of 8 x 768 tokens, a no-grad chunk):
                logprob_fwd / logprob_entropy_fwd, logprob_bwd / logprob_entropy_bwd,
                logprob_bwd_t / logprob_entropy_bwd_t, the two arms of a pair interleaved (A B A B
                ...), median of the rounds, effective GB/s over the bytes each must move; plus the
                eager torch entropy of the same logits (fp32 log_softmax), for scale. Then every
                one of the six against its tempered twin (`*_temp`, `--temperature`, default 0.7),
                interleaved the same way: `<kernel>_ms` / `<kernel>_temp_ms` / `<kernel>_temp_ratio`
                under "temp". Then the kept-set twins (`logprob_fwd_keep`, `logprob_bwd_keep`,
                `logprob_bwd_t_keep`; one mask row per logits row) against their tempered twins, with
                the traffic ratio the mask bytes account for and the tempered twin's own spread, under
                "keep". With an extension that lacks the twins (an older build through
                DLA_EXT_PATH) only the plain kernels are timed.

  rollout_is    the truncated importance weights at S = 64, T = 768: `rollout_is_weights` (token and
                sequence level) and the raw `grpo_loss` op with and without the weight grid
                (`grpo_loss_w`), interleaved, median of the rounds, with the bytes each moves, against
                the composed torch formulas on the GPU. With an extension that lacks the new ops
                (an older build through DLA_EXT_PATH) only the unweighted loss is timed.

  gspo          the raw `grpo_loss` op (token-level ratio) against `grpo_loss_seq` (sequence-level ratio,
                GSPO), unweighted and weighted, at `--rollouts` x `--tokens`: the arms interleaved round
                by round, median / min / max of the rounds per arm, the bytes each moves (10 grid passes against the
                token op's 9: the row pass reads the mask, lp and old, the later loops no longer read old), and the op against the composed torch
                formula. With an extension that lacks the op (an older build through DLA_EXT_PATH)
                only the token op is timed, in the same harness.

Prints one JSON line per kernel (per shape for `logprob`). `--bench` selects one of them."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms


def transient_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def interleaved(fa, fb, rounds, iters):
    """Median ms of two arms timed alternately (same process, same clocks, warm)."""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, iters, warmup=1))
        tb.append(timed(fb, iters, warmup=1))
    ta.sort()
    tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2]


def bench_logprob(dla_ops, dev, rows, V, rounds, iters, temperature=0.7):
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.empty((rows, V), device=dev, dtype=torch.bfloat16)
    for s in range(0, rows, 1024):  # 3 * randn without an fp32 [rows, V] transient
        logits[s:s + 1024] = (3 * torch.randn((min(1024, rows - s), V), device=dev, generator=g)).to(torch.bfloat16)
    tgt = torch.randint(0, V, (rows,), device=dev, generator=g)
    gl = torch.randn(rows, device=dev, generator=g)
    ge = torch.randn(rows, device=dev, generator=g)
    lp0, lse0 = dla_ops.logprob_fwd(logits, tgt)
    lp, lse, ent = dla_ops.logprob_entropy_fwd(logits, tgt)
    nbytes = logits.numel() * 2
    out = {"bench": "logprob", "rows": rows, "V": V, "logits_gb": round(nbytes / 1e9, 3),
           "logp_lse_bitwise_equal": bool(torch.equal(lp, lp0) and torch.equal(lse, lse0))}

    def gbs(ms, passes):
        return round(passes * nbytes / ms / 1e6, 1)

    a, b = interleaved(lambda: dla_ops.logprob_fwd(logits, tgt),
                       lambda: dla_ops.logprob_entropy_fwd(logits, tgt), rounds, iters)
    out.update(fwd_ms=round(a, 4), entropy_fwd_ms=round(b, 4), fwd_ratio=round(b / a, 4),
               fwd_gb_s=gbs(a, 1), entropy_fwd_gb_s=gbs(b, 1))
    # the backward kernels rewrite their input in place; their time does not depend on the values,
    # so they run repeatedly on one scratch copy
    work = logits.clone()
    a, b = interleaved(lambda: dla_ops.logprob_bwd(work, tgt, lse, gl),
                       lambda: dla_ops.logprob_entropy_bwd(work, tgt, lse, ent, gl, ge), rounds, iters)
    out.update(bwd_ms=round(a, 4), entropy_bwd_ms=round(b, 4), bwd_ratio=round(b / a, 4),
               bwd_gb_s=gbs(a, 2), entropy_bwd_gb_s=gbs(b, 2))
    a, b = interleaved(lambda: dla_ops.logprob_bwd_t(work, tgt, lse, gl),
                       lambda: dla_ops.logprob_entropy_bwd_t(work, tgt, lse, ent, gl, ge), rounds, iters)
    out.update(bwd_t_ms=round(a, 4), entropy_bwd_t_ms=round(b, 4), bwd_t_ratio=round(b / a, 4),
               bwd_t_gb_s=gbs(a, 3), entropy_bwd_t_gb_s=gbs(b, 3))
    if hasattr(dla_ops, "logprob_fwd_temp"):  # the tempered twins, each against its plain kernel
        it = float(torch.tensor(1.0 / temperature, dtype=torch.float64).float())
        pairs = [
            ("fwd", 1, lambda: dla_ops.logprob_fwd(logits, tgt), lambda: dla_ops.logprob_fwd_temp(logits, tgt, it)),
            ("entropy_fwd", 1, lambda: dla_ops.logprob_entropy_fwd(logits, tgt),
             lambda: dla_ops.logprob_entropy_fwd_temp(logits, tgt, it)),
            ("bwd", 2, lambda: dla_ops.logprob_bwd(work, tgt, lse, gl),
             lambda: dla_ops.logprob_bwd_temp(work, tgt, lse, gl, it)),
            ("entropy_bwd", 2, lambda: dla_ops.logprob_entropy_bwd(work, tgt, lse, ent, gl, ge),
             lambda: dla_ops.logprob_entropy_bwd_temp(work, tgt, lse, ent, gl, ge, it)),
            ("bwd_t", 3, lambda: dla_ops.logprob_bwd_t(work, tgt, lse, gl),
             lambda: dla_ops.logprob_bwd_t_temp(work, tgt, lse, gl, it)),
            ("entropy_bwd_t", 3, lambda: dla_ops.logprob_entropy_bwd_t(work, tgt, lse, ent, gl, ge),
             lambda: dla_ops.logprob_entropy_bwd_t_temp(work, tgt, lse, ent, gl, ge, it)),
        ]
        temp = {"temperature": temperature}
        for name, passes, plain, tempered in pairs:
            a, b = interleaved(plain, tempered, rounds, iters)
            temp.update({f"{name}_ms": round(a, 4), f"{name}_temp_ms": round(b, 4),
                         f"{name}_temp_ratio": round(b / a, 4), f"{name}_temp_gb_s": gbs(b, passes)})
        lp1, lse1 = dla_ops.logprob_fwd_temp(logits, tgt, 1.0)
        temp["unit_temperature_bitwise_equal"] = bool(torch.equal(lp1, lp0) and torch.equal(lse1, lse0))
        out["temp"] = temp
    if hasattr(dla_ops, "logprob_fwd_keep") and V % 8 == 0:
        # the kept-set twins, each against its tempered twin; one mask row per logits row (every token
        # of a rollout has its own set), the 64 largest logits of each row kept. `*_temp_spread`: the
        # tempered twin against itself, interleaved the same way (the run-to-run spread of the pair).
        it = float(torch.tensor(1.0 / temperature, dtype=torch.float64).float())
        keep = torch.zeros((rows, V // 8), device=dev, dtype=torch.uint8)
        for s in range(0, rows, 1024):
            m = torch.zeros((min(1024, rows - s), V), device=dev, dtype=torch.bool)
            m.scatter_(1, logits[s:s + 1024].topk(64, dim=-1).indices, True)
            w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device=dev, dtype=torch.int32)
            keep[s:s + 1024] = (m.view(m.shape[0], V // 8, 8).int() * w).sum(-1).to(torch.uint8)
            del m
        kr = torch.arange(rows, device=dev)
        lsek = dla_ops.logprob_fwd_keep(logits, tgt, keep, kr, it)[1]
        pairs = [
            ("fwd", 1, 1 / 16, lambda: dla_ops.logprob_fwd_temp(logits, tgt, it),
             lambda: dla_ops.logprob_fwd_keep(logits, tgt, keep, kr, it)),
            ("bwd", 2, 1 / 32, lambda: dla_ops.logprob_bwd_temp(work, tgt, lse, gl, it),
             lambda: dla_ops.logprob_bwd_keep(work, tgt, lsek, gl, keep, kr, it)),
            ("bwd_t", 3, 1 / 48, lambda: dla_ops.logprob_bwd_t_temp(work, tgt, lse, gl, it),
             lambda: dla_ops.logprob_bwd_t_keep(work, tgt, lsek, gl, keep, kr, it)),
        ]
        kp = {"temperature": temperature, "keep_mib": round(keep.numel() / 2 ** 20, 1)}
        for name, passes, extra, tempered, kept in pairs:
            a, b = interleaved(tempered, kept, rounds, iters)
            a1, a2 = interleaved(tempered, tempered, rounds, iters)
            kp.update({f"{name}_temp_ms": round(a, 4), f"{name}_keep_ms": round(b, 4),
                       f"{name}_keep_ratio": round(b / a, 4), f"{name}_traffic_ratio": round(1 + extra, 4),
                       f"{name}_temp_spread": round(max(a1, a2) / min(a1, a2) - 1, 4),
                       f"{name}_keep_gb_s": gbs(b, passes)})
        out["keep"] = kp
        del keep
    del work

    def eager():
        lsm = torch.log_softmax(logits.float(), -1)
        return -(lsm.exp() * lsm).sum(-1)

    want = eager()
    out["entropy_max_abs_diff_vs_eager"] = float((ent - want).abs().max())
    del want
    out["eager_torch_entropy_ms"] = round(timed(eager, max(2, iters // 4), warmup=1), 4)
    out["eager_torch_entropy_transient_mib"] = round(transient_bytes(eager) / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", choices=("all", "kv_replicate", "grpo_loss", "logprob", "rollout_is", "gspo"),
                    default="all")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--logprob-rows", type=int, nargs="+", default=[6144, 8192])
    ap.add_argument("--rounds", type=int, default=5, help="logprob: interleaved rounds per pair")
    ap.add_argument("--temperature", type=float, default=0.7, help="logprob: temperature of the tempered arms")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--token-major", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rollouts", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=768)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from distributed_llm_alignment_amd import ops
    from distributed_llm_alignment_amd.ops import _ext
    from distributed_llm_alignment_amd.ops.losses import _ref_grpo_loss

    dla_ops = _ext.require()
    dev = torch.device("cuda", 0)
    if a.bench in ("all", "kv_replicate"):
        bench_kv_replicate(a, ops, dev)
    if a.bench in ("all", "grpo_loss"):
        bench_grpo_loss(a, ops, dev, _ref_grpo_loss)
    if a.bench in ("all", "logprob"):
        for rows in a.logprob_rows:
            bench_logprob(dla_ops, dev, rows, a.vocab, a.rounds, a.iters, a.temperature)
    if a.bench in ("all", "rollout_is"):
        bench_rollout_is(a, dla_ops, dev)
    if a.bench in ("all", "gspo"):
        bench_gspo(a, dla_ops, dev)
    return 0


def bench_kv_replicate(a, ops, dev):
    L, P, G, Tp, H, D = a.layers, a.prompts, a.group, a.prompt, a.kv_heads, a.head_dim
    T_max = Tp + a.new

    def cache(rows, T):
        if a.token_major:
            return torch.zeros((L, rows, T, H, D), device=dev, dtype=torch.bfloat16)
        return torch.zeros((L, rows, H, T, D), device=dev, dtype=torch.bfloat16).transpose(2, 3)

    sk, sv = cache(P, Tp), cache(P, Tp)
    sk.normal_()
    sv.normal_()
    dk, dv = cache(P * G, T_max), cache(P * G, T_max)

    def hip():
        ops.decode.kv_replicate(sk, sv, dk, dv, G)

    def fallback():
        dk[:, :, :Tp] = sk.repeat_interleave(G, dim=1)
        dv[:, :, :Tp] = sv.repeat_interleave(G, dim=1)

    fallback()
    want_k, want_v = dk.clone(), dv.clone()
    dk.zero_()
    dv.zero_()
    hip()
    same = bool(torch.equal(dk, want_k) and torch.equal(dv, want_v))
    del want_k, want_v
    src_bytes = 2 * sk.numel() * 2
    moved = src_bytes * (1 + G)  # read once, written G times
    t_hip, t_fb = timed(hip, a.iters), timed(fallback, a.iters)
    print(json.dumps({"bench": "kv_replicate", "layout": "token-major" if a.token_major else "head-major",
                      "L": L, "P": P, "G": G, "Tp": Tp, "Hkv": H, "D": D, "bitwise_equal_fallback": same,
                      "needed_gb": round(moved / 1e9, 3), "hip_ms": round(t_hip, 4),
                      "hip_gb_s": round(moved / t_hip / 1e6, 1), "fallback_ms": round(t_fb, 4),
                      "fallback_gb_s_same_bytes": round(moved / t_fb / 1e6, 1),
                      "hip_transient_mib": round(transient_bytes(hip) / 2 ** 20, 1),
                      "fallback_transient_mib": round(transient_bytes(fallback) / 2 ** 20, 1)}), flush=True)
    del sk, sv, dk, dv


def bench_grpo_loss(a, ops, dev, _ref_grpo_loss):
    S, T = a.rollouts, a.tokens
    g = torch.Generator(device=dev).manual_seed(0)
    lp = -torch.rand(S, T, device=dev, generator=g) * 3
    old = lp + 0.3 * torch.randn(S, T, device=dev, generator=g)
    ref = lp + 0.2 * torch.randn(S, T, device=dev, generator=g)
    mask = (torch.rand(S, T, device=dev, generator=g) > 0.3).float()
    adv = torch.randn(S, device=dev, generator=g)
    out = {"bench": "grpo_loss", "S": S, "T": T}
    for lt in ("sequence", "token", "constant"):
        def fused():
            x = lp.detach().requires_grad_(True)
            loss, _ = ops.grpo_loss(x, old, ref, adv, mask, 0.2, 0.28, 0.04, lt, T)
            loss.backward()
            return loss, x.grad

        def composed():
            x = lp.detach().requires_grad_(True)
            loss, _ = _ref_grpo_loss(x, old, ref, adv, mask, 0.2, 0.28, 0.04, lt, T)
            loss.backward()
            return loss, x.grad

        (l1, g1), (l2, g2) = fused(), composed()
        out[f"{lt}_loss_diff"] = float((l1 - l2).detach().abs())
        out[f"{lt}_grad_max_diff"] = float((g1 - g2).abs().max())
        out[f"{lt}_fused_ms"] = round(timed(fused, 50), 4)
        out[f"{lt}_composed_ms"] = round(timed(composed, 50), 4)
    print(json.dumps(out), flush=True)


def bench_rollout_is(a, dla_ops, dev):
    from distributed_llm_alignment_amd.ops import losses

    S, T = a.rollouts, a.tokens
    g = torch.Generator(device=dev).manual_seed(0)
    lp = -torch.rand(S, T, device=dev, generator=g) * 3
    old = lp + 0.3 * torch.randn(S, T, device=dev, generator=g)
    ref = lp + 0.2 * torch.randn(S, T, device=dev, generator=g)
    rlp = old + 0.3 * torch.randn(S, T, device=dev, generator=g)  # the rollout engine's log-probs
    mask = (torch.rand(S, T, device=dev, generator=g) > 0.3).float()
    adv = torch.randn(S, device=dev, generator=g)
    grid = S * T * 4
    tail = (None, 0.2, 0.28, 0.04, 0, float(T))
    out = {"bench": "rollout_is", "S": S, "T": T, "grid_bytes": grid, "rounds": a.rounds, "iters": a.iters,
           # passes over one [S, T] fp32 grid: partials read 4 (+ w), grad reads 4 (+ w) and writes 1
           "grpo_loss_bytes": 9 * grid, "grpo_loss_w_bytes": 11 * grid,
           # token level reads 3 and writes 1; the sequence level reads the mask and both log-probs once more
           "is_token_bytes": 4 * grid, "is_sequence_bytes": 7 * grid}

    def plain():
        return dla_ops.grpo_loss(lp, old, ref, adv, mask, *tail)

    has_new = hasattr(losses, "rollout_is_weights")
    try:
        dla_ops.rollout_is_weights
    except (AttributeError, RuntimeError):
        has_new = False
    if not has_new:  # an older extension: the unweighted loss alone, same harness
        ts = sorted(timed(plain, a.iters, warmup=1) for _ in range(a.rounds))
        out["grpo_loss_ms"] = round(ts[len(ts) // 2], 4)
        print(json.dumps(out), flush=True)
        return
    w, _ = dla_ops.rollout_is_weights(old, rlp, mask, 2.0, 0.5, 0, 0)

    def weighted():
        return dla_ops.grpo_loss_w(lp, old, ref, adv, mask, w, *tail)

    ta, tb = interleaved(plain, weighted, a.rounds, a.iters)
    out.update(grpo_loss_ms=round(ta, 4), grpo_loss_w_ms=round(tb, 4), w_ratio=round(tb / ta, 4),
               grpo_loss_w_gb_s=round(11 * grid / tb / 1e6, 1))
    ones = dla_ops.grpo_loss_w(lp, old, ref, adv, mask, torch.ones_like(w), *tail)
    out["w_ones_bitwise_equal_unweighted"] = all(torch.equal(x, y) for x, y in zip(ones, plain()))
    for level, name in ((0, "token"), (1, "sequence")):
        def fused():
            return dla_ops.rollout_is_weights(old, rlp, mask, 2.0, 0.5, level, 0)

        def composed():
            return losses._ref_rollout_is_weights(old, rlp, mask, 2.0, 0.5, name, "truncate")

        (w1, m1), (w2, m2) = fused(), composed()
        out[f"is_{name}_w_max_diff"] = float((w1 - w2).abs().max())
        out[f"is_{name}_metrics_max_diff"] = float((m1 - m2).abs().max())
        tf, tc = interleaved(fused, composed, a.rounds, a.iters)
        out[f"is_{name}_ms"] = round(tf, 4)
        out[f"is_{name}_composed_ms"] = round(tc, 4)
        out[f"is_{name}_gb_s"] = round(out[f"is_{name}_bytes"] / tf / 1e6, 1)

    def fused_step():  # what `correct` adds to a step plus the weighted loss, through the wrappers
        x = lp.detach().requires_grad_(True)
        wi, _ = losses.rollout_is_weights(old, rlp, mask)
        loss, _ = losses.grpo_loss(x, old, ref, adv, mask, 0.2, 0.28, 0.04, "sequence", T, is_weight=wi)
        loss.backward()
        return loss, x.grad

    def composed_step():
        x = lp.detach().requires_grad_(True)
        wi, _ = losses._ref_rollout_is_weights(old, rlp, mask)
        loss, _ = losses._ref_grpo_loss(x, old, ref, adv, mask, 0.2, 0.28, 0.04, "sequence", T, is_weight=wi)
        loss.backward()
        return loss, x.grad

    (l1, g1), (l2, g2) = fused_step(), composed_step()
    out["step_loss_diff"] = float((l1 - l2).detach().abs())
    out["step_grad_max_diff"] = float((g1 - g2).abs().max())
    tf, tc = interleaved(fused_step, composed_step, a.rounds, a.iters)
    out.update(step_fused_ms=round(tf, 4), step_composed_ms=round(tc, 4))
    print(json.dumps(out), flush=True)


def bench_gspo(a, dla_ops, dev):
    from distributed_llm_alignment_amd.ops import losses

    S, T = a.rollouts, a.tokens
    g = torch.Generator(device=dev).manual_seed(0)
    lp = -torch.rand(S, T, device=dev, generator=g) * 3
    old = lp + 0.3 * torch.randn(S, T, device=dev, generator=g)
    ref = lp + 0.2 * torch.randn(S, T, device=dev, generator=g)
    mask = (torch.rand(S, T, device=dev, generator=g) > 0.3).float()
    adv = torch.randn(S, device=dev, generator=g)
    w = 2.0 * torch.rand(S, T, device=dev, generator=g)
    grid = S * T * 4
    tail = (None, 0.2, 0.28, 0.04, 0, float(T))
    arms = {"grpo_loss": lambda: dla_ops.grpo_loss(lp, old, ref, adv, mask, *tail)}
    # passes over one [S, T] fp32 grid: the token op reads lp, old, ref, m in both launches and writes dlp
    # (4 + 4 + 1). The sequence op reads m, lp, old in the row pass, m, lp, ref (+ w) in the second loop
    # and m, lp, ref in the gradient launch, and writes dlp: 3 + 3 + 3 + 1, and one more with the weights
    nbytes = {"grpo_loss": 9 * grid, "grpo_loss_seq": 10 * grid, "grpo_loss_seq_w": 11 * grid}
    try:
        dla_ops.grpo_loss_seq
        arms["grpo_loss_seq"] = lambda: dla_ops.grpo_loss_seq(lp, old, ref, adv, mask, None, *tail)
        arms["grpo_loss_seq_w"] = lambda: dla_ops.grpo_loss_seq(lp, old, ref, adv, mask, w, *tail)
    except (AttributeError, RuntimeError):
        pass  # an older extension: the token op alone
    out = {"bench": "gspo", "S": S, "T": T, "grid_bytes": grid, "rounds": a.rounds, "iters": a.iters}
    ts = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            ts[k].append(timed(fn, a.iters, warmup=1))
    for k, v in ts.items():
        v.sort()
        out[f"{k}_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        out[f"{k}_gb_s"] = round(nbytes[k] / v[len(v) // 2] / 1e6, 1)
    if "grpo_loss_seq" in arms:
        out["seq_ratio"] = round(out["grpo_loss_seq_ms"]["median"] / out["grpo_loss_ms"]["median"], 4)
        x = lp.detach().requires_grad_(True)
        l1, _ = losses.grpo_loss(x, old, ref, adv, mask, 0.2, 0.28, 0.04, "sequence", T, importance_level="sequence")
        l1.backward()
        y = lp.detach().requires_grad_(True)
        l2, _ = losses._ref_grpo_loss(y, old, ref, adv, mask, 0.2, 0.28, 0.04, "sequence", T,
                                      importance_level="sequence")
        l2.backward()
        out["seq_loss_diff"] = float((l1 - l2).detach().abs())
        out["seq_grad_max_diff"] = float((x.grad - y.grad).abs().max())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    sys.exit(main())
