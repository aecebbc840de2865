"""Distillation (reference: src/training/train_distill.py:32-175).

`distill.use_kl and distill.on_policy` with teachers -> token-masked ensemble forward KL
KL(mean_k softmax(teacher_k) || softmax(student)) over every (unshifted) position, fused in one
HIP row kernel (fwd + in-place grad, no [K, B, T, V] fp32 tensors); otherwise causal-LM CE on
the teacher rollouts. Teachers are frozen (Appendix A #15) and must share the student's
vocabulary. Metrics: `train/loss`, `train/reward_mean`. Checkpoint: student, then teachers.

`distill.gkd.enabled: true` -> on-policy distillation (GKD, Agarwal et al.; not in the reference):
the loss is JSD(`beta`) at `temperature` between student and teacher(s) over the positions that
predict a response token (`objectives.gkd_loss`, csrc/gjsd.hip), and each micro-batch is, with
probability `lmbda`, a batch of sequences the STUDENT samples from the micro-batch's prompts (at the
same `temperature`, `max_new_tokens`, `top_p` / `top_k`; hipGraph decode + fused sampler) which the
teachers then score, else the dataset's teacher rollout. The branch comes from a
`random.Random(seed)` stream every rank advances identically. Also logged: `train/gkd_on_policy`
(share of on-policy micro-batches since the last log) and `train/gkd_gen_len` (mean generated
tokens of those). With `enabled: false` (default) the trainer is the one above, untouched."""
from __future__ import annotations

import argparse
import math
import random
from typing import Dict, List, Optional

import torch

from ..data import TeacherRolloutDataset, build_dataloader
from ..models import generate, load_causal_lm
from ..objectives import distill_loss, gkd_loss
from ..utils.config import add_config_args, config_from_args, hardware_parallel
from .common import (_tokenize_left, effective_batch_msg, lora_enabled, make_engine, maybe_apply_lora, meta_init,
                     parallelize, setup, train_loop)

# GKD's usual settings in the literature; config defaults, not something tuned here
GKD_DEFAULTS = {"enabled": False, "beta": 0.5, "lmbda": 0.5, "temperature": 0.9, "max_new_tokens": 128,
                "top_p": 1.0, "top_k": 0}


def parse_args(argv=None) -> argparse.Namespace:
    return add_config_args(argparse.ArgumentParser(description="Distill aligned teacher into student")).parse_args(argv)


def teacher_paths(config: Dict) -> List[str]:
    dcfg = config.get("distill", {}) or {}
    paths = dcfg.get("teacher_model_names_or_paths") or []
    if not paths:
        single = dcfg.get("teacher_model_name_or_path") or (config.get("model", {}) or {}).get("teacher_path")
        paths = [single] if single else []
    return list(paths)


def gkd_settings(config: Dict) -> Optional[Dict]:
    """The `distill.gkd` section with its defaults, or None when it is off. Every combination the
    GKD path does not serve raises ValueError here, before a model is loaded."""
    dcfg = config.get("distill", {}) or {}
    raw = dcfg.get("gkd") or {}
    unknown = set(raw) - set(GKD_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown distill.gkd key(s): {sorted(unknown)}")
    g = {**GKD_DEFAULTS, **raw}
    if not g["enabled"]:
        return None
    try:
        g.update(beta=float(g["beta"]), lmbda=float(g["lmbda"]), temperature=float(g["temperature"]),
                 max_new_tokens=int(g["max_new_tokens"]), top_p=float(g["top_p"]), top_k=int(g["top_k"]))
    except (TypeError, ValueError) as e:
        raise ValueError(f"distill.gkd: {e}") from None
    if not 0.0 <= g["beta"] <= 1.0:
        raise ValueError(f"distill.gkd.beta must be in [0, 1], got {g['beta']!r}")
    if not 0.0 <= g["lmbda"] <= 1.0:
        raise ValueError(f"distill.gkd.lmbda must be in [0, 1], got {g['lmbda']!r}")
    if not (math.isfinite(g["temperature"]) and g["temperature"] > 0.0):
        raise ValueError(f"distill.gkd.temperature must be finite and > 0, got {g['temperature']!r}")
    if g["lmbda"] > 0.0 and g["max_new_tokens"] < 1:
        raise ValueError(f"distill.gkd.max_new_tokens must be >= 1, got {g['max_new_tokens']!r}")
    if dcfg.get("use_kl", False):
        raise ValueError("distill.gkd.enabled and distill.use_kl are two different losses: set one")
    if not teacher_paths(config):
        raise ValueError("distill.gkd needs a teacher (distill.teacher_model_name(s)_or_path(s))")
    hw = hardware_parallel(config)
    if hw["tp_size"] > 1 or hw["sp_size"] > 1:
        raise ValueError("distill.gkd does not support tensor or sequence parallelism "
                         "(vocab-parallel / sequence-parallel LM heads)")
    z = hw.get("zero_stage")
    if g["lmbda"] > 0.0 and (hw.get("fsdp") or (z is not None and int(z) >= 3)):
        raise ValueError("distill.gkd.lmbda > 0 under ZeRO-3 / FSDP: student rollouts from gathered weights "
                         "are not wired into this trainer; use zero_stage <= 1 or lmbda: 0")
    return g


def main(argv=None) -> int:
    args = parse_args(argv)
    config = config_from_args(args)
    gkd = gkd_settings(config)
    if lora_enabled(config) and gkd and gkd["lmbda"] > 0.0:
        raise ValueError("model.lora with distill.gkd.lmbda > 0: student rollouts need generate(), which does "
                         "not run live adapters; use lmbda: 0 or disable model.lora")
    ctx = setup(config, "distill", default_seed=0)
    model_cfg: Dict = config["model"]
    dcfg: Dict = config.get("distill", {}) or {}
    student = load_causal_lm(model_cfg["student_model_name_or_path"],
                             gradient_checkpointing=model_cfg.get("gradient_checkpointing", True),
                             device=ctx.device, seed=ctx.seed, meta_init=meta_init(ctx))
    use_kl = bool(dcfg.get("use_kl", False) and dcfg.get("on_policy", False))
    teachers: List = []
    if use_kl or gkd:
        paths = teacher_paths(config)
        if not paths:
            raise ValueError("KL distillation requested but no teacher model path provided")
        for i, tp in enumerate(paths):
            tb = load_causal_lm(tp, gradient_checkpointing=False, device=ctx.device, seed=ctx.seed + 1 + i,
                                 meta_init=meta_init(ctx))
            tb.model.eval().requires_grad_(False)
            teachers.append(tb.model)
    parallelize(ctx, student.model)
    maybe_apply_lora(ctx, student.model, model_cfg["student_model_name_or_path"])  # student only
    for t in teachers:
        parallelize(ctx, t)
    tok = student.tokenizer
    max_len = model_cfg.get("max_seq_length", 2048)
    ds = TeacherRolloutDataset(config["data"]["teacher_samples_path"], tok, max_length=max_len,
                               with_prompt=bool(gkd))
    opt = config["optimization"]
    micro = opt["micro_batch_size"]
    loader, sampler = build_dataloader(ds, micro, shuffle=True,
                                       num_workers=config["data"].get("num_workers", 4), seed=ctx.seed)
    engine = make_engine(ctx, student.model, lr=opt["learning_rate"],
                         weight_decay=opt.get("weight_decay", 0.0), max_grad_norm=opt.get("max_grad_norm", 1.0))
    lg = config["logging"]
    ctx.log(effective_batch_msg(ctx, micro))
    student.model.train()

    def step_fn(batch):
        reward = batch.pop("reward")
        loss = distill_loss(student.model, teachers, batch, use_kl)
        return loss, {"reward": reward}

    def extra_log(_step, m):
        return {"train/reward_mean": m["reward"].float().mean()}

    if gkd:
        step_fn, extra_log = _gkd_steps(ctx, gkd, student, teachers, ds, tok, max_len)
        ctx.log(f"GKD: beta {gkd['beta']} lmbda {gkd['lmbda']} temperature {gkd['temperature']}")

    train_loop(ctx, loader, sampler, engine, step_fn, opt["max_train_steps"], [student.model] + teachers, tok,
               log_every=lg.get("log_every_steps", 20), save_every=lg.get("save_every_steps", 400),
               extra_log_fn=extra_log, resume=args.resume, keep_last=lg.get("keep_last"))
    ctx.log("Distillation complete")
    ctx.logger.close()
    return 0


def _gkd_steps(ctx, gkd: Dict, student, teachers, ds: TeacherRolloutDataset, tok, max_len: int):
    """(step_fn, extra_log_fn) of the GKD mode."""
    branch = random.Random(ctx.seed)  # the same draws on every rank: all ranks take the same branch
    gen_g = torch.Generator(device=ctx.device)
    gen_g.manual_seed(ctx.seed * 1000 + (ctx.mesh.dp_rank if ctx.mesh is not None else ctx.dist.rank))
    beta, T, n_new = gkd["beta"], gkd["temperature"], gkd["max_new_tokens"]
    prompt_max = max(1, int(max_len) - n_new)
    since = {"micro": 0, "on": 0, "gen": torch.zeros((), device=ctx.device), "rows": 0}

    def step_fn(batch):
        reward = batch.pop("reward")
        since["micro"] += 1
        if branch.random() < gkd["lmbda"]:
            prompts = [ds.prompt_text(i) for i in batch["index"].tolist()]
            ids, am = _tokenize_left(tok, prompts, prompt_max, ctx.device)
            with torch.no_grad():
                seqs, mask = generate(student.model, ids, am, max_new_tokens=n_new, do_sample=True, temperature=T,
                                      top_p=gkd["top_p"], top_k=gkd["top_k"], pad_token_id=tok.pad_token_id,
                                      eos_token_id=getattr(tok, "eos_token_id", None), generator=gen_g,
                                      return_mask=True)
            Tp = ids.shape[1]
            since["on"] += 1
            since["gen"] += mask[:, Tp:].sum()
            since["rows"] += int(mask.shape[0])
            # per row: its real prompt tokens (Tp less the left padding)
            loss = gkd_loss(student.model, teachers, seqs, mask, am.sum(1), beta, T)
        else:
            loss = gkd_loss(student.model, teachers, batch["input_ids"], batch["attention_mask"],
                            batch["prompt_len"], beta, T)
        return loss, {"reward": reward}

    def extra_log(_step, m):
        rec = {"train/reward_mean": m["reward"].float().mean(),
               "train/gkd_on_policy": since["on"] / max(since["micro"], 1),
               "train/gkd_gen_len": float(since["gen"]) / max(since["rows"], 1)}
        since.update(micro=0, on=0, rows=0)
        since["gen"].zero_()
        return rec

    return step_fn, extra_log


if __name__ == "__main__":
    raise SystemExit(main())
