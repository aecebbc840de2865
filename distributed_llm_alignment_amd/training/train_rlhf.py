"""KL-penalised policy-gradient RLHF ("PPO-style"; reference: src/training/train_rlhf.py:61-166).

Per step: sample `ppo.batch_size` prompts (same seed on every rank), take this rank's contiguous
slice (fixes Appendix A #1), left-pad and generate with the native KV-cache decoder (HIP flash
attention over the cache), score `prompt\\n\\nresponse` with the reward model (eval mode, no grad:
fixes #8), then REINFORCE with a KL-shaped reward and a mean baseline:
    kl = logp_pi - logp_ref ;  r' = r - kl_coef*kl ;  A = r' - mean(r') ;  loss = -mean(A * logp_pi)
(fused HIP kernel). The log-prob mask covers prompt + generated tokens up to and including EOS
(fixes #10). `generation_params.do_sample` defaults to True (#9). `ppo.update_micro_batch: m`
runs the update as gradient-accumulated micro-batches of m rollouts with a baseline each, the
per-process semantics of the reference's multi-process run (`reinforce_update`).

Overlap (BASELINE north star, `ppo.async_rollouts: true`, off by default since it changes the
semantics to one-step-stale rollouts): step k+1's rollouts are generated while step k's gradient
reduce-scatter is still in flight on RCCL's stream. `train/comm_exposed_ms` logs the part of the
gradient collectives the step did not hide (the compute stream's wait at `engine.step`;
parallel/dist.py ExposedCommTimer); tests/test_distributed_cpu.py measures it with 2 gloo ranks.

`ppo.algorithm: ppo` (not in the reference, whose loop is critic-free) switches to token-level
actor-critic PPO, the north-star "PPO RLHF (actor + critic + reward)" configuration: a critic
(`ValueModel`, initialised from `critic.base_model_name_or_path` or the reward backbone) gives
per-token values, the per-token reward is -kl_coef * (logp - logp_ref) plus the reward-model
score on the last generated token, advantages are GAE(gamma, lam) (HIP wave-scan kernel),
whitened; `ppo_epochs` x `num_minibatches` updates of the clipped surrogate + `vf_coef` x the
clipped value loss (fused HIP fwd+bwd kernels), policy and critic each on their own engine.

`ppo.algorithm: grpo` is the critic-free, group-relative family (GRPO and its DAPO / Dr. GRPO
normalisations): each step draws `ppo.batch_size / ppo.group_size` prompts and samples every one
`group_size` times on ONE shared prompt prefill (`generate(num_return_sequences=G)`;
`ppo.group_attention: true` also reads the prompt K/V once per group in every decode step); the reward is
the reward-model score alone, a rollout's advantage is its score standardised inside its group
(`ppo.scale_rewards: false`: only centred), and the update is the token-level clipped surrogate
(`ppo.clip_range` / `ppo.clip_range_high`) plus `ppo.kl_coef` x the k3 KL to the frozen reference,
normalised per `ppo.loss_type: sequence|token|constant` (fused HIP fwd+bwd kernels). No critic:
the memory plan is the REINFORCE one. `ppo_epochs`, `num_minibatches`, `update_micro_batch` and
`async_rollouts` work as for the other algorithms; with one epoch and one minibatch the update is
on-policy and the old-policy forward is skipped.

`ppo.entropy_coef` (default 0) and `ppo.log_entropy` (default false), for `ppo` and `grpo`: the
per-token policy entropy comes out of the LM-head log-prob kernels' own vocabulary pass
(`token_logprobs(with_entropy=True)`); the loss gains -entropy_coef x its mean over the
minibatch's action tokens and `train/entropy` is logged. With both off a run launches exactly the
kernels it launched before. The REINFORCE loop works on sequence log-probs and has no entropy term.

`ppo.rollout_logprobs: off|monitor|old|correct` (default off), for `ppo` and `grpo`: the fused sampler also
returns the log-prob of every sampled token under the engine that sampled it
(`generate(return_logprobs=True)`; temperature 1, full vocabulary, like `token_logprobs`). `monitor`
leaves the update alone and logs `train/rollout_kl` (mean over action tokens of logp_rollout -
logp_trainer) and `train/rollout_logp_absdiff_max`: how far fp8 / stale / differently rounded
rollouts are from the trainer's policy. `old` uses them AS the old-policy log-probs (in PPO's KL
reward too) and skips the trainer's old-policy forward over the rollouts. With `off` the rollouts
do not request them and a run launches exactly the kernels it launched before.

`correct` is truncated importance sampling: the trainer keeps its own old-policy log-probs (ratio,
clip and PPO's KL reward as with `off`; GRPO runs the old-policy forward even on-policy, as
`monitor` does) and multiplies every action token's surrogate by a detached weight, computed once
per rollout batch by one fused HIP op and sliced into minibatches and micro-batches:
    w = min(exp(l), C),  l = logp_trainer_old - logp_rollout     (`rollout_is_mode: truncate`)
    w = exp(l) if F <= exp(l) <= C else 0                        (`rollout_is_mode: mask`)
with C = `ppo.rollout_is_cap` (default 2.0), F = `ppo.rollout_is_floor` (default 1 / C), and
`ppo.rollout_is_level: token` (default) or `sequence`, where l is the row's mean over its action
tokens (the length-normalised ratio, not the product). The weight multiplies the policy-gradient
term only; the k3 KL term, every divisor (action-token counts, never sum w) and clipfrac /
approx_kl / kl stay unweighted. Logged: `train/rollout_is_mean`, `train/rollout_is_frac_high`,
`train/rollout_is_frac_low`, `train/rollout_is_ess`, and `monitor`'s two metrics.

`ppo.logprob_temperature: 1.0 | <float > 0> | rollout` (default 1.0), for `ppo` and `grpo`: the ONE
temperature of every log-prob of the step. The rollouts are drawn from softmax(z / T_gen); at 1.0
the trainer optimises softmax(z), a different distribution. `rollout` resolves to
`generation_params.temperature` when `do_sample` is set (else 1.0). The policy's, old policy's and
reference's `token_logprobs`, the entropy (bonus and `train/entropy`) and the rollout engine's
log-probs (`generate(logprob_temperature=)`) are then all of softmax(z / T), and through them the
ratio, the clip, the k3 KL, PPO's KL reward, `rollout_kl` and the importance weights of `correct`.
The temperature is applied in fp32 inside the LM-head row kernels and the sampler's draw pass, on
the bf16 logits the GEMM wrote. With `rollout_logprobs` on, the value must be 1.0 or the rollout
temperature (the sampler has no other). `train/logprob_temperature` is logged once when the key is
set. At 1.0 (or absent) a run launches exactly the kernels it launched before. The log-prob is
over the full vocabulary: with `top_p < 1` / `top_k` it is still not the filtered draw distribution.

`ppo.keep_sampling_mask: false | true` (default false), for `ppo` and `grpo`: with a top-k / top-p
filter the rollout tokens are drawn from softmax(z / T_gen) renormalised over a kept set K per token.
With the key on the rollouts also return K, packed one bit per vocabulary entry
(`generate(return_keep_mask=True)`, S * n * V / 8 bytes), and EVERY trainer-side log-prob of a token
(policy, old policy, reference) is taken over that token's K, the mask read by the LM-head row
kernels next to the logits (`token_logprobs(keep=, keep_rows=)`): ratio, clip, k3 KL, PPO's KL
reward live on the action space the sampler used. `rollout_logprobs: monitor|old|correct` then use
the engine's kept-set log-probs (the exact behaviour log-probs) against the trainer's kept-set ones,
so `logprob_temperature` must be the rollout temperature there. Not with `reinforce`, an inactive
filter, greedy decoding, `entropy_coef` / `log_entropy` (no entropy under a kept set yet), tensor or
sequence parallelism, or a vocabulary not divisible by 8: each raises at start-up. Absent or false,
a run launches exactly the kernels it launched before.

`ppo.importance_sampling_level: token | sequence` (default token), for `grpo` only: `sequence` is
GSPO (Group Sequence Policy Optimization). The reward and the advantage are per rollout, so the
ratio becomes per rollout too: sr_s = exp(mean over the row's action tokens of logp - logp_old),
the length-normalised ratio (not the product), clipped once per rollout, and every action token of
the row carries the row's surrogate max(-A sr_s, -A clamp(sr_s, 1 - clip_range, 1 + clip_range_high));
the gradient flows through sr_s to every action token (fused HIP fwd+bwd kernels, two launches, no
host sync). The k3 KL term stays per token; `loss_type`, the shared micro-batch divisor (micro-batches
slice whole rows), `rollout_logprobs`, `logprob_temperature` and `keep_sampling_mask` keep their
meaning, and the importance weights of `correct` stay per token. `train/clipfrac` and
`train/approx_kl` are token-weighted means of the per-rollout values. A length-normalised ratio
moves far less than a token ratio, so the clip ranges are orders of magnitude below GRPO's 0.2
(config/rlhf_gspo_llama3_8b.yaml). `ppo` (per-token advantages) and `reinforce` raise at start-up.
`train/importance_sampling_level` is logged once (1 = sequence). At `token` (or absent) a run
launches exactly the kernels it launched before.

`model.lora.enabled` (`ppo.algorithm: grpo | ppo`; config/rlhf_grpo_lora_llama3_8b.yaml): the
policy is frozen and trains LoRA adapters only (attached after `parallelize`, before the engine: no
Adam state for the base). Rollouts run `generate(adapters="merged")`: the captured decode graph
reads weight copies built from W + (alpha / r) B A, refreshed in one HIP pass per projection once
per step, while the prompt prefill runs the live-adapter forward the update runs; the gap between
the two roundings is what `ppo.rollout_logprobs` measures and corrects. With no
`model.reference_model_name_or_path` (or the policy's own path) no second policy is loaded: the
reference is `LoRAReference(policy)`, the policy with its adapters switched off, and the checkpoint
holds the policy (`adapter.safetensors` + merged weights) and the reward model. The PPO critic stays
fully fine-tuned. `reinforce` with `model.lora`, and `ppo.frozen_fp8` with the shared reference,
raise at start-up. Without `model.lora` a run launches what it launched before.
"""
from __future__ import annotations

import argparse
import contextlib
import math
import random
from pathlib import Path
from typing import Dict, List, Optional

import torch

from ..data import read_jsonl
from ..models import (build_reward_model, build_value_model, generate, load_causal_lm,
                      load_reward_checkpoint)
from ..objectives import (action_mask, grpo_denominator, grpo_loss, grpo_rollout_stats, keep_row_grid, ppo_backward,
                          ppo_loss, ppo_rollout_stats, rlhf_loss, rollout_logp_grid, rollout_mismatch)
from ..ops.losses import GRPO_IMPORTANCE_LEVELS, GRPO_LOSS_TYPES, ROLLOUT_IS_LEVELS, ROLLOUT_IS_MODES
from ..parallel.dist import barrier, split_for_rank
from ..utils.checkpoint import save_state
from ..utils.config import add_config_args, config_from_args
from ..utils.logging import RunningLoss
from .common import lora_enabled, maybe_apply_lora, _tokenize_left, make_engine, parallelize, setup


def parse_args(argv=None) -> argparse.Namespace:
    return add_config_args(argparse.ArgumentParser(description="RLHF PPO loop")).parse_args(argv)


def load_prompts(cfg: Dict[str, str]) -> List[str]:
    source = cfg.get("source", "local")
    if source == "hf":
        try:
            from datasets import load_dataset

            ds = load_dataset(cfg["hf_path"], cfg.get("hf_name"), split=cfg.get("split", "train"))
            key = cfg.get("prompt_key", "prompt")
            return [row[key] for row in ds if row.get(key)]
        except Exception:
            if not (cfg.get("prompt_path") or cfg.get("path")):
                raise
    if source == "synthetic":
        from ..data.synthetic import synthetic_prompt_records

        return [r["prompt"] for r in synthetic_prompt_records(int(cfg.get("num_samples", 256)))]
    path = cfg.get("prompt_path") or cfg.get("path")
    return [r["prompt"] for r in read_jsonl(path) if r.get("prompt")]


ROLLOUT_LOGPROBS = ("off", "monitor", "old", "correct")


def rollout_logprobs_mode(ppo: Dict, algo: str) -> str:
    """`ppo.rollout_logprobs` (a bare YAML `off` arrives as False)."""
    v = ppo.get("rollout_logprobs", "off")
    mode = "off" if v is None or v is False else str(v).lower()
    if mode not in ROLLOUT_LOGPROBS:
        raise ValueError(f"ppo.rollout_logprobs must be {'|'.join(ROLLOUT_LOGPROBS)}, got {v!r}")
    if mode != "off" and algo == "reinforce":
        raise ValueError("ppo.rollout_logprobs needs token-level log-probs (ppo.algorithm: ppo|grpo); "
                         "the reinforce loop works on sequence log-probs")
    return mode


def generation_params(ppo: Dict) -> Dict:
    """`ppo.generation_params` as the rollouts use it: a copy with `do_sample` defaulted to True."""
    gen = dict(ppo.get("generation_params") or {"max_new_tokens": 256})
    gen.setdefault("do_sample", True)
    return gen


def draw_temperature(gen: Dict) -> float:
    """The temperature the rollouts are drawn at (`gen` from `generation_params`): its
    `temperature` when sampling, 1.0 for greedy decoding (no draw temperature)."""
    t = float(gen.get("temperature", 1.0))
    return t if gen["do_sample"] and t > 0 else 1.0


def logprob_temperature(ppo: Dict, algo: str) -> float:
    """`ppo.logprob_temperature` resolved to a float (`rollout` -> the draw temperature); bad
    values, and values the algorithm or the sampler cannot honour, raise."""
    v = ppo.get("logprob_temperature", 1.0)
    gen = generation_params(ppo)
    if isinstance(v, str) and v.strip().lower() == "rollout":
        t = draw_temperature(gen)
    else:
        if isinstance(v, bool) or v is None:
            raise ValueError(f"ppo.logprob_temperature must be a number > 0 or 'rollout', got {v!r}")
        try:
            t = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"ppo.logprob_temperature must be a number > 0 or 'rollout', got {v!r}") from None
    if not (math.isfinite(t) and t > 0):
        raise ValueError(f"ppo.logprob_temperature must be finite and > 0, got {v!r}")
    if t != 1.0 and algo == "reinforce":
        raise ValueError("ppo.logprob_temperature needs token-level log-probs (ppo.algorithm: ppo|grpo); "
                         "the reinforce loop works on sequence log-probs at temperature 1")
    if rollout_logprobs_mode(ppo, algo) != "off" and t not in (1.0, draw_temperature(gen)):
        raise ValueError(f"ppo.rollout_logprobs needs ppo.logprob_temperature 1.0 or the rollout temperature "
                         f"({draw_temperature(gen)}): the sampler returns no other log-prob; got {t!r}")
    return t


def keep_sampling_mask(ppo: Dict, algo: str, hardware: Optional[Dict] = None,
                       vocab_size: Optional[int] = None) -> bool:
    """`ppo.keep_sampling_mask` (default false); every combination it cannot honour raises.
    `hardware` (the config's section) and `vocab_size` are checked when given."""
    v = ppo.get("keep_sampling_mask", False)
    if v is None or v is False:
        return False
    if v is not True:
        raise ValueError(f"ppo.keep_sampling_mask must be true or false, got {v!r}")
    if algo == "reinforce":
        raise ValueError("ppo.keep_sampling_mask needs token-level log-probs (ppo.algorithm: ppo|grpo); "
                         "the reinforce loop works on sequence log-probs")
    gen = generation_params(ppo)
    top_k, top_p = int(gen.get("top_k", 0) or 0), float(gen.get("top_p", 1.0))
    if not (gen["do_sample"] and float(gen.get("temperature", 1.0)) > 0):
        raise ValueError("ppo.keep_sampling_mask needs sampled rollouts (generation_params.do_sample with "
                         "temperature > 0): greedy decoding keeps nothing")
    if top_k <= 0 and top_p >= 1.0:
        raise ValueError("ppo.keep_sampling_mask needs an active filter (generation_params.top_k > 0 or "
                         "top_p < 1): without one there is nothing to keep")
    if float(ppo.get("entropy_coef", 0.0) or 0.0) != 0 or bool(ppo.get("log_entropy", False)):
        raise ValueError("ppo.keep_sampling_mask does not support ppo.entropy_coef / ppo.log_entropy: the "
                         "entropy under the kept set is not implemented")
    hw = hardware or {}
    if int(hw.get("tp_size", 1) or 1) > 1 or int(hw.get("sp_size", 1) or 1) > 1 or hw.get("tp_sequence_parallel"):
        raise ValueError("ppo.keep_sampling_mask does not support tensor_parallel / sequence parallel runs "
                         "(hardware.tp_size, hardware.sp_size, hardware.tp_sequence_parallel)")
    if vocab_size is not None and int(vocab_size) % 8 != 0:
        raise ValueError(f"ppo.keep_sampling_mask needs a vocabulary size divisible by 8, got {vocab_size}")
    lp_t = logprob_temperature(ppo, algo)
    if rollout_logprobs_mode(ppo, algo) != "off" and lp_t != draw_temperature(gen):
        raise ValueError(f"ppo.keep_sampling_mask with ppo.rollout_logprobs needs ppo.logprob_temperature to be "
                         f"the generation temperature ({draw_temperature(gen)}; 'rollout'): the engine's kept-set "
                         f"log-prob exists at the draw temperature only; got {lp_t!r}")
    return True


def share_prefix_update(ppo: Dict, algo: str, hardware: Optional[Dict] = None, world: int = 1) -> bool:
    """`ppo.share_prefix_update` (default false): the GRPO update and stats forwards run on the
    prefix-shared layout, every group's prompt computed once (`shared_prefix_pack`). Every
    combination it cannot honour raises: another algorithm, tensor / sequence parallelism, and a
    minibatch or `update_micro_batch` that does not slice whole groups. `world`: the number of
    data-parallel replicas; the `batch_size / group_size` prompts of a step are split between them
    (`split_for_rank`) and each replica cuts its own rollouts into `num_minibatches`."""
    v = ppo.get("share_prefix_update", False)
    if v is None or v is False:
        return False
    if v is not True:
        raise ValueError(f"ppo.share_prefix_update must be true or false, got {v!r}")
    if algo != "grpo":
        raise ValueError(f"ppo.share_prefix_update needs group rollouts (ppo.algorithm: grpo), got ppo.algorithm: {algo}")
    hw = hardware or {}
    if int(hw.get("tp_size", 1) or 1) > 1 or int(hw.get("sp_size", 1) or 1) > 1 or hw.get("tp_sequence_parallel"):
        raise ValueError("ppo.share_prefix_update does not support tensor_parallel / sequence parallel runs "
                         "(hardware.tp_size, hardware.sp_size, hardware.tp_sequence_parallel)")
    group = int(ppo.get("group_size", 8))
    batch, nmb = int(ppo.get("batch_size", 64)), max(1, int(ppo.get("num_minibatches", 1)))
    micro = int(ppo.get("update_micro_batch", 0) or 0)
    world = max(1, int(world))
    per, extra = divmod(batch // max(group, 1), world)  # prompts per replica: per, or per + 1 on `extra` of them
    if group < 1 or batch % group or per % nmb or (extra and (per + 1) % nmb):
        raise ValueError(f"ppo.share_prefix_update: minibatches must hold whole groups; the ppo.batch_size ({batch}) "
                         f"/ ppo.group_size ({group}) prompts of a step, split over {world} data-parallel "
                         f"replica(s), do not divide into ppo.num_minibatches ({nmb}) on every replica")
    if micro and micro % group:
        raise ValueError(f"ppo.share_prefix_update: ppo.update_micro_batch ({micro}) must be a multiple of "
                         f"ppo.group_size ({group}): micro-batches slice whole groups")
    return True


def rollout_is_settings(ppo: Dict) -> Dict:
    """`ppo.rollout_is_cap / _floor / _level / _mode` (for `rollout_logprobs: correct`) as the
    `is_*` keyword arguments of `ppo_rollout_stats` / `grpo_rollout_stats`; bad values raise."""
    try:
        cap = float(ppo.get("rollout_is_cap", 2.0))
        floor = ppo.get("rollout_is_floor")
        floor = None if floor is None else float(floor)
    except (TypeError, ValueError):
        raise ValueError(f"ppo.rollout_is_cap / ppo.rollout_is_floor must be numbers, got "
                         f"{ppo.get('rollout_is_cap')!r} / {ppo.get('rollout_is_floor')!r}") from None
    level = str(ppo.get("rollout_is_level", "token")).lower()
    mode = str(ppo.get("rollout_is_mode", "truncate")).lower()
    if not (math.isfinite(cap) and cap > 0):
        raise ValueError(f"ppo.rollout_is_cap must be finite and > 0, got {cap!r}")
    if floor is not None and not 0 <= floor <= cap:
        raise ValueError(f"ppo.rollout_is_floor must lie in [0, rollout_is_cap = {cap}], got {floor!r}")
    if level not in ROLLOUT_IS_LEVELS:
        raise ValueError(f"ppo.rollout_is_level must be {'|'.join(ROLLOUT_IS_LEVELS)}, got {level!r}")
    if mode not in ROLLOUT_IS_MODES:
        raise ValueError(f"ppo.rollout_is_mode must be {'|'.join(ROLLOUT_IS_MODES)}, got {mode!r}")
    return {"is_cap": cap, "is_floor": floor, "is_level": level, "is_mode": mode}


def importance_sampling_level(ppo: Dict, algo: str) -> str:
    """`ppo.importance_sampling_level` (default token); an unknown value raises, and so does
    `sequence` outside `ppo.algorithm: grpo` (GSPO is defined for per-rollout advantages)."""
    v = ppo.get("importance_sampling_level", "token")
    level = str(v).lower()
    if level not in GRPO_IMPORTANCE_LEVELS:
        raise ValueError(f"ppo.importance_sampling_level must be {'|'.join(GRPO_IMPORTANCE_LEVELS)}, got {v!r}")
    if level == "sequence" and algo != "grpo":
        raise ValueError("ppo.importance_sampling_level: sequence needs per-rollout advantages "
                         f"(ppo.algorithm: grpo), got ppo.algorithm: {algo}")
    return level


def main(argv=None) -> int:
    args = parse_args(argv)
    config = config_from_args(args)
    lora_on = lora_enabled(config)
    model_cfg: Dict = config["model"]
    ppo = config["ppo"]
    ref_path = model_cfg.get("reference_model_name_or_path")
    # model.lora with no reference path, or the policy's own: the frozen reference of the k3 KL term
    # is the policy with its adapters switched off -- no second copy of the policy is loaded
    shared_ref = lora_on and (not ref_path or str(ref_path) == str(model_cfg["policy_model_name_or_path"]))
    if lora_on and str(ppo.get("algorithm", "reinforce")).lower() not in ("grpo", "ppo"):
        raise ValueError("model.lora in the RLHF trainer is supported for ppo.algorithm: grpo and ppo; the "
                         "reinforce loop works on sequence log-probs and has none of the rollout-mismatch "
                         "tooling (ppo.rollout_logprobs) that merged-adapter rollouts rely on")
    if shared_ref and ppo.get("frozen_fp8", False):
        raise ValueError("ppo.frozen_fp8 with the shared LoRA reference: the reference runs the policy's own "
                         "bf16 base weights; give a separate model.reference_model_name_or_path or drop "
                         "frozen_fp8 (the reward model keeps its own fp8 option only with a separate reference)")
    ctx = setup(config, "rlhf", default_seed=0)
    group = 1
    if str(ppo.get("algorithm", "reinforce")).lower() == "grpo":
        # ppo.batch_size stays the number of rollouts per step: whole groups of one prompt each
        group = int(ppo.get("group_size", 8))
        if group < 1 or int(ppo.get("batch_size", 64)) % group:
            raise ValueError(f"ppo.batch_size ({ppo.get('batch_size', 64)}) must be divisible by "
                             f"ppo.group_size ({group})")
        if str(ppo.get("loss_type", "sequence")).lower() not in GRPO_LOSS_TYPES:
            raise ValueError(f"ppo.loss_type must be {'|'.join(GRPO_LOSS_TYPES)}, got {ppo.get('loss_type')!r}")
    is_level = importance_sampling_level(ppo, str(ppo.get("algorithm", "reinforce")).lower())
    policy = load_causal_lm(model_cfg["policy_model_name_or_path"],
                            gradient_checkpointing=model_cfg.get("gradient_checkpointing", True),
                            device=ctx.device, seed=ctx.seed)
    ref = None
    if not shared_ref:
        ref = load_causal_lm(model_cfg["reference_model_name_or_path"], gradient_checkpointing=False,
                             device=ctx.device, seed=ctx.seed)
        ref.model.eval().requires_grad_(False)
    rcfg = config.get("reward_model", {}) or {}
    rbase = rcfg.get("base_model_name_or_path", model_cfg["policy_model_name_or_path"])
    rpath = rcfg.get("path")
    if rpath and Path(rpath).is_dir() and (Path(rpath) / "config.json").exists() and "base_model_name_or_path" not in rcfg:
        rbase = rpath
    rm, rtok = build_reward_model(rbase, pooling="last_token", dropout=0.1, device=ctx.device, seed=ctx.seed)
    if rpath and Path(rpath).exists():
        ctx.log(f"Loaded reward weights from {load_reward_checkpoint(rm, rpath)}")
    rm.eval().requires_grad_(False)
    if ppo.get("frozen_fp8", False):  # reference + reward model on the fp8 inference GEMMs (opt-in)
        from ..ops import enable_fp8_inference

        enable_fp8_inference(ref.model)
        enable_fp8_inference(rm.backbone)
    for m in (policy.model, rm) if shared_ref else (policy.model, ref.model, rm):
        parallelize(ctx, m)
    maybe_apply_lora(ctx, policy.model, model_cfg["policy_model_name_or_path"])
    if shared_ref:
        import types

        from ..models.lora import LoRAReference

        # (`ref.model` is what the loops read; `ref.saved` what they checkpoint next to the policy)
        ref = types.SimpleNamespace(model=LoRAReference(policy.model), saved=[])
        ctx.log("RLHF reference: the policy with its LoRA adapters switched off (no second model)")
    else:
        ref.saved = [ref.model]

    prompts = load_prompts(config["sampling"])
    gen = generation_params(ppo)
    engine = make_engine(ctx, policy.model, lr=ppo.get("learning_rate", 1e-6), betas=(0.9, 0.95),
                         weight_decay=ppo.get("weight_decay", 0.01),
                         max_grad_norm=ppo.get("max_grad_norm", 1.0))
    steps = ppo.get("steps", 1024)
    batch_size = ppo.get("batch_size", 64)
    kl_coef = ppo.get("kl_coef", 0.1)
    max_len = model_cfg.get("max_seq_length", 1024)
    tok = policy.tokenizer
    rng = random.Random(ctx.seed)
    gen_g = torch.Generator(device=ctx.device)
    gen_g.manual_seed(ctx.seed * 1000 + (ctx.mesh.dp_rank if ctx.mesh is not None else ctx.dist.rank))
    running = RunningLoss()
    log_every = (config.get("logging", {}) or {}).get("log_every_steps", 10)
    algo = str(ppo.get("algorithm", "reinforce")).lower()
    if algo not in ("reinforce", "ppo", "grpo"):
        raise ValueError(f"ppo.algorithm must be reinforce|ppo|grpo, got {algo!r}")
    want_logp = rollout_logprobs_mode(ppo, algo) != "off"
    rollout_is_settings(ppo)  # bad ppo.rollout_is_* values fail here, before any rollout
    lp_temp = logprob_temperature(ppo, algo)  # likewise
    keep_on = keep_sampling_mask(ppo, algo, ctx.hw, policy.model.cfg.vocab_size)  # likewise
    share_prefix_update(ppo, algo, ctx.hw, ctx.dp_size)  # likewise

    # reward inputs built on the device when the reward tokenizer equals the policy's (no
    # decode / re-tokenise round trip through the host; training/handoff.py), else the
    # reference's text path (src/training/train_rlhf.py:131-147)
    from .handoff import RewardHandoff

    handoff = RewardHandoff(tok, rtok, policy.model.cfg.vocab_size, ctx.device, max_len,
                            ppo.get("reward_handoff", "auto"),
                            validate_every=int(ppo.get("reward_handoff_validate_every", 16)))
    ctx.log(f"reward hand-off: {'device ids' if handoff.device_path else 'decode + re-tokenise'}")

    def rollout():
        # grpo: batch_size / group_size prompts, split by prompt (a group never straddles ranks)
        batch_prompts = rng.sample(prompts, k=min(batch_size // group, len(prompts)))
        mine = split_for_rank(batch_prompts)
        ids, am = _tokenize_left(tok, mine, max_len, ctx.device)
        seqs, mask, *rlp = generate(policy.model, ids, am, max_new_tokens=gen.get("max_new_tokens", 256),
                                    do_sample=gen["do_sample"], temperature=gen.get("temperature", 1.0),
                                    top_p=gen.get("top_p", 1.0), top_k=gen.get("top_k", 0),
                                    pad_token_id=tok.pad_token_id, eos_token_id=getattr(tok, "eos_token_id", None),
                                    generator=gen_g, return_mask=True,
                                    weight_dtype=ppo.get("rollout_weight_dtype", "bf16"),
                                    num_return_sequences=group, share_prefill=bool(ppo.get("share_prefill", True)),
                                    group_attention=bool(ppo.get("group_attention", False)),
                                    return_logprobs=want_logp,
                                    # live adapters: the decode graph reads weight copies built from
                                    # W + s B A, refreshed once per step (models.generation.generate)
                                    adapters="merged" if lora_on else None,
                                    logprob_temperature=lp_temp if want_logp and (lp_temp != 1.0 or keep_on) else None,
                                    **({"return_keep_mask": True} if keep_on else {}))
        keep = rlp.pop() if keep_on else None  # uint8 [S, n, V / 8], last in the returned tuple
        if group > 1:  # the reward hand-off sees one prompt row per rollout
            mine = [p for p in mine for _ in range(group)]
            ids, am = ids.repeat_interleave(group, 0), am.repeat_interleave(group, 0)
        r_ids, r_mask = handoff(mine, ids, am, seqs, mask)
        with torch.no_grad():
            scores = rm(r_ids, r_mask)
        # the sampling engine's token log-probs in the trainer's [S, T] action grid, or None
        rlp = rollout_logp_grid(rlp[0], ids.shape[1], seqs.shape[1]) if want_logp else None
        return seqs, mask, scores, ids.shape[1], rlp, keep

    policy.model.train()
    if algo == "ppo":
        return _ppo_loop(ctx, config, ppo, policy, ref, rm, rollout, engine, steps, kl_coef, log_every)
    if algo == "grpo":
        return _grpo_loop(ctx, config, ppo, policy, ref, rm, rollout, engine, steps, group, log_every, is_level)
    micro = int(ppo.get("update_micro_batch", 0) or 0)
    pending = rollout()
    for step in range(steps):
        seqs, mask, scores, _, _, _ = pending
        loss, m = reinforce_update(policy.model, ref.model, engine, seqs, mask, scores, kl_coef, micro)
        if ppo.get("async_rollouts", False) and step + 1 < steps:
            # the bucketed reduce-scatter launched by the backward hooks is in flight on RCCL's
            # stream; generating the next rollouts (pre-update weights) overlaps it
            pending = rollout()
            engine.step()
        else:
            engine.step()
            if step + 1 < steps:
                pending = rollout()
        running.update(loss.detach())
        if (step + 1) % log_every == 0:
            ctx.logger.log({"train/loss": running.average, "train/kl": m["kl"],
                            "train/reward_mean": scores.mean(), "train/grad_norm": engine.last_grad_norm,
                            "train/comm_exposed_ms": engine.comm_timer.last_step_ms()},
                           step + 1)
            running = RunningLoss()
    barrier()
    save_state(config["logging"]["output_dir"], [policy.model, *ref.saved, rm], engine, None, steps, tok)
    ctx.log("RLHF PPO loop complete")
    ctx.logger.close()
    return 0


def micro_bounds(n: int, micro: int):
    """[start, stop) of each update micro-batch. A ragged tail (n % micro != 0) is folded into the
    previous micro-batch instead of standing alone: a 1-rollout micro-batch's mean baseline is its
    own reward, so its advantage (and policy gradient) would be exactly zero while it still
    carried weight."""
    b = [(s, min(n, s + micro)) for s in range(0, n, micro)]
    if len(b) > 1 and b[-1][1] - b[-1][0] < micro:
        b[-2:] = [(b[-2][0], n)]
    return b


def reinforce_update(policy, ref, engine, seqs, mask, scores, kl_coef: float, micro: int = 0):
    """Backward of the KL-penalised policy-gradient loss over this rank's rollouts.

    micro > 0 (`ppo.update_micro_batch`): gradient-accumulated micro-batches of `micro` rollouts,
    each with its own mean baseline and weighted by its share of the rollouts -- the gradient of
    a job with that many rollouts per process (the reference splits `ppo.batch_size` across
    processes and takes `rewards.mean()` per process, src/training/train_rlhf.py:114,151, then
    DDP averages), and no activation recompute is needed for a large one-GPU batch.
    Returns (loss, metrics) like `rlhf_loss`."""
    n = seqs.shape[0]
    if micro <= 0 or micro >= n:
        loss, m = rlhf_loss(policy, ref, seqs, mask, scores, kl_coef)
        loss.backward()
        return loss, m
    bounds = micro_bounds(n, micro)
    tot, kl = 0.0, 0.0
    for i, (s0, s1) in enumerate(bounds):
        sl = slice(s0, s1)
        w = (sl.stop - sl.start) / n
        ctx = engine.no_sync() if i < len(bounds) - 1 else contextlib.nullcontext()
        with ctx:
            loss, m = rlhf_loss(policy, ref, seqs[sl], mask[sl], scores[sl], kl_coef)
            (loss * w).backward()
        tot = tot + loss.detach() * w
        kl = kl + m["kl"] * w
    return tot, {"kl": kl}


# the per-rollout entries of the GRPO stats that minibatches and micro-batches slice
GRPO_ROWS = ("act", "advantages", "ref_logp", "old_logp", "is_weight", "keep_rows")


def grpo_update(policy, engine, seqs, mask, stats, clip_low: float, clip_high, beta: float,
                loss_type: str, max_len, micro: int = 0, entropy_coef: float = 0.0,
                log_entropy: bool = False, temperature: float = 1.0, keep=None,
                importance_level: str = "token", shared_prefix=None):
    """Backward of the GRPO loss over one minibatch of rollouts. micro > 0
    (`ppo.update_micro_batch`): gradient-accumulated micro-batches of `micro` rollouts that share
    the whole minibatch's divisor (`denom`, a device tensor: no host sync), so their gradients sum
    to the full minibatch's; every micro-batch but the last runs under `engine.no_sync()`. The
    entropy bonus (`ppo.entropy_coef`) is likewise normalised by the whole minibatch's
    action-token count. `stats["is_weight"]` (optional) is sliced with the other per-rollout
    entries. `temperature`: the log-prob temperature of `grpo_loss`. `keep`: the rollout batch's
    whole sampling mask (`stats["keep_rows"]`, sliced with the rows, indexes it). `importance_level`:
    `ppo.importance_sampling_level`; micro-batches slice whole rows, so a row's sequence-level ratio
    never straddles two of them. `shared_prefix=(G, prompt_len)` (`ppo.share_prefix_update`): the
    policy runs on the prefix-shared layout; the minibatch and every micro-batch must then hold
    whole groups (ValueError). Returns (loss, metrics) with token-weighted metric means."""
    n = seqs.shape[0]
    rows = GRPO_ROWS
    if shared_prefix is not None and (n % shared_prefix[0] or (0 < micro < n and micro % shared_prefix[0])):
        raise ValueError(f"share_prefix_update: a minibatch of {n} rollouts in micro-batches of {micro} does not "
                         f"slice whole groups of {shared_prefix[0]}")
    if micro <= 0 or micro >= n:
        loss, m = grpo_loss(policy, seqs, mask, stats, clip_low, clip_high, beta, loss_type, max_len,
                            entropy_coef=entropy_coef, log_entropy=log_entropy, temperature=temperature, keep=keep,
                            importance_level=importance_level, shared_prefix=shared_prefix)
        loss.backward()
        return loss.detach(), m
    denom = grpo_denominator(stats["act"], loss_type, max_len)
    bounds = micro_bounds(n, micro)
    tot, acc = 0.0, {"clipfrac": 0.0, "approx_kl": 0.0, "kl_ref": 0.0}
    if entropy_coef != 0 or log_entropy:
        acc["entropy"] = 0.0
    tokens = stats["act"].sum().clamp(min=1)
    for i, (s0, s1) in enumerate(bounds):
        mb = {k: (stats[k][s0:s1] if stats.get(k) is not None else None) for k in rows}
        ctx = engine.no_sync() if i < len(bounds) - 1 else contextlib.nullcontext()
        with ctx:
            loss, m = grpo_loss(policy, seqs[s0:s1], mask[s0:s1], mb, clip_low, clip_high, beta, loss_type,
                                max_len, denom, entropy_coef, log_entropy, tokens, temperature=temperature,
                                keep=keep, importance_level=importance_level, shared_prefix=shared_prefix)
            loss.backward()
        tot = tot + loss.detach()
        for k in acc:
            acc[k] = acc[k] + m[k] * m["tokens"] / tokens
    return tot, {"kl": acc["kl_ref"], "tokens": tokens, **acc}


def _grpo_loop(ctx, config, ppo, policy, ref, rm, rollout, engine, steps, group, log_every,
               importance_level: str = "token") -> int:
    """Critic-free group-relative policy optimisation (`ppo.algorithm: grpo`)."""
    clip_low = float(ppo.get("clip_range", 0.2))
    clip_high = ppo.get("clip_range_high")
    clip_high = float(clip_high) if clip_high is not None else None
    beta = float(ppo.get("kl_coef", 0.04))
    loss_type = str(ppo.get("loss_type", "sequence")).lower()
    scale_std = bool(ppo.get("scale_rewards", True))
    gen_len = int((ppo.get("generation_params", {}) or {}).get("max_new_tokens", 256))
    epochs, nmb = int(ppo.get("ppo_epochs", 1)), max(1, int(ppo.get("num_minibatches", 1)))
    micro = int(ppo.get("update_micro_batch", 0) or 0)
    overlap = bool(ppo.get("async_rollouts", False))
    entropy_coef, log_entropy = float(ppo.get("entropy_coef", 0.0) or 0.0), bool(ppo.get("log_entropy", False))
    need_old = epochs * nmb > 1  # a single update per rollout batch is on-policy: rho = 1
    lp_mode = rollout_logprobs_mode(ppo, "grpo")
    is_kw = rollout_is_settings(ppo) if lp_mode == "correct" else {}
    lp_temp = logprob_temperature(ppo, "grpo")
    log_temp = "logprob_temperature" in ppo  # logged once, and only when the key is set
    log_level = importance_level == "sequence"  # logged once
    share = share_prefix_update(ppo, "grpo", ctx.hw, ctx.dp_size)
    log_share = share  # logged once
    rows = GRPO_ROWS
    running = RunningLoss()
    pending = rollout()
    for step in range(steps):
        seqs, mask, scores, tp, rlp, keep = pending
        kkw = {}
        if keep is not None:  # every log-prob of the step over the set its token was drawn from
            kkw = {"keep": keep, "keep_rows": keep_row_grid(action_mask(mask, tp), tp, keep.shape[1])}
        # monitor: the trainer's own old-policy log-probs are computed even on-policy, to compare;
        # old: the rollout engine's ARE the old-policy log-probs (rho reflects fp8 / stale /
        # rounding mismatch, which the clip handles) and the policy forward is skipped;
        # correct: the trainer's own stay the old-policy log-probs (computed even on-policy) and
        # the gap goes into detached truncated importance weights on every action token
        stats = grpo_rollout_stats(policy.model, ref.model, seqs, mask, tp, scores, group, beta, scale_std,
                                   need_old or lp_mode == "monitor",
                                   old_logp=rlp if lp_mode == "old" else None,
                                   rollout_logp=rlp if lp_mode == "correct" else None, **is_kw,
                                   temperature=lp_temp, **kkw, **({"shared_prefix": (group, tp)} if share else {}))
        mism = rollout_mismatch(rlp, stats["old_logp"], stats["act"]) if lp_mode in ("monitor", "correct") else {}
        mism.update(stats.get("rollout_is", {}))
        if lp_mode in ("monitor", "correct") and not need_old:
            stats["old_logp"] = None  # the update itself stays the on-policy one (rho = 1 exactly)
        S = seqs.shape[0]
        bounds = [(i * S // nmb, (i + 1) * S // nmb) for i in range(nmb)]
        for ep in range(epochs):
            for mi, (a, b) in enumerate(bounds):
                if b <= a:
                    continue
                mb = {k: (stats[k][a:b] if stats.get(k) is not None else None) for k in rows}
                loss, m = grpo_update(policy.model, engine, seqs[a:b], mask[a:b], mb, clip_low, clip_high,
                                      beta, loss_type, gen_len, micro, entropy_coef, log_entropy, lp_temp,
                                      keep=keep, importance_level=importance_level,
                                      **({"shared_prefix": (group, tp)} if share else {}))
                last = ep == epochs - 1 and mi == len(bounds) - 1
                if last and overlap and step + 1 < steps:
                    pending = rollout()  # overlaps the in-flight gradient collectives (see _ppo_loop)
                engine.step()
                running.update(loss)
        if not overlap and step + 1 < steps:
            pending = rollout()
        if (step + 1) % log_every == 0:
            ctx.logger.log({"train/loss": running.average, "train/kl": m["kl"],
                            "train/reward_mean": stats["scores"].mean(),
                            "train/reward_std": stats["reward_std"],
                            "train/frac_zero_std": stats["frac_zero_std"],
                            "train/clipfrac": m["clipfrac"], "train/approx_kl": m["approx_kl"],
                            **({"train/entropy": m["entropy"]} if "entropy" in m else {}),
                            **{f"train/{k}": v for k, v in mism.items()},
                            **({"train/logprob_temperature": lp_temp} if log_temp else {}),
                            **({"train/importance_sampling_level":
                                GRPO_IMPORTANCE_LEVELS.index(importance_level)} if log_level else {}),
                            **({"train/share_prefix_update": 1} if log_share else {}),
                            "train/grad_norm": engine.last_grad_norm,
                            "train/comm_exposed_ms": engine.comm_timer.last_step_ms()}, step + 1)
            running, log_temp, log_level, log_share = RunningLoss(), False, False, False
    barrier()
    save_state(config["logging"]["output_dir"], [policy.model, *ref.saved, rm], engine, None, steps,
               policy.tokenizer)
    ctx.log("RLHF GRPO loop complete")
    ctx.logger.close()
    return 0


def _ppo_loop(ctx, config, ppo, policy, ref, rm, rollout, engine, steps, kl_coef, log_every) -> int:
    """Token-level actor-critic PPO (`ppo.algorithm: ppo`)."""
    model_cfg = config["model"]
    ccfg = config.get("critic", {}) or {}
    rcfg = config.get("reward_model", {}) or {}
    cbase = ccfg.get("base_model_name_or_path") or rcfg.get("base_model_name_or_path") \
        or model_cfg["policy_model_name_or_path"]
    critic, _ = build_value_model(cbase, device=ctx.device, seed=ctx.seed + 1,
                                  gradient_checkpointing=ccfg.get("gradient_checkpointing",
                                                                  model_cfg.get("gradient_checkpointing", True)))
    parallelize(ctx, critic)
    critic.train()
    critic_engine = make_engine(ctx, critic, lr=ccfg.get("learning_rate", ppo.get("learning_rate", 1e-6)),
                                betas=(0.9, 0.95), weight_decay=ppo.get("weight_decay", 0.01),
                                max_grad_norm=ppo.get("max_grad_norm", 1.0))
    gamma, lam = float(ppo.get("gamma", 1.0)), float(ppo.get("lam", 0.95))
    clip, vclip = float(ppo.get("clip_range", 0.2)), float(ppo.get("value_clip_range", 0.2))
    vf_coef = float(ppo.get("vf_coef", 0.1))
    epochs, nmb = int(ppo.get("ppo_epochs", 1)), max(1, int(ppo.get("num_minibatches", 1)))
    overlap = bool(ppo.get("async_rollouts", False))
    entropy_coef, log_entropy = float(ppo.get("entropy_coef", 0.0) or 0.0), bool(ppo.get("log_entropy", False))
    lp_mode = rollout_logprobs_mode(ppo, "ppo")
    is_kw = rollout_is_settings(ppo) if lp_mode == "correct" else {}
    lp_temp = logprob_temperature(ppo, "ppo")
    log_temp = "logprob_temperature" in ppo  # logged once, and only when the key is set
    running = RunningLoss()
    pending = rollout()
    for step in range(steps):
        seqs, mask, scores, tp, rlp, keep = pending
        kkw = {}
        if keep is not None:  # every log-prob of the step over the set its token was drawn from
            kkw = {"keep": keep, "keep_rows": keep_row_grid(action_mask(mask, tp), tp, keep.shape[1])}
        stats = ppo_rollout_stats(policy.model, ref.model, critic, seqs, mask, tp, scores, kl_coef,
                                  gamma, lam, old_logp=rlp if lp_mode == "old" else None,
                                  rollout_logp=rlp if lp_mode == "correct" else None, **is_kw,
                                  temperature=lp_temp, **kkw)
        mism = rollout_mismatch(rlp, stats["old_logp"], stats["act"]) if lp_mode in ("monitor", "correct") else {}
        mism.update(stats.get("rollout_is", {}))
        S = seqs.shape[0]
        bounds = [(i * S // nmb, (i + 1) * S // nmb) for i in range(nmb)]
        for ep in range(epochs):
            for mi, (a, b) in enumerate(bounds):
                if b <= a:
                    continue
                mb = {k: v[a:b] for k, v in stats.items() if k in ("old_logp", "values", "advantages", "returns", "act", "is_weight", "keep_rows")}
                loss, m = ppo_loss(policy.model, critic, seqs[a:b], mask[a:b], mb, clip, vclip, vf_coef,
                                   entropy_coef, log_entropy, temperature=lp_temp, keep=keep)
                ppo_backward(loss)
                last = ep == epochs - 1 and mi == len(bounds) - 1
                if last and overlap and step + 1 < steps:
                    # overlaps the in-flight ZeRO-0/1 bucket collectives (they are waited on in
                    # step()); an FSDP engine has already drained its reduce-scatters in its
                    # end-of-backward callback, so there the rollout only runs ahead of step()
                    pending = rollout()
                engine.step()
                critic_engine.step()
                running.update(loss.detach())
        if not overlap and step + 1 < steps:
            pending = rollout()
        if (step + 1) % log_every == 0:
            ctx.logger.log({"train/loss": running.average, "train/kl": stats["kl"].mean(),
                            "train/reward_mean": stats["scores"].mean(),
                            "train/policy_loss": m["policy_loss"], "train/value_loss": m["value_loss"],
                            "train/clipfrac": m["clipfrac"], "train/approx_kl": m["approx_kl"],
                            **({"train/entropy": m["entropy"]} if "entropy" in m else {}),
                            **{f"train/{k}": v for k, v in mism.items()},
                            **({"train/logprob_temperature": lp_temp} if log_temp else {}),
                            "train/grad_norm": engine.last_grad_norm,
                            "train/comm_exposed_ms": engine.comm_timer.last_step_ms()}, step + 1)
            running, log_temp = RunningLoss(), False
    barrier()
    out = save_state(config["logging"]["output_dir"], [policy.model, *ref.saved, rm, critic], engine, None,
                     steps, policy.tokenizer)
    from ..utils.stream_st import save_streamed

    cst = critic_engine.optimizer_state()
    save_streamed(Path(out) / f"critic_optimizer_shard_{ctx.dist.rank}.safetensors",
                  {k: v for k, v in cst.items() if isinstance(v, torch.Tensor) or v is None},
                  {k: (list(v) if isinstance(v, tuple) else v) for k, v in cst.items()
                   if not (isinstance(v, torch.Tensor) or v is None)})
    ctx.log("RLHF PPO (actor-critic) loop complete")
    ctx.logger.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
