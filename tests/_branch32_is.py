"""The package's fp32 CPU branch of the importance-weight op and the weighted surrogates on the
inputs of tests/_refs64_is.py, one dict of fp32 outputs per op with the keys of the matching fp64
reference (the counterpart of tests/_branch32.py). The GPU module takes E32 from these."""
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd.ops import losses

import _refs64 as R
import _refs64_is as RI

IS_KEYS = ("is_mean", "is_frac_high", "is_frac_low", "is_ess", "tokens")


def _leaf(x):
    return x.clone().requires_grad_(True)


def is_weights(trainer_lp, rollout_lp, m, level, mode, cap=RI.IS_CAP, floor=RI.IS_FLOOR):
    w, met = losses.rollout_is_weights(trainer_lp, rollout_lp, m, cap=cap, floor=floor, level=level, mode=mode)
    return {"w": w, "metrics": torch.stack([met[k] for k in IS_KEYS])}


def grpo_w(lp, old, ref, adv, m, w, beta, mode, max_len=None, denom=None, clip=R.GRPO_CLIP):
    x = _leaf(lp)
    dn = None if denom is None else torch.tensor([denom], dtype=torch.float32)
    loss, met = losses.grpo_loss(x, old, ref, adv, m, clip_low=clip[0], clip_high=clip[1], beta=beta,
                                 loss_type=mode, max_len=max_len, denom=dn, is_weight=w)
    (g,) = torch.autograd.grad(loss, x)
    metrics = torch.stack([met["clipfrac"], met["approx_kl"], met["kl_ref"], met["tokens"]])
    return {"loss": loss.detach(), "dlp": g, "metrics": metrics}


def ppo_policy_w(lp, old, adv, m, w, eps=R.PPO_EPS):
    x = _leaf(lp)
    loss, met = losses.ppo_policy_loss(x, old, adv, m, clip_eps=eps, is_weight=w)
    (g,) = torch.autograd.grad(loss, x)
    return {"loss": loss.detach(), "dlp": g, "clipfrac": met["clipfrac"], "approx_kl": met["approx_kl"],
            "count": m.sum()}
