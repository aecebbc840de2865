"""The package's fp32 CPU branch (`ops.*`, `optim.adamw.*` on CPU tensors) run on the inputs of
tests/_refs64.py, one dict of fp32 outputs per op with the keys of the matching fp64 reference.
Gradients come from autograd through the CPU branch. test_refs64_cpu.py ties these to the fp64
references; the GPU modules take E32 (the fp32 branch's own error against fp64) from them."""
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import logprob as lpmod
from distributed_llm_alignment_amd.ops import losses
from distributed_llm_alignment_amd.optim import adamw as opt

import _refs64 as R


def _leaf(x):
    return x.clone().requires_grad_(True)


def seq_reduce(lp, mask, coef, mean):
    x = _leaf(lp)
    out = lpmod.seq_reduce(x, mask, mean=mean)
    (g,) = torch.autograd.grad(out, x, coef)
    return {"out": out.detach(), "grad": g}


def dpo(pol, ref, beta, ls):
    B = pol.numel() // 2
    x = _leaf(pol)
    loss, met = losses.dpo_loss(x[:B], x[B:], ref[:B], ref[B:], beta=beta, label_smoothing=ls)
    (g,) = torch.autograd.grad(loss, x)
    metrics = torch.stack([met["rewards/chosen"], met["rewards/rejected"], met["rewards/accuracy"],
                           met["rewards/margin"]])
    return {"loss": loss.detach(), "dpol": g, "rewards": met["rewards_per_seq"], "metrics": metrics}


def pairwise(sc, sr):
    a, b = _leaf(sc), _leaf(sr)
    loss, acc = losses.pairwise_loss(a, b, return_accuracy=True)
    dsc, dsr = torch.autograd.grad(loss, (a, b))
    return {"loss": loss.detach(), "dsc": dsc, "dsr": dsr, "acc": acc}


def klpg(lp, lr, reward, kl_coef=R.KL_COEF):
    x = _leaf(lp)
    loss, klm, adv = losses.kl_penalty_pg(x, lr, reward, kl_coef=kl_coef)
    (g,) = torch.autograd.grad(loss, x)
    return {"loss": loss.detach(), "kl_mean": klm.detach(), "adv": adv.detach(), "dlp": g}


def gae(r, v, m, gamma, lam):
    adv, ret = losses.gae(r, v, m, gamma=gamma, lam=lam)
    return {"adv": adv, "ret": ret}


def ppo_policy(lp, old, adv, m, eps=R.PPO_EPS):
    x = _leaf(lp)
    loss, met = losses.ppo_policy_loss(x, old, adv, m, clip_eps=eps)
    (g,) = torch.autograd.grad(loss, x)
    return {"loss": loss.detach(), "dlp": g, "clipfrac": met["clipfrac"], "approx_kl": met["approx_kl"],
            "count": m.sum()}


def ppo_value(val, old, ret, m, clip=R.PPO_VCLIP):
    x = _leaf(val)
    loss = losses.ppo_value_loss(x, old, ret, m, clip=clip)
    (g,) = torch.autograd.grad(loss, x)
    return {"loss": loss.detach(), "dval": g}


def group_advantages(scores, G, scale_std, eps=R.GROUP_EPS):
    adv, sd = losses._ref_group_advantages(scores, G, scale_std, eps)
    adv2, met = losses.group_advantages(scores, G, scale_std, eps)
    assert torch.equal(adv, adv2)
    return {"adv": adv, "sd": sd}


def grpo(lp, old, ref, adv, m, beta, mode, max_len=None, denom=None, clip=R.GRPO_CLIP):
    x = _leaf(lp)
    dn = None if denom is None else torch.tensor([denom], dtype=torch.float32)
    loss, met = losses.grpo_loss(x, old, ref, adv, m, clip_low=clip[0], clip_high=clip[1], beta=beta,
                                 loss_type=mode, max_len=max_len, denom=dn)
    (g,) = torch.autograd.grad(loss, x)
    metrics = torch.stack([met["clipfrac"], met["approx_kl"], met["kl_ref"], met["tokens"]])
    return {"loss": loss.detach(), "dlp": g, "metrics": metrics}


def adamw(w, grad, m, v, step, wd, clip=None, grad_scale=1.0):
    """One fp32 step on a master copy -> (w, m, v) (new tensors)."""
    w, m, v = w.clone(), m.clone(), v.clone()
    c = None if clip is None else torch.tensor(clip, dtype=torch.float32)
    hp = R.ADAMW_HP
    opt.adamw_update(None, w, grad, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, step, clip=c,
                     grad_scale=grad_scale)
    return w, m, v


def grad_sumsq(g, out, accumulate):
    return opt.grad_sumsq(g, out, accumulate=accumulate)


def clip_coef(sumsq, max_norm):
    return opt.clip_coefficient(sumsq, max_norm)


def logprob(x, tgt):
    """The formula of `_ref_linear_logprob` on given logits (fp32 log-softmax of the bf16 logits)."""
    z = x.float()
    lse = torch.logsumexp(z, -1)
    lp = z.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1) - lse
    return {"logp": torch.where(tgt >= 0, lp, torch.zeros_like(lp)), "lse": lse}


def logprob_bwd(x, tgt, g):
    z = x.float()
    p = torch.softmax(z, -1)
    onehot = torch.zeros_like(z)
    onehot.scatter_(-1, tgt.clamp(min=0).unsqueeze(-1), 1.0)
    out = g.unsqueeze(-1) * (onehot - p) * (tgt >= 0).float().unsqueeze(-1)
    return out.masked_fill(z == R.NINF, 0.0)


def ensemble_kl(s, t, g):
    x = _leaf(s.float())
    kl = ops.ensemble_kl(x, t.float())
    (gr,) = torch.autograd.grad(kl, x, g)
    return {"kl": kl.detach(), "grad": gr}
