"""Sequence-level alignment objectives as fused HIP epilogue kernels.

Each GPU path is one launch computing loss, gradient coefficients and metrics together (no
host sync); CPU paths are the literal reference formulas:
  * dpo_loss        src/training/train_dpo.py:42-44
  * pairwise_loss   src/models/reward_model.py:67-68
  * kl_penalty_pg   src/training/train_rlhf.py:149-153
  * ensemble_kl     src/training/train_distill.py:127-144
  * gae / ppo_policy_loss / ppo_value_loss: token-level actor-critic PPO (north-star config; the
    reference's REINFORCE above stays the default RLHF algorithm)
  * group_advantages / grpo_loss: critic-free group-relative policy optimisation (GRPO and its
    DAPO / Dr. GRPO normalisations, and GSPO's sequence-level ratio; not in the reference)
  * rollout_is_weights: truncated importance weights for the rollout engine / trainer mismatch,
    taken by grpo_loss / ppo_policy_loss as `is_weight` (not in the reference)
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _ext


# ------------------------------------------------------------------------------------- DPO
class _DPOFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pol, ref, beta, label_smoothing):
        loss, dpol, rewards, metrics = _ext.require().dpo_loss(pol, ref, beta, label_smoothing)
        ctx.save_for_backward(dpol)
        ctx.mark_non_differentiable(rewards, metrics)
        return loss, rewards, metrics

    @staticmethod
    def backward(ctx, gloss, _gr, _gm):
        (dpol,) = ctx.saved_tensors
        return dpol * gloss, None, None, None


def dpo_loss(policy_chosen: torch.Tensor, policy_rejected: torch.Tensor, ref_chosen: torch.Tensor,
             ref_rejected: torch.Tensor, beta: float = 0.1, label_smoothing: float = 0.0
             ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """-logsigmoid(beta*((pc-pr)-(rc-rr))).mean() (+ optional conservative label smoothing).

    Returns (loss, metrics) where metrics holds device tensors: chosen/rejected implicit
    rewards, reward accuracy and margin (no host sync)."""
    pol = torch.cat([policy_chosen, policy_rejected]).float().contiguous()
    ref = torch.cat([ref_chosen, ref_rejected]).float().detach().contiguous()
    B = policy_chosen.shape[0]
    if _ext.use_native(pol):
        loss, rewards, m = _DPOFn.apply(pol, ref, float(beta), float(label_smoothing))
        metrics = {"rewards/chosen": m[0], "rewards/rejected": m[1], "rewards/accuracy": m[2],
                   "rewards/margin": m[3], "rewards_per_seq": rewards}
        return loss, metrics
    z = beta * ((pol[:B] - pol[B:]) - (ref[:B] - ref[B:]))
    loss = (-(1 - label_smoothing) * F.logsigmoid(z) - label_smoothing * F.logsigmoid(-z)).mean()
    rc = (beta * (pol[:B] - ref[:B])).detach()
    rr = (beta * (pol[B:] - ref[B:])).detach()
    metrics = {"rewards/chosen": rc.mean(), "rewards/rejected": rr.mean(),
               "rewards/accuracy": (rc > rr).float().mean(), "rewards/margin": z.detach().mean(),
               "rewards_per_seq": torch.cat([rc, rr])}
    return loss, metrics


# ------------------------------------------------------------------------------ pairwise RM
class _PairwiseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sc, sr):
        loss, dsc, dsr, acc = _ext.require().pairwise_loss(sc, sr)
        ctx.save_for_backward(dsc, dsr)
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        dsc, dsr = ctx.saved_tensors
        return dsc * gloss, dsr * gloss


def pairwise_loss(chosen_scores: torch.Tensor, rejected_scores: torch.Tensor,
                  return_accuracy: bool = False):
    """Bradley-Terry: -logsigmoid(s_c - s_r).mean()."""
    sc = chosen_scores.float().contiguous()
    sr = rejected_scores.float().contiguous()
    if _ext.use_native(sc):
        loss, acc = _PairwiseFn.apply(sc, sr)
    else:
        loss = -F.logsigmoid(sc - sr).mean()
        acc = (sc > sr).float().mean().detach()
    return (loss, acc) if return_accuracy else loss


# ------------------------------------------------------------------- REINFORCE + KL penalty
class _KLPGFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, lr, reward, kl_coef):
        loss, klm, dlp, adv = _ext.require().kl_penalty_pg(lp, lr, reward, kl_coef)
        ctx.save_for_backward(dlp)
        ctx.mark_non_differentiable(klm, adv)
        return loss, klm, adv

    @staticmethod
    def backward(ctx, gloss, _gk, _ga):
        (dlp,) = ctx.saved_tensors
        return dlp * gloss, None, None, None


def kl_penalty_pg(policy_logp: torch.Tensor, ref_logp: torch.Tensor, reward: torch.Tensor,
                  kl_coef: float = 0.1):
    """kl = lp - lr; r' = r - c*kl; A = r' - mean(r'); loss = -mean(stopgrad(A) * lp).

    Returns (loss, kl_mean, advantages)."""
    lp = policy_logp.float().contiguous()
    lr = ref_logp.float().detach().contiguous()
    r = reward.float().detach().contiguous()
    if _ext.use_native(lp):
        return _KLPGFn.apply(lp, lr, r, float(kl_coef))
    kl = lp.detach() - lr
    shaped = r - kl_coef * kl
    adv = shaped - shaped.mean()
    loss = -(adv * lp).mean()
    return loss, kl.mean(), adv


# ----------------------------------------------------------------- ensemble-KL distillation
class _EnsembleKLFn(torch.autograd.Function):
    """KL(p_bar || q) per row from student logits [N, V] and K teacher logits [K, N, V]."""

    @staticmethod
    def forward(ctx, s_logits, t_logits):
        ops = _ext.require()
        s_lse = ops.row_lse(s_logits)
        K, N, V = t_logits.shape
        t_lse = ops.row_lse(t_logits.view(K * N, V)).view(K, N)
        kl = ops.ensemble_kl(s_logits, t_logits, s_lse, t_lse, None, False)  # read-only here
        ctx.save_for_backward(s_logits, t_logits, s_lse, t_lse)
        return kl

    @staticmethod
    def backward(ctx, g):
        ops = _ext.require()
        s_logits, t_logits, s_lse, t_lse = ctx.saved_tensors
        ds = s_logits.clone()
        ops.ensemble_kl(ds, t_logits, s_lse, t_lse, g.float().contiguous(), True)
        return ds, None


def ensemble_kl(student_logits: torch.Tensor, teacher_logits: torch.Tensor) -> torch.Tensor:
    """student [N, V], teachers [K, N, V] (same vocab) -> per-row KL(mean_k p_k || q) [N]."""
    if _ext.use_native(student_logits):
        return _EnsembleKLFn.apply(student_logits.contiguous(), teacher_logits.contiguous().detach())
    logq = F.log_softmax(student_logits.float(), dim=-1)
    pbar = torch.softmax(teacher_logits.float(), dim=-1).mean(0)
    return F.kl_div(logq, pbar, reduction="none").sum(-1)


# ------------------------------------------------- generalised JSD(beta) distillation (GKD)
def _inv_temp(temperature: float) -> float:
    """float(1 / temperature): the divide in double, rounded once to fp32 (as the `*_temp` ops)."""
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"temperature must be finite and > 0, got {temperature!r}")
    return torch.tensor(1.0 / t, dtype=torch.float64).float().item()


def _check_beta(beta: float) -> float:
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1], got {beta!r}")
    return beta


class _GJSDFn(torch.autograd.Function):
    """Per-row JSD(beta) on the HIP kernels: one launch forward, one backward; the gradient goes
    into a buffer of its own (the saved logits are only read)."""

    @staticmethod
    def forward(ctx, s_logits, t_logits, row_mask, beta, inv_temp):
        loss, aux, s_lse, t_lse = _ext.require().gjsd_fwd(s_logits, t_logits, row_mask, beta, inv_temp)
        ctx.save_for_backward(s_logits, t_logits, s_lse, t_lse, aux, row_mask)
        ctx.beta, ctx.inv_temp = beta, inv_temp
        return loss

    @staticmethod
    def backward(ctx, g):
        s_logits, t_logits, s_lse, t_lse, aux, row_mask = ctx.saved_tensors
        ds = _ext.require().gjsd_bwd(s_logits, t_logits, s_lse, t_lse, aux, row_mask, g.float().contiguous(),
                                     ctx.beta, ctx.inv_temp)
        return ds, None, None, None, None


def _gjsd_cpu(s: torch.Tensor, t: torch.Tensor, beta: float, inv_temp: float,
              row_mask: Optional[torch.Tensor]) -> torch.Tensor:
    i = torch.tensor(inv_temp, dtype=torch.float32)
    lq = F.log_softmax(s.float() * i, dim=-1)
    lpk = F.log_softmax(t.detach().float() * i, dim=-1)
    K = lpk.shape[0]
    lp = lpk[0] if K == 1 else torch.logsumexp(lpk, 0) - math.log(K)
    q_dead, p_dead = lq == -math.inf, lp == -math.inf
    zero = torch.zeros_like(lp)
    inf = torch.full_like(lp, math.inf)
    # a -inf entry is replaced BEFORE it meets a product: its term is an exact 0 and autograd never
    # sees 0 * inf there
    lqs, lps = torch.where(q_dead, zero, lq), torch.where(p_dead, zero, lp)

    def p_sum(lm, m_dead):  # sum_v p (log p - log m); +inf where m = 0 < p
        term = torch.where(m_dead, inf, lps.exp() * (lps - torch.where(m_dead, zero, lm)))
        return torch.where(p_dead, zero, term).sum(-1)

    def q_sum(lm, m_dead):
        term = torch.where(m_dead, inf, lqs.exp() * (lqs - torch.where(m_dead, zero, lm)))
        return torch.where(q_dead, zero, term).sum(-1)

    if beta == 0.0:
        loss = p_sum(lq, q_dead)
    elif beta == 1.0:
        loss = q_sum(lp, p_dead)
    else:
        both = q_dead & p_dead  # m = 0 only there, and there neither sum has a term
        lm = torch.logaddexp(torch.where(both, zero, lp + math.log(beta)),
                             torch.where(both, zero, lq + math.log1p(-beta)))
        never = torch.zeros_like(both)
        loss = beta * p_sum(lm, never) + (1.0 - beta) * q_sum(lm, never)
    if row_mask is not None:
        loss = torch.where(row_mask != 0, loss, torch.zeros_like(loss))
    return loss


def generalized_jsd(student_logits: torch.Tensor, teacher_logits: torch.Tensor, beta: float = 0.5,
                    temperature: float = 1.0, row_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row generalised Jensen-Shannon divergence JSD(beta) of GKD (Agarwal et al.):
    student [N, V], teachers [K, N, V] (same vocabulary, K <= 8 on the GPU) -> [N] fp32.

    With i = float(1 / temperature) (divided in double, rounded once to fp32), q = softmax(i s) and
    p = (1/K) sum_k softmax(i t_k):

        beta = 0      L = sum_v p (log p - log q)                  forward KL (at i = 1: `ensemble_kl`)
        beta = 1      L = A,  A = sum_v q (log q - log p)          reverse KL
        0 < beta < 1  m = beta p + (1 - beta) q
                      L = beta sum_v p (log p - log m) + (1 - beta) A,   A = sum_v q (log q - log m)

        dL/ds_v = i (q_v - p_v)                        beta = 0
        dL/ds_v = i c q_v (log q_v - log m_v - A)      beta > 0; c = 1 - beta (beta = 1: c = 1, m = p)

    The gradient flows through the student only; teachers are constants. Everything is formed in
    the log domain (log p = logsumexp_k log p_k - log K, log m = logaddexp), so rows whose student
    and teachers disagree by hundreds of nats stay finite.
    Conventions: an entry with q_v = 0 (student logit -inf) adds exactly 0 to A and receives gradient
    exactly 0; an entry with p_v = 0 adds exactly 0 to the p sums. The mathematically infinite cases,
    beta = 0 with q_v = 0 < p_v and beta = 1 with p_v = 0 < q_v, return +inf (as `ensemble_kl` does),
    and the gradient of such a row is unspecified.
    `row_mask` [N] (fp32 or uint8 on the GPU; any dtype on the CPU): a row with mask 0 has loss and
    gradient exactly 0 and its logits are never read into a sum (NaN there does not surface on the
    GPU; the CPU formula masks the value, and its autograd must not be fed NaN logits).
    GPU: `gjsd_fwd` / `gjsd_bwd` (csrc/gjsd.hip), one launch each, no host sync; the logits may be
    row-strided views. CPU: the formula above on log_softmax(x.float() * i)."""
    beta = _check_beta(beta)
    it = _inv_temp(temperature)
    if _ext.use_native(student_logits):
        mask = None
        if row_mask is not None:
            mask = row_mask if row_mask.dtype == torch.uint8 else row_mask.float()
            mask = mask.detach().contiguous()
        if student_logits.stride(-1) != 1:
            student_logits = student_logits.contiguous()
        teacher_logits = teacher_logits.detach()
        if teacher_logits.stride(-1) != 1:
            teacher_logits = teacher_logits.contiguous()
        return _GJSDFn.apply(student_logits, teacher_logits, mask, beta, it)
    return _gjsd_cpu(student_logits, teacher_logits, beta, it, row_mask)


# ------------------------------------------------------------- PPO (actor-critic) objectives
# Token-level PPO for the north-star "PPO RLHF (actor + critic + reward)" configuration; the
# reference's sequence-level REINFORCE (train_rlhf.py:149-153, `kl_penalty_pg` above) stays the
# default algorithm. [S, T] fp32 grids; `mask` selects action tokens.
def gae(rewards: torch.Tensor, values: torch.Tensor, mask: torch.Tensor, gamma: float = 1.0,
        lam: float = 0.95):
    """Generalised advantage estimation (no gradient):
    A_t = m_t (delta_t + gamma lam m_{t+1} A_{t+1}), delta_t = r_t + gamma m_{t+1} V_{t+1} - V_t.
    Returns (advantages, returns = A + V)."""
    r = rewards.detach().float().contiguous()
    v = values.detach().float().contiguous()
    m = mask.detach().float().contiguous()
    if _ext.use_native(r):
        return _ext.require().gae(r, v, m, float(gamma), float(lam))
    S, T = r.shape
    adv = torch.zeros_like(r)
    nxt = torch.zeros(S, dtype=r.dtype, device=r.device)
    zero = torch.zeros_like(nxt)
    for t in range(T - 1, -1, -1):
        mn = m[:, t + 1] if t + 1 < T else zero
        vn = v[:, t + 1] if t + 1 < T else zero
        delta = r[:, t] + gamma * mn * vn - v[:, t]
        nxt = m[:, t] * (delta + gamma * lam * mn * nxt)
        adv[:, t] = nxt
    return adv, adv + v


class _PPOPolicyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, old, adv, mask, eps):
        loss, dlp, metrics = _ext.require().ppo_policy_loss(lp, old, adv, mask, eps)
        ctx.save_for_backward(dlp)
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, gloss, _gm):
        (dlp,) = ctx.saved_tensors
        return dlp * gloss, None, None, None, None


class _PPOPolicyWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, old, adv, mask, w, eps):
        loss, dlp, metrics = _ext.require().ppo_policy_loss_w(lp, old, adv, mask, w, eps)
        ctx.save_for_backward(dlp)
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, gloss, _gm):
        (dlp,) = ctx.saved_tensors
        return dlp * gloss, None, None, None, None, None


def ppo_policy_loss(logp: torch.Tensor, old_logp: torch.Tensor, advantages: torch.Tensor,
                    mask: torch.Tensor, clip_eps: float = 0.2, *, is_weight: Optional[torch.Tensor] = None):
    """Clipped surrogate, mean over masked tokens of max(-A rho, -A clip(rho, 1 +- eps)),
    rho = exp(logp - old_logp). Returns (loss, {clipfrac, approx_kl}) (device tensors).
    `is_weight` (a detached grid like `logp`, e.g. from `rollout_is_weights`) multiplies every
    token's surrogate; the divisor stays the masked-token count and the metrics stay unweighted."""
    lp = logp.float().contiguous()
    old = old_logp.detach().float().contiguous()
    a = advantages.detach().float().contiguous()
    m = mask.detach().float().contiguous()
    w = None
    if is_weight is not None:
        w = is_weight.detach().float().contiguous()
        if w.shape != lp.shape:
            raise ValueError(f"ppo_policy_loss: is_weight {tuple(w.shape)} must have logp's shape {tuple(lp.shape)}")
    if _ext.use_native(lp):
        if w is None:
            loss, met = _PPOPolicyFn.apply(lp, old, a, m, float(clip_eps))
        else:
            loss, met = _PPOPolicyWFn.apply(lp, old, a, m, w, float(clip_eps))
        return loss, {"clipfrac": met[0], "approx_kl": met[1]}
    n = m.sum().clamp(min=1)
    rho = torch.exp(lp - old)
    per = torch.maximum(-a * rho, -a * rho.clamp(1 - clip_eps, 1 + clip_eps))
    if w is not None:
        per = w * per
    loss = (per * m).sum() / n
    with torch.no_grad():
        clipfrac = (((rho - 1).abs() > clip_eps).float() * m).sum() / n
        akl = (((rho - 1) - (lp - old)) * m).sum() / n
    return loss, {"clipfrac": clipfrac, "approx_kl": akl}


class _PPOValueFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, old, ret, mask, clip):
        loss, dval = _ext.require().ppo_value_loss(val, old, ret, mask, clip)
        ctx.save_for_backward(dval)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dval,) = ctx.saved_tensors
        return dval * g, None, None, None, None


def ppo_value_loss(values: torch.Tensor, old_values: torch.Tensor, returns: torch.Tensor,
                   mask: torch.Tensor, clip: float = 0.2) -> torch.Tensor:
    """0.5 * masked mean of max((V - R)^2, (V_clip - R)^2), V_clip = V_old + clamp(V - V_old, +-c)."""
    v = values.float().contiguous()
    old = old_values.detach().float().contiguous()
    R = returns.detach().float().contiguous()
    m = mask.detach().float().contiguous()
    if _ext.use_native(v):
        return _PPOValueFn.apply(v, old, R, m, float(clip))
    n = m.sum().clamp(min=1)
    vc = old + (v - old).clamp(-clip, clip)
    return 0.5 * (torch.maximum((v - R) ** 2, (vc - R) ** 2) * m).sum() / n


# ------------------------------------------------------- GRPO (critic-free, group-relative)
# Every prompt is sampled G times (rows p*G .. p*G+G-1 of the rollout batch); a rollout's advantage
# is its reward standardised inside its group, and the update is a token-level clipped surrogate
# plus a k3 KL term to the frozen reference. `loss_type` picks the normalisation: "sequence"
# (GRPO), "token" (DAPO), "constant" (Dr. GRPO).
GRPO_LOSS_TYPES = ("sequence", "token", "constant")
# the importance ratio of the clipped surrogate: per token (GRPO), or one length-normalised ratio
# per rollout (GSPO, Group Sequence Policy Optimization)
GRPO_IMPORTANCE_LEVELS = ("token", "sequence")


def _ref_group_advantages(scores: torch.Tensor, G: int, scale_std: bool = True, eps: float = 1e-4):
    """The torch formula of `group_advantages` (any device): (adv [P*G], in-group std [P])."""
    r = scores.detach().float().reshape(-1, G)
    mu = r.mean(1, keepdim=True)
    sd = ((r - mu) ** 2).mean(1, keepdim=True).sqrt()
    const = r.max(1, keepdim=True).values == r.min(1, keepdim=True).values
    sd = torch.where(const, torch.zeros_like(sd), sd)
    adv = (r - mu) / (sd + eps) if scale_std else r - mu
    adv = torch.where(const, torch.zeros_like(adv), adv)  # a constant group is exactly 0
    return adv.reshape(-1), sd.reshape(-1)


def group_advantages(scores: torch.Tensor, G: int, scale_std: bool = True, eps: float = 1e-4
                     ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """Group-relative advantages (no gradient): per group of G consecutive scores mu = mean,
    sd = population std; adv = (r - mu) / (sd + eps), or r - mu with `scale_std=False`
    (Dr. GRPO). A constant-reward group gives exactly 0. Returns (adv [P*G], metrics) with device
    tensors `frac_zero_std` (groups with sd == 0) and `reward_std` (mean in-group sd)."""
    G = int(G)
    if G < 1 or scores.numel() % G:
        raise ValueError(f"group_advantages: {scores.numel()} scores do not split into groups of {G}")
    r = scores.detach().float().contiguous().view(-1)
    if _ext.use_native(r):
        adv, sd = _ext.require().group_advantages(r, G, bool(scale_std), float(eps))
    else:
        adv, sd = _ref_group_advantages(r, G, scale_std, eps)
    return adv, {"frac_zero_std": (sd == 0).float().mean(), "reward_std": sd.mean()}


def _ref_grpo_loss(logp, old_logp, ref_logp, adv, mask, clip_low: float = 0.2,
                   clip_high: Optional[float] = None, beta: float = 0.04, loss_type: str = "sequence",
                   max_len: Optional[int] = None, denom: Optional[torch.Tensor] = None,
                   is_weight: Optional[torch.Tensor] = None, importance_level: str = "token"):
    """The torch formula of `grpo_loss` (any device, differentiable in `logp` through autograd)."""
    if importance_level not in GRPO_IMPORTANCE_LEVELS:
        raise ValueError(f"grpo_loss: importance_level must be one of {'|'.join(GRPO_IMPORTANCE_LEVELS)}, "
                         f"got {importance_level!r}")
    clip_high = clip_low if clip_high is None else clip_high
    lp = logp.float()
    m = mask.detach().float()
    a = adv.detach().float().view(-1, 1)
    old = lp.detach() if old_logp is None else old_logp.detach().float()
    if importance_level == "sequence":
        return _ref_gspo_loss(lp, old, ref_logp, a, m, clip_low, clip_high, beta, loss_type, max_len, denom,
                              is_weight)
    d = lp - old
    rho = torch.exp(d)
    per = torch.maximum(-a * rho, -a * rho.clamp(1 - clip_low, 1 + clip_high))
    if is_weight is not None:
        per = is_weight.detach().float() * per
    kl = torch.zeros_like(per)
    if ref_logp is not None:
        dr = ref_logp.detach().float() - lp
        kl = torch.exp(dr) - dr - 1
        per = per + beta * kl
    S = lp.shape[0]
    c = m.sum(1)
    if loss_type == "sequence":
        num, div = ((per * m).sum(1) / c.clamp(min=1)).sum(), float(S)
    elif loss_type == "token":
        num, div = (per * m).sum(), m.sum().clamp(min=1)
    else:
        num, div = (per * m).sum(), float(S) * float(max_len if max_len is not None else 0)
    if denom is not None:
        div = denom.detach().float().reshape(())
    loss = num / div
    with torch.no_grad():
        n = m.sum()
        inv = 1.0 / n.clamp(min=1)
        out = ((rho < 1 - clip_low) | (rho > 1 + clip_high)).float()
        metrics = {"clipfrac": (out * m).sum() * inv, "approx_kl": (((rho - 1) - d) * m).sum() * inv,
                   "kl_ref": (kl * m).sum() * inv, "tokens": n}
    return loss, metrics


def _ref_gspo_loss(lp, old, ref_logp, a, m, clip_low, clip_high, beta, loss_type, max_len, denom, is_weight):
    """`_ref_grpo_loss` at `importance_level="sequence"` (its prepared operands: fp32 `lp`, detached
    `old` and `m`, `a` [S, 1]). Entries outside the mask are selected away before any sum, so NaN
    or junk there reaches neither an output nor the gradient. Precondition: exp(l_s) finite (with
    A = 0 an infinite ratio would give NaN here; the kernel returns the clamped branch)."""
    on = m != 0
    zero = torch.zeros_like(lp)
    c = m.sum(1, keepdim=True)
    ls = torch.where(on, lp - old, zero).sum(1, keepdim=True) / c.clamp(min=1)
    sr = torch.exp(ls)
    pg = torch.maximum(-a * sr, -a * sr.clamp(1 - clip_low, 1 + clip_high))  # [S, 1]: the row's surrogate
    per = pg.expand_as(lp)
    if is_weight is not None:
        per = torch.where(on, is_weight.detach().float(), zero) * per
    kl = zero
    if ref_logp is not None:
        dr = torch.where(on, ref_logp.detach().float() - lp, zero)
        kl = torch.exp(dr) - dr - 1
        per = per + beta * kl
    per = torch.where(on, per, zero)
    S = lp.shape[0]
    if loss_type == "sequence":
        num, div = ((per * m).sum(1) / c.view(-1).clamp(min=1)).sum(), float(S)
    elif loss_type == "token":
        num, div = (per * m).sum(), m.sum().clamp(min=1)
    else:
        num, div = (per * m).sum(), float(S) * float(max_len if max_len is not None else 0)
    if denom is not None:
        div = denom.detach().float().reshape(())
    loss = num / div
    with torch.no_grad():
        n = m.sum()
        inv = 1.0 / n.clamp(min=1)
        out = ((sr < 1 - clip_low) | (sr > 1 + clip_high)).float()
        metrics = {"clipfrac": (out * c).sum() * inv, "approx_kl": (((sr - 1) - ls) * c).sum() * inv,
                   "kl_ref": (kl * m).sum() * inv, "tokens": n}
    return loss, metrics


class _GRPOFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, old, ref, adv, mask, denom, clip_low, clip_high, beta, mode, max_len):
        loss, dlp, metrics = _ext.require().grpo_loss(lp, old, ref, adv, mask, denom, clip_low, clip_high,
                                                      beta, mode, max_len)
        ctx.save_for_backward(dlp)
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, gloss, _gm):
        (dlp,) = ctx.saved_tensors
        return (dlp * gloss,) + (None,) * 10


class _GRPOWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, old, ref, adv, mask, w, denom, clip_low, clip_high, beta, mode, max_len):
        loss, dlp, metrics = _ext.require().grpo_loss_w(lp, old, ref, adv, mask, w, denom, clip_low,
                                                        clip_high, beta, mode, max_len)
        ctx.save_for_backward(dlp)
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, gloss, _gm):
        (dlp,) = ctx.saved_tensors
        return (dlp * gloss,) + (None,) * 11


class _GRPOSeqFn(torch.autograd.Function):
    """`grpo_loss_seq`: the sequence-level ratio (GSPO); `w` may be None."""

    @staticmethod
    def forward(ctx, lp, old, ref, adv, mask, w, denom, clip_low, clip_high, beta, mode, max_len):
        loss, dlp, metrics = _ext.require().grpo_loss_seq(lp, old, ref, adv, mask, w, denom, clip_low,
                                                          clip_high, beta, mode, max_len)
        ctx.save_for_backward(dlp)
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, gloss, _gm):
        (dlp,) = ctx.saved_tensors
        return (dlp * gloss,) + (None,) * 11


def grpo_loss(logp: torch.Tensor, old_logp: Optional[torch.Tensor], ref_logp: Optional[torch.Tensor],
              adv: torch.Tensor, mask: torch.Tensor, clip_low: float = 0.2,
              clip_high: Optional[float] = None, beta: float = 0.04, loss_type: str = "sequence",
              max_len: Optional[int] = None, denom: Optional[torch.Tensor] = None, *,
              is_weight: Optional[torch.Tensor] = None, importance_level: str = "token"
              ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """GRPO objective on [S, T] fp32 grids (`mask`: action tokens), `adv` [S] one value per rollout.

        d = logp - old; rho = exp(d); pg = max(-A rho, -A clamp(rho, 1 - clip_low, 1 + clip_high))
        dr = ref - logp; kl = exp(dr) - dr - 1 (k3); per = pg + beta kl
        sequence: sum_s [sum_t m per / max(c_s, 1)] / S     token: sum m per / max(sum m, 1)
        constant: sum m per / (S max_len)

    `old_logp=None`: on-policy (old = logp.detach()); `ref_logp=None` only with beta == 0;
    `clip_high=None`: clip_low. `denom` (fp32 device tensor [1]) replaces the final divisor, so the
    micro-batches of one rollout batch share the whole batch's normaliser without a host sync
    (sequence mode: the full batch's S). `is_weight` ([S, T], detached, e.g. from
    `rollout_is_weights`) multiplies pg only: per = w pg + beta kl; the divisors stay the
    action-token counts and the metrics stay unweighted. Returns (loss, metrics) with device
    tensors `clipfrac`, `approx_kl`, `kl_ref` (token means over the mask) and `tokens`.

    `importance_level="sequence"` (GSPO): one length-normalised ratio per rollout replaces rho, and
    every action token of the row carries the row's surrogate; kl, the normalisations, `denom` and
    the unweighted divisors keep their meaning:

        l_s = sum_{t: m != 0} d / max(c_s, 1); sr_s = exp(l_s)        (c_s = 0: l_s = 0, sr_s = 1)
        pg_s = max(-A sr_s, -A clamp(sr_s, 1 - clip_low, 1 + clip_high)); per = w pg_s + beta kl
        dloss/dlogp_u = m_u scale_s [g_s (l1 >= l2 ? l1 : 0) - beta (exp(dr_u) - 1)],
        g_s = sum_t m w / max(c_s, 1) (1 without `is_weight`), scale_s the token-level scale
        clipfrac = sum_s c_s [sr_s outside the clip range] / n; approx_kl = sum_s c_s ((sr_s - 1) - l_s) / n

    Entries outside the mask are never read into a sum there: NaN or junk in them reaches no
    output. A fully masked row contributes 0 and takes a zero gradient row."""
    if importance_level not in GRPO_IMPORTANCE_LEVELS:
        raise ValueError(f"grpo_loss: importance_level must be one of {'|'.join(GRPO_IMPORTANCE_LEVELS)}, "
                         f"got {importance_level!r}")
    if loss_type not in GRPO_LOSS_TYPES:
        raise ValueError(f"grpo_loss: loss_type must be one of {'|'.join(GRPO_LOSS_TYPES)}, got {loss_type!r}")
    if loss_type == "constant" and max_len is None and denom is None:
        raise ValueError("grpo_loss: loss_type='constant' needs max_len")
    if ref_logp is None and beta != 0:
        raise ValueError("grpo_loss: ref_logp=None is allowed only with beta == 0")
    clip_high = clip_low if clip_high is None else clip_high
    lp = logp.float().contiguous()
    w = None
    if is_weight is not None:
        w = is_weight.detach().float().contiguous()
        if w.shape != lp.shape:
            raise ValueError(f"grpo_loss: is_weight {tuple(w.shape)} must have logp's shape {tuple(lp.shape)}")
    if not _ext.use_native(lp):
        return _ref_grpo_loss(lp, old_logp, ref_logp, adv, mask, clip_low, clip_high,
                              beta, loss_type, max_len, denom, w, importance_level)
    # absent operands alias logp: d = 0 (rho = 1) on-policy, dr = 0 (kl = 0) without a reference
    old = lp.detach() if old_logp is None else old_logp.detach().float().contiguous()
    ref = lp.detach() if ref_logp is None else ref_logp.detach().float().contiguous()
    a = adv.detach().float().contiguous().view(-1)
    m = mask.detach().float().contiguous()
    dn = denom.detach().float().reshape(1) if denom is not None else None
    tail = (dn, float(clip_low), float(clip_high), float(beta), GRPO_LOSS_TYPES.index(loss_type),
            float(max_len or 0))
    if importance_level == "sequence":
        loss, met = _GRPOSeqFn.apply(lp, old, ref, a, m, w, *tail)
    elif w is None:
        loss, met = _GRPOFn.apply(lp, old, ref, a, m, *tail)
    else:
        loss, met = _GRPOWFn.apply(lp, old, ref, a, m, w, *tail)
    return loss, {"clipfrac": met[0], "approx_kl": met[1], "kl_ref": met[2], "tokens": met[3]}


# ------------------------------------------- truncated importance weights (rollout / trainer)
# The rollout engine (bf16 / fp8 decode kernels, possibly one step stale) is not the policy the
# trainer differentiates. Truncated importance sampling keeps the trainer's own old-policy
# log-probs for the PPO ratio and multiplies every action token's surrogate by a detached, capped
# w = min(pi_trainer_old(a) / pi_rollout(a), C); the masked variant drops tokens outside [F, C].
ROLLOUT_IS_LEVELS = ("token", "sequence")
ROLLOUT_IS_MODES = ("truncate", "mask")


def _rollout_is_args(cap, floor, level, mode):
    if level not in ROLLOUT_IS_LEVELS:
        raise ValueError(f"rollout_is_weights: level must be {'|'.join(ROLLOUT_IS_LEVELS)}, got {level!r}")
    if mode not in ROLLOUT_IS_MODES:
        raise ValueError(f"rollout_is_weights: mode must be {'|'.join(ROLLOUT_IS_MODES)}, got {mode!r}")
    cap = float(cap)
    if not (math.isfinite(cap) and cap > 0):
        raise ValueError(f"rollout_is_weights: cap must be finite and > 0, got {cap!r}")
    floor = 1.0 / cap if floor is None else float(floor)
    if not 0 <= floor <= cap:
        raise ValueError(f"rollout_is_weights: floor must lie in [0, cap = {cap}], got {floor!r}")
    return cap, floor


def _ref_rollout_is_weights(trainer_lp, rollout_lp, mask, cap: float = 2.0, floor: Optional[float] = None,
                            level: str = "token", mode: str = "truncate"):
    """The torch formula of `rollout_is_weights` (any device): (w [S, T], metrics [5])."""
    cap, floor = _rollout_is_args(cap, floor, level, mode)
    m = mask.detach().float()
    on = m != 0
    d = torch.where(on, trainer_lp.detach().float() - rollout_lp.detach().float(), torch.zeros_like(m))
    if level == "sequence":
        d = (d.sum(1, keepdim=True) / m.sum(1, keepdim=True).clamp(min=1)).expand_as(m)
    r = torch.exp(d)
    high = (r > cap) & on
    low = (r < floor) & on if mode == "mask" else torch.zeros_like(on)
    w = r.clamp(max=cap) if mode == "truncate" else torch.where(high | low, torch.zeros_like(r), r)
    w = torch.where(on, w, torch.zeros_like(w))
    n = m.sum()
    n1 = n.clamp(min=1)
    sw, sw2 = w.sum(), (w * w).sum()
    # a fraction: <= 1 by Cauchy-Schwarz, clamped against the last rounding
    ess = torch.where(sw2 > 0, (sw * sw / (n1 * sw2.clamp(min=torch.finfo(torch.float32).tiny))).clamp(max=1),
                      torch.zeros_like(sw))
    return w, torch.stack([sw / n1, high.float().sum() / n1, low.float().sum() / n1, ess, n])


@torch.no_grad()
def rollout_is_weights(trainer_lp: torch.Tensor, rollout_lp: torch.Tensor, mask: torch.Tensor,
                       cap: float = 2.0, floor: Optional[float] = None, level: str = "token",
                       mode: str = "truncate") -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """Truncated importance weights (no gradient) on [S, T] fp32 action grids: `trainer_lp` the
    trainer's own old-policy log-probs, `rollout_lp` the rollout engine's, `mask` the action tokens.

        d = trainer_lp - rollout_lp;  token: l = d;  sequence: l_s = sum_t m d / max(sum_t m, 1)
        r = exp(l);  truncate: w = min(r, cap);  mask: w = r if floor <= r <= cap else 0;  w = 0 off the mask

    The sequence level is the length-normalised (geometric-mean) ratio, not the product.
    `floor=None`: 1 / cap (mask mode only). Returns (w, metrics) with device tensors over the n
    action tokens: `is_mean`, `is_frac_high` (r > cap), `is_frac_low` (r < floor, mask mode; else 0),
    `is_ess` = (sum w)^2 / (n sum w^2) (at most 1; 0 when every w is 0) and `tokens` = n. One fused HIP op (two launches, no
    atomics, no host sync) on the GPU."""
    cap, floor = _rollout_is_args(cap, floor, level, mode)
    t = trainer_lp.detach().float().contiguous()
    r = rollout_lp.detach().float().contiguous()
    m = mask.detach().float().contiguous()
    if t.dim() != 2 or r.shape != t.shape or m.shape != t.shape:
        raise ValueError(f"rollout_is_weights: three [S, T] grids of one shape, got {tuple(t.shape)}, "
                         f"{tuple(r.shape)}, {tuple(m.shape)}")
    if _ext.use_native(t):
        w, met = _ext.require().rollout_is_weights(t, r, m, cap, floor, ROLLOUT_IS_LEVELS.index(level),
                                                   ROLLOUT_IS_MODES.index(mode))
    else:
        w, met = _ref_rollout_is_weights(t, r, m, cap, floor, level, mode)
    return w, {"is_mean": met[0], "is_frac_high": met[1], "is_frac_low": met[2], "is_ess": met[3],
               "tokens": met[4]}
