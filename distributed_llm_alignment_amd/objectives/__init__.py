"""Training objectives (SURVEY layer L5), each a pure function of (models, batch) so trainers,
benchmarks and tests share one implementation.

  dpo_step_loss    reference train_dpo.py:106-121 (length-normalised seq log-probs, DPO loss)
  sft_loss         reference train_sft.py:145-146 (HF causal-LM CE, ignore -100)
  reward_loss      reference train_reward.py:139-148 (Bradley-Terry pairwise)
  rlhf_loss        reference train_rlhf.py:127-153 (REINFORCE with KL-shaped reward)
  ppo_rollout_stats / ppo_loss  token-level actor-critic PPO (GAE, clipped surrogate + value
                   loss) for `ppo.algorithm: ppo` (north-star config; not in the reference)
  rollout_is_stats truncated importance weights (rollout engine vs trainer) for the two below
  grpo_rollout_stats / grpo_loss  critic-free group-relative policy optimisation (group
                   advantages, token-level clipped surrogate + k3 KL to the reference) for
                   `ppo.algorithm: grpo` (not in the reference)
  distill_loss     reference train_distill.py:125-147 (CE on rollouts or ensemble forward KL)
  gkd_loss         on-policy distillation (GKD): JSD(beta) at a temperature over response positions,
                   on dataset rows or on sequences the student sampled (not in the reference)
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .. import ops


def concat_pair(batch: Dict[str, Dict[str, torch.Tensor]], pad_id: int = 0):
    """Stack chosen and rejected into one [2B, T] batch (one forward instead of two; the math is
    per-sequence so this is identical to the reference's separate forwards)."""
    c, r = batch["chosen"], batch["rejected"]
    T = max(c["input_ids"].shape[1], r["input_ids"].shape[1])

    def pad(x, v):
        return F.pad(x, (0, T - x.shape[1]), value=v)

    ids = torch.cat([pad(c["input_ids"], pad_id), pad(r["input_ids"], pad_id)])
    mask = torch.cat([pad(c["attention_mask"], 0), pad(r["attention_mask"], 0)])
    loss_mask = None
    if "loss_mask" in c:
        loss_mask = torch.cat([pad(c["loss_mask"], 0), pad(r["loss_mask"], 0)])
    return ids, mask, loss_mask


def sequence_logps(model, ids, mask, reduction: str = "mean", loss_mask=None):
    """Per-sequence log-prob; `loss_mask` (optional) restricts scoring to response tokens."""
    if loss_mask is None:
        return model.sequence_logprob(ids, mask, reduction)
    from ..models.transformer import sp_seq_reduce

    h = model(ids, mask)
    tgt, m = model._sp_targets(*ops.shifted_targets(ids, loss_mask))
    lp = model._masked_token_logprob(h, tgt)
    return sp_seq_reduce(model.sp, lp, m, reduction == "mean")


def dpo_step_loss(policy, ref, batch, beta: float = 0.1, label_smoothing: float = 0.0,
                  reduction: str = "mean", ref_logps: Optional[torch.Tensor] = None, pad_id: int = 0):
    ids, mask, lm = concat_pair(batch, pad_id)
    B = ids.shape[0] // 2
    pol = sequence_logps(policy, ids, mask, reduction, lm)
    if ref_logps is None:
        with torch.no_grad():
            ref_logps = sequence_logps(ref, ids, mask, reduction, lm)
    loss, metrics = ops.dpo_loss(pol[:B], pol[B:], ref_logps[:B], ref_logps[B:], beta, label_smoothing)
    metrics["policy_chosen_logps"] = pol[:B].detach()
    metrics["policy_rejected_logps"] = pol[B:].detach()
    return loss, metrics


def ref_sequence_logps(ref, batch, reduction: str = "mean", pad_id: int = 0):
    """The frozen reference's per-sequence log-probs for a preference batch ([2B]: chosen, rejected)."""
    ids, mask, lm = concat_pair(batch, pad_id)
    with torch.no_grad():
        return sequence_logps(ref, ids, mask, reduction, lm)


class RefLogpsStream:
    """Runs the frozen reference forward on a second HIP stream so it overlaps the policy's
    forward/backward on the main stream (the two are independent until the DPO loss). The ref
    pass is GEMM-light relative to its memory-bound phases (attention, norms, SwiGLU) and the
    policy's are the same: interleaving the two streams fills the gaps each leaves on the CUs.
    `submit(batch)` returns a handle; `result(handle)` makes the main stream wait for it.
    On CPU (or with enabled=False) it simply computes inline."""

    def __init__(self, ref, reduction: str = "mean", pad_id: int = 0, enabled: bool = True):
        self.ref, self.reduction, self.pad_id = ref, reduction, pad_id
        dev = next(ref.parameters()).device
        self.stream = torch.cuda.Stream(device=dev) if (enabled and dev.type == "cuda") else None

    def submit(self, batch):
        if self.stream is None:
            return ref_sequence_logps(self.ref, batch, self.reduction, self.pad_id), None
        main = torch.cuda.current_stream(self.stream.device)
        self.stream.wait_stream(main)  # batch tensors were produced on the main stream
        with torch.cuda.stream(self.stream):
            lp = ref_sequence_logps(self.ref, batch, self.reduction, self.pad_id)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return lp, ev

    def result(self, handle):
        lp, ev = handle
        if ev is not None:
            main = torch.cuda.current_stream(lp.device)
            main.wait_event(ev)
            lp.record_stream(main)
        return lp


def sft_loss(model, batch) -> torch.Tensor:
    return model.causal_lm_loss(batch["input_ids"], batch["labels"], batch.get("attention_mask"),
                                batch.get("segment_ids"))


def reward_loss(rm, batch, pad_id: int = 0):
    ids, mask, _ = concat_pair(batch, pad_id)
    B = ids.shape[0] // 2
    scores = rm(ids, mask)
    loss, acc = ops.pairwise_loss(scores[:B], scores[B:], return_accuracy=True)
    return loss, {"accuracy": acc, "chosen_scores": scores[:B].detach(), "rejected_scores": scores[B:].detach()}


def rlhf_loss(policy, ref, seqs, mask, rewards, kl_coef: float = 0.1):
    pol = policy.sequence_logprob(seqs, mask, "mean")
    with torch.no_grad():
        ref_lp = ref.sequence_logprob(seqs, mask, "mean")
    loss, kl_mean, adv = ops.kl_penalty_pg(pol, ref_lp, rewards, kl_coef)
    return loss, {"kl": kl_mean, "advantages": adv, "policy_logps": pol.detach()}


def action_mask(mask: torch.Tensor, prompt_len: int) -> torch.Tensor:
    """[S, T] fp32: 1 at grid positions t whose action (token t + 1) is a generated, valid token
    (prompt tokens and padding after EOS are not actions)."""
    S, T = mask.shape
    act = torch.zeros((S, T), dtype=torch.float32, device=mask.device)
    gen = (torch.arange(1, T, device=mask.device) >= prompt_len).float()
    act[:, :-1] = mask[:, 1:].float() * gen
    return act


def rollout_logp_grid(logp: torch.Tensor, prompt_len: int, T: int) -> torch.Tensor:
    """The rollout engine's log-probs (`generate(return_logprobs=True)`, [S, n]: column j belongs
    to the token at sequence position prompt_len + j) placed into the [S, T] action grid of
    `token_logprobs` / `action_mask`, where position t holds the log-prob of token t + 1: column
    j goes to prompt_len + j - 1, everything else is 0."""
    S, n = logp.shape
    if prompt_len < 1 or prompt_len + n > T:
        raise ValueError(f"rollout_logp_grid: prompt_len {prompt_len} + {n} generated columns do not fit T = {T}")
    grid = torch.zeros((S, T), dtype=torch.float32, device=logp.device)
    grid[:, prompt_len - 1:prompt_len - 1 + n] = logp.float()
    return grid


def keep_row_grid(act: torch.Tensor, prompt_len: int, n: int) -> torch.Tensor:
    """int64 [S, T]: the row of a flattened `generate(return_keep_mask=True)` mask ([S * n, V / 8])
    that every action position reads, s * n + (t - (prompt_len - 1)) where act[s, t] == 1
    (`rollout_logp_grid`'s alignment: grid position t scores token t + 1, generated column
    t + 1 - prompt_len), and -1 everywhere else (prompt positions, padding, after EOS): a
    non-action position never reads a mask row. The `keep_rows` of `token_logprobs`."""
    S, T = act.shape
    if prompt_len < 1 or prompt_len + n > T:
        raise ValueError(f"keep_row_grid: prompt_len {prompt_len} + {n} generated columns do not fit T = {T}")
    col = torch.arange(T, device=act.device) - (prompt_len - 1)
    idx = torch.arange(S, device=act.device).unsqueeze(1) * n + col.unsqueeze(0)
    ok = (act > 0) & (col >= 0).unsqueeze(0) & (col < n).unsqueeze(0)
    return torch.where(ok, idx, torch.full_like(idx, -1))


def keep_fraction(full_lp: torch.Tensor, kept_lp: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
    """`train/keep_fraction`: the mean over action tokens of exp(logp_full - logp_kept), the share of
    the (tempered) full-vocabulary mass the kept sets hold, from two [S, T] action grids of log-probs of
    the same tokens at the same temperature (a device tensor: no host sync)."""
    f = torch.exp((full_lp.float() - kept_lp.float()) * act) * act
    return f.sum() / act.sum().clamp(min=1)


def _keep_kw(keep, keep_rows) -> dict:
    """`token_logprobs` keywords of the step's sampling mask: none without one, so a default run makes
    the calls (and launches the kernels) it always made."""
    if keep is None and keep_rows is None:
        return {}
    if keep is None or keep_rows is None:
        raise ValueError("keep and keep_rows go together")
    return {"keep": keep.reshape(-1, keep.shape[-1]), "keep_rows": keep_rows}


def rollout_mismatch(rollout_lp: torch.Tensor, trainer_lp: torch.Tensor, act: torch.Tensor):
    """How far the engine that sampled the rollouts is from the trainer's own forward, on the
    sampled tokens (both [S, T] action grids): `rollout_kl`, the mean over action tokens of
    logp_rollout - logp_trainer (the k1 estimate of KL(rollout engine || trainer)), and
    `rollout_logp_absdiff_max`. Device tensors: no host sync."""
    d = (rollout_lp.float() - trainer_lp.float()) * act
    return {"rollout_kl": d.sum() / act.sum().clamp(min=1), "rollout_logp_absdiff_max": d.abs().max()}


def rollout_is_stats(rollout_logp: torch.Tensor, trainer_lp: torch.Tensor, act: torch.Tensor,
                     cap: float = 2.0, floor: Optional[float] = None, level: str = "token",
                     mode: str = "truncate"):
    """The `is_weight` / `rollout_is` entries of the PPO / GRPO stats: the truncated importance
    weights of one rollout batch (`ops.rollout_is_weights` of the trainer's own old-policy
    log-probs against the rollout engine's, both [S, T] action grids) and their metrics
    `rollout_is_mean`, `rollout_is_frac_high`, `rollout_is_frac_low`, `rollout_is_ess` (device
    tensors: no host sync)."""
    w, met = ops.rollout_is_weights(trainer_lp, rollout_logp, act, cap, floor, level, mode)
    return {"is_weight": w, "rollout_is": {f"rollout_{k}": v for k, v in met.items() if k != "tokens"}}


def _share_kw(shared_prefix) -> dict:
    """`token_logprobs` keyword of prefix sharing (`shared_prefix=(G, prompt_len)`: every group's
    prompt computed once, `models.transformer.shared_prefix_pack`): none when off, so a default run
    makes the calls (and launches the kernels) it always made."""
    if shared_prefix is None:
        return {}
    G, prompt_len = shared_prefix
    return {"shared_prefix": (int(G), int(prompt_len))}


def _temp_kw(temperature: float) -> dict:
    """`token_logprobs` keywords for the step's log-prob temperature: none at 1.0, so a default
    run makes the calls (and launches the kernels) it always made."""
    return {} if temperature == 1.0 else {"temperature": float(temperature)}


@torch.no_grad()
def ppo_rollout_stats(policy, ref, critic, seqs, mask, prompt_len: int, scores, kl_coef: float = 0.1,
                      gamma: float = 1.0, lam: float = 0.95, whiten: bool = True,
                      old_logp: Optional[torch.Tensor] = None, rollout_logp: Optional[torch.Tensor] = None,
                      is_cap: float = 2.0, is_floor: Optional[float] = None, is_level: str = "token",
                      is_mode: str = "truncate", temperature: float = 1.0,
                      keep: Optional[torch.Tensor] = None, keep_rows: Optional[torch.Tensor] = None):
    """Token-level PPO targets for one batch of rollouts (actor-critic; the north-star
    "PPO RLHF (actor + critic + reward)" config). Per-token reward = -kl_coef * (logp - logp_ref)
    on every action, plus the reward-model score on the last action; GAE(gamma, lam) over the
    critic's values; advantages whitened over the action tokens. `old_logp` ([S, T] action grid,
    e.g. `rollout_logp_grid` of the rollout engine's log-probs): used as the old-policy log-probs,
    in the KL reward too, instead of a policy forward over the rollouts. `rollout_logp` (the same
    kind of grid) instead leaves the old-policy log-probs and the KL reward the trainer's own and
    adds `is_weight` / `rollout_is` (`rollout_is_stats` with the four `is_*` settings): truncated
    importance weights for `ppo_loss`, computed once per rollout batch. `temperature`: every
    log-prob here (policy, reference) is of softmax(logits / temperature); grids passed in must be
    at the same temperature. `keep` / `keep_rows` (`generate(return_keep_mask=True)`,
    `keep_row_grid`): every log-prob here is over the kept set of its token; grids passed in must be
    the engine's kept-set log-probs. `keep_rows` is returned in the stats (sliced by rows with the
    rest; `keep` stays whole, the indices are global)."""
    tkw = {**_temp_kw(temperature), **_keep_kw(keep, keep_rows)}
    old_lp = old_logp.float() if old_logp is not None else policy.token_logprobs(seqs, mask, **tkw)
    ref_lp = ref.token_logprobs(seqs, mask, **tkw)
    values = critic(seqs, mask)
    act = action_mask(mask, prompt_len)
    kl = (old_lp - ref_lp) * act
    rewards = -kl_coef * kl
    S, T = act.shape
    last = (act * torch.arange(T, device=act.device, dtype=act.dtype)).argmax(1)
    has = act.sum(1) > 0
    rewards[torch.arange(S, device=act.device), last] += torch.where(has, scores.float(), torch.zeros_like(scores.float()))
    adv, ret = ops.gae(rewards, values, act, gamma, lam)
    if whiten:
        n = act.sum().clamp(min=1)
        mu = (adv * act).sum() / n
        var = (((adv - mu) ** 2) * act).sum() / n
        adv = (adv - mu) * torch.rsqrt(var + 1e-8) * act
    out = {"old_logp": old_lp, "values": values, "advantages": adv, "returns": ret, "act": act,
           "kl": kl.sum(1) / act.sum(1).clamp(min=1), "scores": scores.float()}
    if keep_rows is not None:
        out["keep_rows"] = keep_rows
    if rollout_logp is not None:
        out.update(rollout_is_stats(rollout_logp, old_lp, act, is_cap, is_floor, is_level, is_mode))
    return out


# The actor and the critic of a PPO minibatch are independent until the summed loss: the critic's
# forward (and, through autograd's per-node streams, its backward) runs on a side stream so the two
# models' kernels share the chip. At the PPO shapes (4 rollouts x 768 tokens per minibatch) the
# o / down projections are [3072, 4096] outputs = 192 256x256 tiles for 256 CUs, so one model alone
# leaves a quarter of the CUs idle in every such GEMM. DLA_PPO_CRITIC_STREAM=0: one stream.
PPO_CRITIC_STREAM = os.environ.get("DLA_PPO_CRITIC_STREAM", "1") != "0"
_CRITIC_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def ppo_critic_stream(device: torch.device):
    """The side stream the critic runs on (None off the GPU or when disabled)."""
    if not (PPO_CRITIC_STREAM and device.type == "cuda"):
        return None
    i = device.index if device.index is not None else torch.cuda.current_device()
    if i not in _CRITIC_STREAMS:
        _CRITIC_STREAMS[i] = torch.cuda.Stream(device=i)
    return _CRITIC_STREAMS[i]


def token_logprobs_entropy(policy, seqs, mask, act, entropy_coef: float = 0.0, log_entropy: bool = False,
                           n_act: Optional[torch.Tensor] = None, temperature: float = 1.0,
                           keep: Optional[torch.Tensor] = None, keep_rows: Optional[torch.Tensor] = None,
                           shared_prefix=None):
    """Token log-probs of a PPO / GRPO (micro-)batch and, when `entropy_coef != 0` or
    `log_entropy`, the policy entropy from the same LM-head pass: returns (lp, bonus, entropy).
    `bonus` = entropy_coef * sum(ent * act) / n_act (None when the coefficient is 0: the entropy is
    then detached and the plain backward kernels run); `n_act`, a device tensor (no host sync), is
    the action-token count the bonus is normalised by -- the whole minibatch's for micro-batches,
    this batch's own by default. `entropy` is this batch's detached mean over action tokens (None
    when off). `temperature`: log-probs and entropy of softmax(logits / temperature). `keep` /
    `keep_rows`: the log-probs over the kept sets; the entropy under a kept set does not exist yet, so
    an entropy bonus or `log_entropy` together with them raises ValueError. `shared_prefix`
    (`(G, prompt_len)`, whole groups of G rows): the forward shares each group's prompt."""
    tkw = {**_temp_kw(temperature), **_keep_kw(keep, keep_rows), **_share_kw(shared_prefix)}
    if keep is not None and (entropy_coef != 0 or log_entropy):
        raise ValueError("entropy_coef / log_entropy are not supported together with a keep mask")
    if entropy_coef == 0 and not log_entropy:
        return policy.token_logprobs(seqs, mask, **tkw), None, None
    lp, ent = policy.token_logprobs(seqs, mask, with_entropy=True, **tkw)
    if entropy_coef == 0:
        ent = ent.detach()
    tot = (ent * act).sum()
    own = act.sum().clamp(min=1)
    bonus = None
    if entropy_coef != 0:
        bonus = entropy_coef * tot / (own if n_act is None else n_act.reshape(()))
    return lp, bonus, tot.detach() / own


def ppo_loss(policy, critic, seqs, mask, stats: Dict[str, torch.Tensor], clip_eps: float = 0.2,
             value_clip: float = 0.2, vf_coef: float = 0.1, entropy_coef: float = 0.0,
             log_entropy: bool = False, temperature: float = 1.0,
             keep: Optional[torch.Tensor] = None, keep_rows: Optional[torch.Tensor] = None):
    """Clipped surrogate (HIP fused fwd+bwd) + vf_coef * clipped value loss on one minibatch,
    minus entropy_coef * the mean policy entropy over action tokens (`metrics["entropy"]`, also
    with `log_entropy` alone). `stats["is_weight"]` (optional) weights the surrogate per token.
    `temperature`: the policy's log-probs and entropy at that temperature (as in `stats`).
    `keep` (+ `keep_rows`, default `stats["keep_rows"]`): the policy's log-probs over the kept sets.
    Run its backward through `ppo_backward` (joins the critic's stream
    afterwards)."""
    cs = ppo_critic_stream(seqs.device)
    main = torch.cuda.current_stream(seqs.device) if cs is not None else None
    if cs is not None:
        cs.wait_stream(main)  # the critic's weights (last optimizer step) and this minibatch
        with torch.cuda.stream(cs):
            v = critic(seqs, mask)
            vl = ops.ppo_value_loss(v, stats["values"], stats["returns"], stats["act"], value_clip)
    if keep is not None and keep_rows is None:
        keep_rows = stats.get("keep_rows")
    lp, bonus, entropy = token_logprobs_entropy(policy, seqs, mask, stats["act"], entropy_coef, log_entropy,
                                                temperature=temperature, keep=keep, keep_rows=keep_rows)
    pl, pm = ops.ppo_policy_loss(lp, stats["old_logp"], stats["advantages"], stats["act"], clip_eps,
                                 is_weight=stats.get("is_weight"))
    if cs is None:
        v = critic(seqs, mask)
        vl = ops.ppo_value_loss(v, stats["values"], stats["returns"], stats["act"], value_clip)
    else:
        main.wait_stream(cs)
        vl.record_stream(main)
    loss, m = pl + vf_coef * vl, {"policy_loss": pl.detach(), "value_loss": vl.detach(), **pm}
    if bonus is not None:
        loss = loss - bonus
    if entropy is not None:
        m["entropy"] = entropy
    return loss, m


def ppo_backward(loss: torch.Tensor) -> None:
    """loss.backward() for `ppo_loss`: the critic's backward nodes run on its side stream and its
    weight gradients are accumulated there (GEMM-epilogue main_grad writes that autograd does not
    order against the caller's stream), so the caller's stream waits for that stream before the
    optimizer steps read the gradient buffers."""
    loss.backward()
    cs = ppo_critic_stream(loss.device)
    if cs is not None:
        torch.cuda.current_stream(loss.device).wait_stream(cs)


@torch.no_grad()
def grpo_rollout_stats(policy, ref, seqs, mask, prompt_len: int, scores, G: int, beta: float = 0.04,
                       scale_std: bool = True, need_old: bool = False,
                       old_logp: Optional[torch.Tensor] = None, rollout_logp: Optional[torch.Tensor] = None,
                       is_cap: float = 2.0, is_floor: Optional[float] = None, is_level: str = "token",
                       is_mode: str = "truncate", temperature: float = 1.0,
                       keep: Optional[torch.Tensor] = None, keep_rows: Optional[torch.Tensor] = None,
                       shared_prefix=None):
    """GRPO targets for one batch of group rollouts (rows p*G .. p*G+G-1 sample prompt p). The
    reward is the reward-model score alone (the KL lives in the loss); a rollout's advantage is its
    score standardised inside its group. The reference's token log-probs are skipped entirely
    when beta == 0, and the old policy's are computed only with `need_old` (more than one update
    per rollout batch; a single on-policy update uses old = logp.detach()). `old_logp` ([S, T]
    action grid, e.g. `rollout_logp_grid` of the rollout engine's log-probs): returned as the
    old-policy log-probs, whatever `need_old`, with no policy forward. `rollout_logp` (the same
    kind of grid) instead keeps the old-policy log-probs the trainer's own (the forward always
    runs, as with `need_old`) and adds `is_weight` / `rollout_is` (`rollout_is_stats` with the four
    `is_*` settings): truncated importance weights for `grpo_loss`, computed once per rollout batch. `temperature`:
    every log-prob here is of softmax(logits / temperature); grids passed in must be at the same.
    `keep` / `keep_rows`: as in `ppo_rollout_stats`. `shared_prefix=(G, prompt_len)`, the same
    keyword as `grpo_loss` takes (it must repeat this call's `G` and `prompt_len`: ValueError): the
    reference and old-policy forwards run on the prefix-shared layout, each group's prompt once."""
    if shared_prefix is not None and tuple(int(x) for x in shared_prefix) != (int(G), int(prompt_len)):
        raise ValueError(f"shared_prefix {tuple(shared_prefix)} differs from (G, prompt_len) = ({G}, {prompt_len})")
    tkw = {**_temp_kw(temperature), **_keep_kw(keep, keep_rows), **_share_kw(shared_prefix)}
    act = action_mask(mask, prompt_len)
    adv, gm = ops.group_advantages(scores, G, scale_std)
    ref_lp = ref.token_logprobs(seqs, mask, **tkw) if beta != 0 else None
    if old_logp is not None:
        old_logp = old_logp.float()
    elif need_old or rollout_logp is not None:
        old_logp = policy.token_logprobs(seqs, mask, **tkw)
    out = {"act": act, "advantages": adv, "ref_logp": ref_lp, "old_logp": old_logp,
           "scores": scores.float(), "reward_std": gm["reward_std"], "frac_zero_std": gm["frac_zero_std"]}
    if keep_rows is not None:
        out["keep_rows"] = keep_rows
    if rollout_logp is not None:
        out.update(rollout_is_stats(rollout_logp, old_logp, act, is_cap, is_floor, is_level, is_mode))
    return out


def grpo_loss(policy, seqs, mask, stats: Dict[str, torch.Tensor], clip_low: float = 0.2,
              clip_high: Optional[float] = None, beta: float = 0.04, loss_type: str = "sequence",
              max_len: Optional[int] = None, denom: Optional[torch.Tensor] = None,
              entropy_coef: float = 0.0, log_entropy: bool = False, n_act: Optional[torch.Tensor] = None,
              temperature: float = 1.0, keep: Optional[torch.Tensor] = None,
              keep_rows: Optional[torch.Tensor] = None, importance_level: str = "token",
              shared_prefix=None):
    """Token-level clipped surrogate + beta * k3 KL to the reference (HIP fused fwd+bwd) on one
    (micro-)batch of rollouts; `stats` from `grpo_rollout_stats`, sliced to the same rows.
    `entropy_coef` / `log_entropy` / `n_act`: the entropy bonus and metric of
    `token_logprobs_entropy`. `stats["is_weight"]` (optional) weights the policy-gradient term per
    token. `temperature`: the policy's log-probs and entropy at that temperature (as in `stats`).
    `keep` (+ `keep_rows`, default `stats["keep_rows"]`): the policy's log-probs over the kept sets.
    `importance_level`: "token", or "sequence" for one length-normalised ratio per rollout (GSPO;
    `ops.grpo_loss`). `shared_prefix=(G, prompt_len)`: the rows are whole groups of G rollouts and
    the policy forward and backward run on the prefix-shared layout (each prompt once)."""
    if keep is not None and keep_rows is None:
        keep_rows = stats.get("keep_rows")
    lp, bonus, entropy = token_logprobs_entropy(policy, seqs, mask, stats["act"], entropy_coef, log_entropy,
                                                n_act, temperature=temperature, keep=keep, keep_rows=keep_rows,
                                                shared_prefix=shared_prefix)
    loss, m = ops.grpo_loss(lp, stats.get("old_logp"), stats.get("ref_logp"), stats["advantages"],
                            stats["act"], clip_low, clip_high, beta, loss_type, max_len, denom,
                            is_weight=stats.get("is_weight"), importance_level=importance_level)
    if bonus is not None:
        loss = loss - bonus
    if entropy is not None:
        m = {**m, "entropy": entropy}
    return loss, {"kl": m["kl_ref"], **m}


def grpo_denominator(act: torch.Tensor, loss_type: str, max_len: Optional[int] = None) -> torch.Tensor:
    """The whole rollout batch's divisor as a device tensor [1] (no host sync), shared by its
    micro-batches: S (sequence), the action-token count (token), S * max_len (constant)."""
    S = act.shape[0]
    if loss_type == "token":
        return act.sum().clamp(min=1).reshape(1)
    return torch.full((1,), float(S if loss_type == "sequence" else S * int(max_len)),
                      dtype=torch.float32, device=act.device)


# Tokens per ensemble-KL chunk: (teachers + 1) x chunk x V bf16 logits exist at a time
# (V = 51200, 2 teachers, 1024 tokens: 315 MB) instead of [K, S, T, V] for the whole batch.
KL_CHUNK_TOKENS = int(os.environ.get("DLA_KL_CHUNK_TOKENS", "1024"))


def _kl_chunk(student, teachers, hs_c, ths_c):
    s_logits = student.logits(hs_c)
    with torch.no_grad():
        t_logits = torch.stack([t.logits(h) for t, h in zip(teachers, ths_c)])
    return ops.ensemble_kl(s_logits, t_logits)


def chunked_ensemble_kl(student, teachers: Sequence, hs: torch.Tensor, ths: Sequence[torch.Tensor],
                        chunk: Optional[int] = None) -> torch.Tensor:
    """Per-token forward KL(mean_k softmax(teacher_k) || softmax(student)) from final hidden rows
    (student hs [N, H] with grad, teacher hidden [N, H] each), token-chunked: each chunk's
    student and teacher logits are produced by the LM-head GEMMs, reduced by the fused HIP
    ensemble-KL kernel and dropped; the backward recomputes the chunk (activation checkpoint), so
    neither [K, N, V] teacher logits nor [N, V] student logits are ever materialised whole
    (reference: src/training/train_distill.py:130-144 stacks all teacher logits)."""
    from torch.utils.checkpoint import checkpoint

    chunk = int(chunk or KL_CHUNK_TOKENS)
    N = hs.shape[0]
    outs = []
    for i in range(0, N, chunk):
        hs_c = hs[i:i + chunk]
        ths_c = [h[i:i + chunk] for h in ths]
        if torch.is_grad_enabled() and hs.requires_grad and N > chunk:
            outs.append(checkpoint(_kl_chunk, student, teachers, hs_c, ths_c, use_reentrant=False))
        else:
            outs.append(_kl_chunk(student, teachers, hs_c, ths_c))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def distill_loss(student, teachers: Sequence, batch, use_kl: bool):
    """CE on teacher rollouts (labels = input_ids) or token-masked ensemble forward-KL. KL mode
    compares every position (unshifted), as the reference does (train_distill.py:140-144)."""
    if not (use_kl and teachers):
        return student.causal_lm_loss(batch["input_ids"], batch["labels"], batch.get("attention_mask"))
    ids, mask = batch["input_ids"], batch["attention_mask"]
    for t in teachers:
        if t.cfg.vocab_size != student.cfg.vocab_size:
            raise ValueError("KL distillation requires teacher and student to share a vocabulary "
                             "(SURVEY Appendix A #15)")
    hs = student(ids, mask)
    with torch.no_grad():
        ths = [t(ids, mask) for t in teachers]  # teacher hidden states only: [S, T, H] each
    S, T = hs.shape[0], hs.shape[1]
    kl = chunked_ensemble_kl(student, teachers, hs.reshape(S * T, -1),
                             [h.reshape(S * T, -1) for h in ths]).view(S, T)
    sp = student.sp
    if sp is None:
        m = mask.float()
        return (kl * m).sum() / m.sum()
    m = sp.local(sp.pad(mask.float(), 0))  # sequence parallel: this rank's token slice
    return sp.reduce((kl * m).sum()) / sp.reduce(m.sum())


# ------------------------------------------------------------ on-policy distillation (GKD)
def _gkd_chunk(student, teachers, hs_c, ths_c, mask_c, beta, temperature):
    s_logits = student.logits(hs_c)
    with torch.no_grad():
        t_logits = torch.stack([t.logits(h) for t, h in zip(teachers, ths_c)])
    return ops.generalized_jsd(s_logits, t_logits, beta=beta, temperature=temperature, row_mask=mask_c)


def chunked_gkd(student, teachers: Sequence, hs: torch.Tensor, ths: Sequence[torch.Tensor], beta: float,
                temperature: float, row_mask: Optional[torch.Tensor], chunk: Optional[int] = None) -> torch.Tensor:
    """Per-row JSD(beta) (`ops.generalized_jsd`) from final hidden rows, in `chunked_ensemble_kl`'s
    structure: chunks of KL_CHUNK_TOKENS rows, each chunk's logits produced, reduced and dropped,
    recomputed in the backward (activation checkpoint); the `row_mask` [N] slice travels with its
    rows (masked rows: exactly 0, logits not read)."""
    from torch.utils.checkpoint import checkpoint

    chunk = int(chunk or KL_CHUNK_TOKENS)
    N = hs.shape[0]
    outs = []
    for i in range(0, N, chunk):
        hs_c = hs[i:i + chunk]
        ths_c = [h[i:i + chunk] for h in ths]
        m_c = None if row_mask is None else row_mask[i:i + chunk]
        if torch.is_grad_enabled() and hs.requires_grad and N > chunk:
            outs.append(checkpoint(_gkd_chunk, student, teachers, hs_c, ths_c, m_c, beta, temperature,
                                   use_reentrant=False))
        else:
            outs.append(_gkd_chunk(student, teachers, hs_c, ths_c, m_c, beta, temperature))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def gkd_position_mask(attention_mask: torch.Tensor, prompt_len) -> torch.Tensor:
    """[S, T] float: 1 at position t of row s when token t + 1 is a real response token, i.e.
    first_real + prompt_len_s - 1 <= t <= last_real - 1 (first_real / last_real: the row's first and
    last attended positions; `prompt_len`, an int or [S], counts the row's real prompt tokens). The
    same rule serves right-padded dataset rows (first_real = 0) and left-padded generated rows. A row
    with no response token, or with nothing attended, is all 0."""
    am = attention_mask != 0
    S, T = am.shape
    idx = torch.arange(T, device=am.device).expand(S, T)
    first = torch.where(am, idx, torch.full_like(idx, T)).min(1).values
    last = torch.where(am, idx, torch.full_like(idx, -1)).max(1).values
    pl = torch.as_tensor(prompt_len, device=am.device, dtype=idx.dtype)
    lo = (first + pl - 1).clamp(min=0).unsqueeze(1)
    return ((idx >= lo) & (idx <= (last - 1).unsqueeze(1))).float()


def gkd_loss(student, teachers: Sequence, input_ids: torch.Tensor, attention_mask: torch.Tensor, prompt_len,
             beta: float, temperature: float) -> torch.Tensor:
    """Generalised knowledge distillation on one micro-batch: JSD(beta) at `temperature` between the
    student's and the teachers' (mean) next-token distributions, over the positions that predict a
    response token (`gkd_position_mask`): sum(mask * L) / max(sum(mask), 1)."""
    if not teachers:
        raise ValueError("GKD needs at least one teacher")
    for m in (student, *teachers):
        if getattr(m, "vocab_parallel", None) is not None:
            raise ValueError("GKD does not support a vocab-parallel LM head (tensor parallelism)")
        if getattr(m, "sp", None) is not None:
            raise ValueError("GKD does not support sequence parallelism")
    for t in teachers:
        if t.cfg.vocab_size != student.cfg.vocab_size:
            raise ValueError("GKD requires teacher and student to share a vocabulary")
    hs = student(input_ids, attention_mask)
    with torch.no_grad():
        ths = [t(input_ids, attention_mask) for t in teachers]
    S, T = hs.shape[0], hs.shape[1]
    mask = gkd_position_mask(attention_mask, prompt_len)
    L = chunked_gkd(student, teachers, hs.reshape(S * T, -1), [h.reshape(S * T, -1) for h in ths],
                    beta, temperature, mask.reshape(-1)).view(S, T)
    return (mask * L).sum() / mask.sum().clamp(min=1)
