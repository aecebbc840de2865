"""Fused LM-head log-probabilities (SURVEY K9 + K10 + K11 + K16).

`linear_logprob(hidden, weight, targets)` = log_softmax(hidden @ W^T)[targets] per row without
ever materialising fp32 [N, V] tensors:
  * forward: one hipBLASLt GEMM -> bf16 logits; the HIP row kernel streams each logits row once
    (online max/sum) and emits logp + lse (fp32, per row).
  * backward: the HIP kernel rewrites the SAVED bf16 logits in place into dlogits
    (g * (onehot - softmax)), which feed the two grad GEMMs directly (dH = dL W, dW = dL^T H);
    with a main_grad on the LM head the same kernel also writes dL^T, the TN weight-gradient
    operand, so no separate transpose pass re-reads the [N, V] gradient.
    With grads off (frozen reference / reward scoring) logits are produced chunk by chunk and
    dropped, so the no-grad footprint is one chunk.
Semantics mirror the reference `compute_logprobs` (src/training/train_dpo.py:31-39): logits in
the model dtype (bf16), log-softmax in fp32, targets < 0 ignored (logp 0, no gradient).

`linear_logprob_entropy(hidden, weight, targets)` also returns the entropy of each row's softmax,
from the same vocabulary pass (a third online accumulator in the row kernel) and with its
gradient written by the same in-place dlogits pass: the policy entropy of PPO / GRPO without an
fp32 [N, V] softmax.

Both take `temperature` (default 1.0): the log-prob and entropy of softmax(logits / temperature),
the distribution a sampler at that temperature draws from. The row kernels apply
inv_temp = float(1 / temperature) in fp32 to the bf16 logits the GEMM wrote (the `*_temp` ops);
at 1.0 the plain ops run, kernel for kernel.

`linear_logprob(..., keep=, keep_rows=)` takes every row's log-prob over a KEPT subset of the
vocabulary, the set a top-k / top-p sampler drew the row's token from ("keep sampling mask"): `keep`
is uint8 [M, V / 8], bit j (LSB first) of byte i = vocabulary entry 8 i + j (`pack_keep`), and
`keep_rows` int64 [N] names the mask row of every logits row (< 0: the full vocabulary). The row
kernels read the mask byte next to each 16-byte logits vector (the `*_keep` ops), so no -inf is
ever written into the [N, V] logits; entries outside the set get exactly zero gradient.

`sequence_logprob(...)` adds the masked per-sequence reduction (length-normalised mean by default,
exactly the reference's `/ mask.sum(1).clamp(min=1)`, or sum) as a HIP kernel pair.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _ext
from .linear import input_grad

# no-grad (frozen reference) logits are produced and dropped per chunk of rows: 8192 rows x the
# Llama-3 vocabulary is a 2.1 GB bf16 transient, one GEMM per DPO micro-batch (two 4096-row
# chunks ran 2 x 2.93 ms vs 5.5 ms for the one 8192-row GEMM in the step, profiles/r6_*)
_NO_GRAD_CHUNK = 8192
# dlogits^T from the logprob backward kernel (A/B switch, read once)
LOGPROB_T = os.environ.get("DLA_LOGPROB_T", "1") != "0"


def inv_temperature(temperature: float) -> float:
    """The fp32 scalar the tempered kernels multiply by: 1 / temperature, the divide in double and
    rounded once to fp32 (returned widened, as the ops take it)."""
    t = float(temperature)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    return torch.tensor(1.0 / t, dtype=torch.float64).float().item()


def _ref_linear_logprob(hidden, weight, targets, temperature: float = 1.0):
    logits = F.linear(hidden, weight).float()
    if temperature != 1.0:
        logits = logits * inv_temperature(temperature)
    lse = torch.logsumexp(logits, dim=-1)
    safe = targets.clamp(min=0)
    lp = logits.gather(-1, safe.unsqueeze(-1)).squeeze(-1) - lse
    return torch.where(targets >= 0, lp, torch.zeros_like(lp))


def pack_keep(mask: torch.Tensor) -> torch.Tensor:
    """bool [..., V] (V % 8 == 0) -> uint8 [..., V / 8]: bit j (LSB first) of byte i = entry 8 i + j."""
    V = mask.shape[-1]
    if V % 8 != 0:
        raise ValueError(f"pack_keep: the vocabulary size must be a multiple of 8, got {V}")
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=mask.device)
    return (mask.reshape(*mask.shape[:-1], V // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_keep(keep: torch.Tensor) -> torch.Tensor:
    """uint8 [..., V / 8] -> bool [..., V], the inverse of `pack_keep`."""
    sh = torch.arange(8, dtype=torch.int32, device=keep.device)
    bits = (keep.to(torch.int32).unsqueeze(-1) >> sh) & 1
    return bits.bool().reshape(*keep.shape[:-1], keep.shape[-1] * 8)


def _check_keep(keep, keep_rows, N: int, V: int):
    if keep is None or keep_rows is None:
        raise ValueError("keep and keep_rows go together")
    if V % 8 != 0:
        raise ValueError(f"a keep mask needs a vocabulary size that is a multiple of 8, got {V}")
    if keep.dtype != torch.uint8 or keep.dim() != 2 or keep.shape[1] * 8 != V:
        raise ValueError(f"keep must be uint8 [M, V / 8] = [M, {V // 8}], got {keep.dtype} {tuple(keep.shape)}")
    if keep_rows.dtype != torch.int64 or tuple(keep_rows.shape) != (N,):
        raise ValueError(f"keep_rows must be int64 [{N}], got {keep_rows.dtype} {tuple(keep_rows.shape)}")


def keep_rows_bool(keep: torch.Tensor, keep_rows: torch.Tensor) -> torch.Tensor:
    """bool [N, V]: the kept set of every row (all True where keep_rows < 0), in torch."""
    m = unpack_keep(keep)[keep_rows.clamp(min=0)]
    return m | (keep_rows < 0).unsqueeze(-1)


def _ref_linear_logprob_keep(hidden, weight, targets, temperature, keep, keep_rows):
    """The formula of record: log_softmax of the fp32 logits times `inv_temperature`, with the entries
    outside the row's kept set at -inf."""
    logits = F.linear(hidden, weight).float() * inv_temperature(temperature)
    logits = logits.masked_fill(~keep_rows_bool(keep, keep_rows), float("-inf"))
    # (log_softmax spelled as `_ref_linear_logprob` spells it, so an all-ones mask gives its bits)
    lse = torch.logsumexp(logits, dim=-1)
    lp = logits.gather(-1, targets.clamp(min=0).unsqueeze(-1)).squeeze(-1) - lse
    return torch.where(targets >= 0, lp, torch.zeros_like(lp))


class _LinearLogprobFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, targets, inv_temp=None, keep=None, keep_rows=None):
        # inv_temp: None = the plain ops; a float = the tempered twins (see `inv_temperature`)
        # keep / keep_rows (with a float inv_temp): the kept-set twins of the tempered ops
        ops = _ext.require()
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        N = hidden.shape[0]
        ctx.inv_temp = inv_temp
        ctx.keep, ctx.keep_rows = keep, keep_rows

        def fwd(lg, tg, kr=None):
            if keep is not None:
                return ops.logprob_fwd_keep(lg, tg, keep, kr, inv_temp)
            return ops.logprob_fwd(lg, tg) if inv_temp is None else ops.logprob_fwd_temp(lg, tg, inv_temp)

        if need_grad:
            logits = F.linear(hidden, weight)
            logp, lse = fwd(logits, targets, keep_rows)
            ctx.save_for_backward(hidden, targets, lse, logits)
            ctx.weight = weight  # (on ctx: see ops.linear._LinearMainGradFn)
            return logp
        logp = torch.empty(N, dtype=torch.float32, device=hidden.device)
        for s in range(0, N, _NO_GRAD_CHUNK):
            e = min(N, s + _NO_GRAD_CHUNK)
            lg = F.linear(hidden[s:e], weight)
            lp, _ = fwd(lg, targets[s:e], keep_rows[s:e] if keep is not None else None)
            logp[s:e] = lp
        return logp

    @staticmethod
    def backward(ctx, g):
        ops = _ext.require()
        hidden, targets, lse, logits = ctx.saved_tensors
        weight = ctx.weight
        it = ctx.inv_temp
        keep, kr = ctx.keep, ctx.keep_rows
        from .linear import _tn_ok, accumulate_weight_grad

        g = g.float().contiguous()
        dlt = None
        mg = getattr(weight, "main_grad", None)
        if (LOGPROB_T and ctx.needs_input_grad[1] and mg is not None and not getattr(weight, "_dla_shared", False)
                and _tn_ok(mg, logits.shape[0])):
            # the LM head's weight gradient runs as a TN GEMM on dlogits^T: write it from the
            # same pass that turns the logits into dlogits (undefined when the shape is outside
            # the kernel -> in-place kernel + transpose inside accumulate_weight_grad)
            if keep is not None:
                dlt = ops.logprob_bwd_t_keep(logits, targets, lse, g, keep, kr, it)
            else:
                dlt = (ops.logprob_bwd_t(logits, targets, lse, g) if it is None
                       else ops.logprob_bwd_t_temp(logits, targets, lse, g, it))
            if not dlt.numel():
                dlt = None
        if dlt is None:
            if keep is not None:
                ops.logprob_bwd_keep(logits, targets, lse, g, keep, kr, it)
            elif it is None:
                ops.logprob_bwd(logits, targets, lse, g)
            else:
                ops.logprob_bwd_temp(logits, targets, lse, g, it)
        dlogits = logits  # rewritten in place
        dh = input_grad(dlogits, weight) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            if not accumulate_weight_grad(weight, dlogits, hidden, dyt=dlt):
                dw = dlogits.t() @ hidden
        return dh, dw, None, None, None, None


def linear_logprob(hidden: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor,
                   temperature: float = 1.0, keep: Optional[torch.Tensor] = None,
                   keep_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hidden [N, H], weight [V, H], targets [N] (int64, <0 = ignore) -> logp [N] fp32, of
    softmax(hidden @ W^T / temperature). With `keep` (uint8 [M, V / 8], `pack_keep`) and `keep_rows`
    (int64 [N], < 0 = no mask; every other value must be < M) the softmax of row r runs over the
    entries kept in row keep_rows[r] only: logp is -inf for a target outside the set, and the
    entries outside it get exactly zero gradient."""
    if keep is not None or keep_rows is not None:
        _check_keep(keep, keep_rows, hidden.shape[0], weight.shape[0])
        if _ext.use_native(hidden):
            return _LinearLogprobFn.apply(hidden.contiguous(), weight, targets.contiguous(),
                                          inv_temperature(temperature), keep.contiguous(), keep_rows.contiguous())
        return _ref_linear_logprob_keep(hidden, weight, targets, temperature, keep, keep_rows)
    if _ext.use_native(hidden):
        if temperature == 1.0:
            return _LinearLogprobFn.apply(hidden.contiguous(), weight, targets.contiguous(), None, None, None)
        return _LinearLogprobFn.apply(hidden.contiguous(), weight, targets.contiguous(),
                                      inv_temperature(temperature), None, None)
    return _ref_linear_logprob(hidden, weight, targets, temperature)


def _ref_logits_logprob_entropy(logits, targets, temperature: float = 1.0):
    """The formula of record on fp32 logits: logp as `_ref_linear_logprob`, ent = -sum_v p_v (z_v - lse)
    (fp32), both 0 on ignored rows; a -inf logit has p = 0 and adds exactly 0. With a temperature z is
    the fp32 logits times `inv_temperature(temperature)`."""
    if temperature != 1.0:
        logits = logits * inv_temperature(temperature)
    lse = torch.logsumexp(logits, dim=-1)
    safe = targets.clamp(min=0)
    lp = logits.gather(-1, safe.unsqueeze(-1)).squeeze(-1) - lse
    lsm = logits - lse.unsqueeze(-1)
    ent = -(torch.exp(lsm) * lsm.masked_fill(logits == float("-inf"), 0.0)).sum(-1)
    zero = torch.zeros_like(lp)
    return torch.where(targets >= 0, lp, zero), torch.where(targets >= 0, ent, zero)


def _ref_linear_logprob_entropy(hidden, weight, targets, temperature: float = 1.0):
    return _ref_logits_logprob_entropy(F.linear(hidden, weight).float(), targets, temperature)


class _LinearLogprobEntropyFn(torch.autograd.Function):
    """`_LinearLogprobFn` with the row entropy as a second output of the same vocabulary pass; its
    gradient goes into the same in-place dlogits pass. With no gradient arriving for the entropy
    (logging only) the backward runs the plain log-prob kernels."""

    @staticmethod
    def forward(ctx, hidden, weight, targets, inv_temp=None):
        ops = _ext.require()
        ctx.set_materialize_grads(False)
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        N = hidden.shape[0]
        ctx.inv_temp = inv_temp

        def fwd(lg, tg):
            return (ops.logprob_entropy_fwd(lg, tg) if inv_temp is None
                    else ops.logprob_entropy_fwd_temp(lg, tg, inv_temp))

        if need_grad:
            logits = F.linear(hidden, weight)
            logp, lse, ent = fwd(logits, targets)
            ent = ent.masked_fill_(targets < 0, 0.0)
            ctx.save_for_backward(hidden, targets, lse, ent, logits)
            ctx.weight = weight  # (on ctx: see ops.linear._LinearMainGradFn)
            return logp, ent
        logp = torch.empty(N, dtype=torch.float32, device=hidden.device)
        ent = torch.empty(N, dtype=torch.float32, device=hidden.device)
        for s in range(0, N, _NO_GRAD_CHUNK):
            e = min(N, s + _NO_GRAD_CHUNK)
            lg = F.linear(hidden[s:e], weight)
            lp, _, en = fwd(lg, targets[s:e])
            logp[s:e] = lp
            ent[s:e] = en
        return logp, ent.masked_fill_(targets < 0, 0.0)

    @staticmethod
    def backward(ctx, g, ge):
        ops = _ext.require()
        hidden, targets, lse, ent, logits = ctx.saved_tensors
        weight = ctx.weight
        it = ctx.inv_temp
        if g is None and ge is None:
            return None, None, None, None
        from .linear import _tn_ok, accumulate_weight_grad

        g = torch.zeros_like(lse) if g is None else g.float().contiguous()
        ge = None if ge is None else ge.float().contiguous()
        dlt = None
        mg = getattr(weight, "main_grad", None)
        if (LOGPROB_T and ctx.needs_input_grad[1] and mg is not None and not getattr(weight, "_dla_shared", False)
                and _tn_ok(mg, logits.shape[0])):
            # as in _LinearLogprobFn: dlogits^T from the same pass (empty outside the kernel's shapes)
            if it is None:
                dlt = (ops.logprob_bwd_t(logits, targets, lse, g) if ge is None
                       else ops.logprob_entropy_bwd_t(logits, targets, lse, ent, g, ge))
            else:
                dlt = (ops.logprob_bwd_t_temp(logits, targets, lse, g, it) if ge is None
                       else ops.logprob_entropy_bwd_t_temp(logits, targets, lse, ent, g, ge, it))
            if not dlt.numel():
                dlt = None
        if dlt is None:
            if it is None:
                if ge is None:
                    ops.logprob_bwd(logits, targets, lse, g)
                else:
                    ops.logprob_entropy_bwd(logits, targets, lse, ent, g, ge)
            elif ge is None:
                ops.logprob_bwd_temp(logits, targets, lse, g, it)
            else:
                ops.logprob_entropy_bwd_temp(logits, targets, lse, ent, g, ge, it)
        dlogits = logits  # rewritten in place
        dh = input_grad(dlogits, weight) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            if not accumulate_weight_grad(weight, dlogits, hidden, dyt=dlt):
                dw = dlogits.t() @ hidden
        return dh, dw, None, None


def linear_logprob_entropy(hidden: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor,
                           temperature: float = 1.0):
    """hidden [N, H], weight [V, H], targets [N] (int64, <0 = ignore) -> (logp, ent), fp32 [N]:
    `linear_logprob` plus the entropy of softmax(hidden @ W^T / temperature) per row (0 where
    ignored), differentiable through both."""
    if _ext.use_native(hidden):
        if temperature == 1.0:
            return _LinearLogprobEntropyFn.apply(hidden.contiguous(), weight, targets.contiguous(), None)
        return _LinearLogprobEntropyFn.apply(hidden.contiguous(), weight, targets.contiguous(),
                                             inv_temperature(temperature))
    return _ref_linear_logprob_entropy(hidden, weight, targets, temperature)


class _SeqReduceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, mask, mean):
        ops = _ext.require()
        s, cnt = ops.seq_reduce(lp, mask)
        ctx.save_for_backward(mask, cnt)
        ctx.mean = mean
        return s / cnt.clamp(min=1.0) if mean else s

    @staticmethod
    def backward(ctx, g):
        mask, cnt = ctx.saved_tensors
        return _ext.require().seq_expand_grad(g.float().contiguous(), mask, cnt, ctx.mean), None, None


def seq_reduce(token_lp: torch.Tensor, mask: torch.Tensor, mean: bool = True) -> torch.Tensor:
    """token_lp [S, T] fp32, mask [S, T] -> masked mean (or sum) over T."""
    mask = mask.float().contiguous()
    if _ext.use_native(token_lp):
        return _SeqReduceFn.apply(token_lp.contiguous(), mask, mean)
    s = (token_lp * mask).sum(dim=1)
    return s / mask.sum(dim=1).clamp(min=1) if mean else s


def shifted_targets(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                    ignore_index: int = -100):
    """targets[t] = input_ids[t+1]; last position ignored. mask[t] = am[t] * am[t+1].

    For right padding this equals the reference's `attention_mask[:, 1:]`; for left padding it
    also drops the pad -> first-token "prediction" the reference would score (its query row
    sees no valid keys)."""
    S, T = input_ids.shape
    tgt = torch.full_like(input_ids, ignore_index)
    tgt[:, :-1] = input_ids[:, 1:]
    mask = torch.zeros((S, T), dtype=torch.float32, device=input_ids.device)
    if attention_mask is None:
        mask[:, :-1] = 1.0
    else:
        am = attention_mask.float()
        mask[:, :-1] = am[:, 1:] * am[:, :-1]
    tgt = torch.where(mask > 0, tgt, torch.full_like(tgt, ignore_index))
    return tgt, mask


def sequence_logprob(hidden: torch.Tensor, weight: torch.Tensor, input_ids: torch.Tensor,
                     attention_mask: Optional[torch.Tensor] = None,
                     reduction: str = "mean") -> torch.Tensor:
    """Per-sequence log p(x_{t+1} | x_<=t) reduced over valid positions.

    hidden [S, T, H] final hidden states (after the final norm), weight [V, H] LM head.
    reduction 'mean' reproduces the reference's length-normalised `compute_logprobs`.
    """
    S, T, H = hidden.shape
    tgt, mask = shifted_targets(input_ids, attention_mask)
    lp = linear_logprob(hidden.reshape(S * T, H), weight, tgt.reshape(-1)).view(S, T)
    return seq_reduce(lp, mask, mean=(reduction == "mean"))


def token_nll(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """HF ForCausalLMLoss: mean over labels != -100 of -log p(labels[t+1] | x_<=t)."""
    S, T, H = hidden.shape
    tgt = torch.full_like(labels, -100)
    tgt[:, :-1] = labels[:, 1:]
    tgt = tgt.reshape(-1)
    lp = linear_logprob(hidden.reshape(S * T, H), weight, tgt)
    n = (tgt >= 0).sum().clamp(min=1)
    return -(lp.sum() / n)
