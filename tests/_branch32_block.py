"""The package's CPU branches of the block ops run in fp32 on the inputs of tests/_refs64_block.py:
one dict of fp32 outputs per op with the keys of the matching fp64 reference. Gradients come from
autograd through the CPU branch. Where a branch rounds to its input dtype at the end
(`_ref_norm(...).to(dtype)`, `swiglu`, `gelu_new`, `_ref_rope`) it is fed fp32 copies of the bf16
values, so it stays fp32. test_block_refs_cpu.py ties these to the fp64 references; the GPU module
takes E32 (the fp32 branch's own error against fp64) from them."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.models.reward import RewardModel
from distributed_llm_alignment_amd.ops.attention import _ref_rope

import _refs64_block as RB


def _leaf(x):
    return x.detach().float().clone().requires_grad_(True)


def norm(x, res, w, b, eps, rms):
    """ops.add_norm on the fp32 copy of the contract's stream s = bf16(x + r); rstd and mean by the
    branch's own formula (`_ref_norm` does not return them)."""
    s = RB.stream(x, res).float()
    y, _ = ops.add_norm(s, None, w.float(), None if b is None else b.float(), eps, rms)
    mu = torch.zeros(s.shape[0]) if rms else s.mean(-1)
    rstd = torch.rsqrt((s - mu[:, None]).pow(2).mean(-1) + eps)
    return {"s": s, "y": y, "rstd": rstd, "mean": mu}


def norm_bwd(dy, s, w, dres, eps, rms, has_bias):
    sl, wl = _leaf(s), _leaf(w)
    bl = torch.zeros(w.numel(), requires_grad=True) if has_bias else None
    y, _ = ops.add_norm(sl, None, wl, bl, eps, rms)
    gs = torch.autograd.grad(y, [sl, wl] + ([bl] if has_bias else []), dy.float())
    out = {"ds": gs[0] if dres is None else gs[0] + dres.float(), "dw": gs[1]}
    if has_bias:
        out["db"] = gs[2]
    return out


def swiglu(gu, dy):
    x = _leaf(gu)
    out = ops.swiglu(x)
    (g,) = torch.autograd.grad(out, x, dy.float())
    return {"out": out.detach(), "dgu": g}


def gelu_new(x, dy):
    xl = _leaf(x)
    y = ops.gelu_new(xl)
    (g,) = torch.autograd.grad(y, xl, dy.float())
    return {"y": y.detach(), "dx": g}


def rope(src, cos, sin, pos, rot, bwd=False):
    """`_ref_rope` on [1, tokens, heads, D]; the backward is autograd through it."""
    x = _leaf(src).unsqueeze(0)
    if not bwd:
        return {"out": _ref_rope(x.detach(), cos, sin, pos[None], rot)[0]}
    x = torch.zeros_like(x).requires_grad_(True)
    y = _ref_rope(x, cos, sin, pos[None], rot)
    (g,) = torch.autograd.grad(y, x, src.float().unsqueeze(0))
    return {"out": g[0]}


def embed_bwd(sid, perm, dy, base, V):
    """F.embedding with autograd on the in-range positions, added onto `base` in fp32."""
    ok = (sid >= 0) & (sid < V)
    tbl = torch.zeros(V, dy.shape[1], requires_grad=True)
    out = F.embedding(sid[ok], tbl)
    (g,) = torch.autograd.grad(out, tbl, dy.float()[perm[ok]])
    return {"grad": base.float() + g}


def reward_head(hidden, last, mask, w, bias, keep, scale, ds, pooled_round=True):
    """The reward model's PyTorch head: RewardModel.pool, the (given) dropout mask, Linear(H, 1).
    Last-token pooling is the gather of `pool` at the given index. Mean pooling: the contract's
    bf16 rounding of the pooled row is applied to the fp32 pool (`pooled_round`)."""
    h = _leaf(hidden)
    B, T, H = h.shape
    if mask is not None:
        pooled = RewardModel.pool(SimpleNamespace(pooling="mean"), h, mask)
        if pooled_round:
            pooled = pooled + (pooled.detach().to(RB.BF).float() - pooled.detach())  # straight-through
    else:
        pooled = h[torch.arange(B), last.long()]
    wl = _leaf(w).reshape(1, H)
    dropped = pooled * keep.float() * scale
    score = F.linear(dropped, wl, None if bias is None else bias.float()).squeeze(-1)
    dh, dw = torch.autograd.grad(score, (h, wl), ds)
    return {"score": score.detach(), "pooled": dropped.detach(), "dhidden": dh, "dw": dw.reshape(-1)}
