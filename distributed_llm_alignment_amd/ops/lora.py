"""LoRA adapter on a frozen projection: y = x W^T + s (x A^T) B^T, s = alpha / r.

The base product runs on the existing GEMM paths (F.linear, or `add_gemm` with the residual as
its C input); the two rank-r products run on the HIP kernels of csrc/lora.hip:

    t = lora_shrink(x, A, s)          t [M, r]  = bf16(s * x A^T)       streams x once
    lora_expand_add_(y, t, B)         y [M, N] += t B^T, in place       reads and writes y once

The formula of record (CPU branch, and every GPU case outside `lora_ok`):

    t = (s * (x.float() @ A.float().t())).to(x.dtype)
    y = (y0.float() + t.float() @ B.float().t()).to(x.dtype)

`s` is applied once, in fp32, inside the shrink; the expand runs with scale 1. With B == 0 the
output equals the base projection bit for bit. Backward: the frozen base weight gets no gradient
(no dW GEMM, no activation transposes, no main_grad traffic for it); `t` and the scaled `dts` are
treated as exact in the gradients (the bf16 rounding is the identity there).

Small-operand layouts: the expand kernel reads its small operand as [N, r] (forward: B) or as
[r, N] (backward dx += dts A: A as stored) through a template flag, the strided 2-byte loads
amortised over the token tiles a wave walks. The shrink kernel wants [r, K] rows; the backward
shrink dts = s dy B gets B^T from a `transpose_bf16` copy of the adapter (r x N elements): the
cached one of `ops.linear.transposed_weight` for engine-owned adapters (refreshed once per
optimizer step), a fresh one otherwise.

Dispatch on the GPU (bf16): the kernels run where they were measured to win against the library
GEMM of the same step (profiles/lora.md): the shrink at r <= SHRINK_KERNEL_MAX_RANK and
K <= SHRINK_KERNEL_MAX_K, the expand at r <= EXPAND_KERNEL_MAX_RANK. Elsewhere the library pair
runs, which keeps the rounding of the formula of record: `torch.mm(..., out_dtype=float32)`, the
scale in fp32, one rounding (shrink); `y.addmm_(t, B^T)`, whose epilogue adds y to the fp32
accumulator and rounds once (expand). DLA_LORA_KERNELS=0 forces the library pair everywhere,
DLA_LORA_KERNELS=1 the kernels for every eligible call (A/B switch).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _ext
from .linear import (accumulate_weight_grad, add_gemm, fp8_inference_ok, fp8_linear_frozen, input_grad,
                     transposed_weight)

_MODE = os.environ.get("DLA_LORA_KERNELS", "auto")
KERNELS = _MODE != "0"
KERNEL_RANKS = (8, 16, 32, 64)
# where the hand-written kernels are the default (measured, profiles/lora.md); "1" lifts the gates
SHRINK_KERNEL_MAX_RANK = 64 if _MODE == "1" else 32
SHRINK_KERNEL_MAX_K = (1 << 30) if _MODE == "1" else 4096
EXPAND_KERNEL_MAX_RANK = 64 if _MODE == "1" else 16


def _rows16(t: torch.Tensor) -> bool:
    """2-D bf16 GPU tensor the kernels can read with 16-byte loads."""
    return (t.dim() == 2 and t.is_cuda and t.dtype == torch.bfloat16 and t.stride(1) == 1
            and t.shape[1] % 8 == 0 and t.shape[1] >= 8 and t.stride(0) % 8 == 0
            and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0)


# which path served each dispatched call (tests assert that the kernels ran where they should)
CALLS = {"shrink_kernel": 0, "shrink_library": 0, "shrink_composition": 0,
         "expand_kernel": 0, "expand_library": 0, "expand_composition": 0}


def shrink_ok(x2: torch.Tensor, a: torch.Tensor) -> bool:
    """The shrink kernel can serve this call (eligibility; the default gates are `shrink_preferred`)."""
    return (_ext.available() and _rows16(x2) and _rows16(a) and a.shape[0] in KERNEL_RANKS
            and a.shape[1] == x2.shape[1] and x2.shape[0] > 0 and x2.shape[1] < (1 << 30))


def expand_ok(y2: torch.Tensor, t: torch.Tensor, b: torch.Tensor, transposed: bool = False) -> bool:
    if not (_ext.available() and _rows16(y2) and _rows16(t) and t.shape[1] in KERNEL_RANKS
            and t.shape[0] == y2.shape[0] and y2.shape[0] > 0 and y2.shape[1] < (1 << 22)):
        return False
    if transposed:
        return (b.dim() == 2 and b.is_cuda and b.dtype == torch.bfloat16 and b.stride(1) == 1
                and tuple(b.shape) == (t.shape[1], y2.shape[1]) and b.stride(0) >= b.shape[1])
    return _rows16(b) and tuple(b.shape) == (y2.shape[1], t.shape[1])


def lora_ok(x2: torch.Tensor, A: torch.Tensor, B: torch.Tensor) -> bool:
    """The kernels serve this adapter call: extension loaded, bf16, r in {8, 16, 32, 64},
    K % 8 == 0 and N % 8 == 0, unit inner strides, row strides multiples of 8, 16-byte-aligned
    bases. Anything else takes the torch composition."""
    return (shrink_ok(x2, A) and _rows16(B) and B.shape[1] == A.shape[0] and B.shape[0] < (1 << 22))


def shrink_preferred(x2: torch.Tensor, a: torch.Tensor) -> bool:
    """`shrink_ok` and inside the shapes where the kernel is the default."""
    return (KERNELS and shrink_ok(x2, a) and a.shape[0] <= SHRINK_KERNEL_MAX_RANK
            and a.shape[1] <= SHRINK_KERNEL_MAX_K)


def expand_preferred(y2: torch.Tensor, t: torch.Tensor, b: torch.Tensor, transposed: bool = False) -> bool:
    return KERNELS and expand_ok(y2, t, b, transposed) and t.shape[1] <= EXPAND_KERNEL_MAX_RANK


def shrink_library(x2: torch.Tensor, a: torch.Tensor, scale: float) -> torch.Tensor:
    """The formula of record on the library GEMM: bf16 operands, fp32 output, the scale in fp32,
    one rounding. `a` [r, K] (any strides)."""
    return (float(scale) * torch.mm(x2, a.t(), out_dtype=torch.float32)).to(x2.dtype)


def shrink_composition(x2: torch.Tensor, a: torch.Tensor, scale: float) -> torch.Tensor:
    return (float(scale) * (x2.float() @ a.float().t())).to(x2.dtype)


def expand_add_composition(y2: torch.Tensor, t: torch.Tensor, b: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """`b` as [N, r]; returns a new tensor."""
    d = t.float() @ b.float().t()
    if scale != 1.0:
        d = float(scale) * d
    return (y2.float() + d).to(y2.dtype)


def lora_shrink(x2: torch.Tensor, a: torch.Tensor, scale: float, transposed: bool = False,
                force_kernel: bool = False) -> torch.Tensor:
    """t [M, r] = (scale * x2 @ a^T) rounded once; `a` is [r, K], or [K, r] with `transposed`
    (the kernel then reads a transposed copy of `a`, cached when a training engine owns `a`).
    An eligible call (`shrink_ok`) runs the HIP kernel inside the default gates, or anywhere with
    `force_kernel`, and the library GEMM otherwise; an ineligible one the composition of record."""
    if x2.is_cuda:
        _ext.require()
        r, K = (a.shape[1], a.shape[0]) if transposed else (a.shape[0], a.shape[1])
        if transposed:  # the transposed copy is contiguous and aligned: `a` itself must be readable
            eligible = (_ext.available() and _rows16(x2) and _rows16(a) and r in KERNEL_RANKS
                        and K == x2.shape[1] and x2.shape[0] > 0 and K < (1 << 30))
        else:
            eligible = shrink_ok(x2, a)
        if eligible:
            if force_kernel or (KERNELS and r <= SHRINK_KERNEL_MAX_RANK and K <= SHRINK_KERNEL_MAX_K):
                CALLS["shrink_kernel"] += 1
                return torch.ops.dla.lora_shrink(x2, _transposed_small(a) if transposed else a.detach(), float(scale))
            CALLS["shrink_library"] += 1
            return shrink_library(x2, (a.t() if transposed else a).detach(), scale)
    CALLS["shrink_composition"] += 1
    return shrink_composition(x2, a.t() if transposed else a, scale)


def _transposed_small(a: torch.Tensor) -> torch.Tensor:
    """a^T for the backward shrink. The cached copy (ops.linear.transposed_weight) is keyed on the
    tensor's version and the owning engine's weight epoch; in-place kernel updates and `.data`
    writes move neither, so only engine-owned parameters (`_dla_epoch` present: the engine bumps
    it at every step and load) use the cache. Anything else is transposed afresh (r x N elements)."""
    if getattr(a, "_dla_epoch", None) is not None:
        return transposed_weight(a)
    at = torch.empty((a.shape[1], a.shape[0]), dtype=a.dtype, device=a.device)
    torch.ops.dla.transpose_bf16(a.detach(), at)
    return at


def lora_expand_add_(y2: torch.Tensor, t: torch.Tensor, b: torch.Tensor, scale: float = 1.0,
                     transposed: bool = False, force_kernel: bool = False) -> torch.Tensor:
    """y2 += scale * t @ b^T in place with one rounding; `b` is [N, r], or [r, N] with
    `transposed`. Returns y2. Dispatch as `lora_shrink`; the library path is `addmm_`, whose
    epilogue adds y2 to the fp32 accumulator and rounds once (scale 1 only)."""
    if y2.is_cuda:
        _ext.require()
        if expand_ok(y2, t, b, transposed):
            if force_kernel or expand_preferred(y2, t, b, transposed):
                CALLS["expand_kernel"] += 1
                torch.ops.dla.lora_expand_add_(y2, t, b.detach(), float(scale), bool(transposed))
                return y2
            if scale == 1.0:
                CALLS["expand_library"] += 1
                y2.addmm_(t, (b if transposed else b.t()).detach())
                return y2
    CALLS["expand_composition"] += 1
    y2.copy_(expand_add_composition(y2, t, b.t() if transposed else b, scale))
    return y2


class _LoRALinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, A, B, bias, resid, scale):
        K, N = x.shape[-1], weight.shape[0]
        x2 = x.reshape(-1, K)
        # both base paths return a fresh tensor, so the in-place expand is safe
        if fp8_inference_ok(x2, weight, bias):
            # the no-grad prefill of an fp8 rollout (ops.linear.fp8_inference_scope): the base
            # product on the fp8 inference GEMM, as `ops.linear` / `linear_add` run it without adapters
            y = fp8_linear_frozen(x2, weight)
            if resid is not None:
                y.add_(resid.reshape(-1, N))
        elif resid is not None:
            y = add_gemm(x2, weight, resid.reshape(-1, N))
        else:
            y = F.linear(x2, weight, bias)
        t = lora_shrink(x2, A, scale)
        lora_expand_add_(y, t, B)
        ctx.save_for_backward(x, t)
        # weights ride on ctx, not save_for_backward (see ops.linear._LinearMainGradFn): under
        # activation recompute the adapters' main_grad must stay visible
        ctx.weight, ctx.A, ctx.B = weight, A, B
        ctx.scale = float(scale)
        ctx.has_bias, ctx.has_resid = bias is not None, resid is not None
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x, t = ctx.saved_tensors
        weight, A, B = ctx.weight, ctx.A, ctx.B
        K, N = x.shape[-1], dy.shape[-1]
        dy2 = dy.reshape(-1, N)
        x2 = x.reshape(-1, K)
        dts = lora_shrink(dy2, B, ctx.scale, transposed=True)  # bf16(scale * dy B)
        dA = dB = None
        if ctx.needs_input_grad[3] and not accumulate_weight_grad(B, dy2, t):
            dB = dy2.t() @ t
        if ctx.needs_input_grad[2] and not accumulate_weight_grad(A, dts, x2):
            dA = dts.t() @ x2
        dx = None
        if ctx.needs_input_grad[0]:
            dx2 = input_grad(dy2, weight)
            if dx2.data_ptr() == dy2.data_ptr():  # never write into the incoming gradient
                dx2 = dx2.clone()
            lora_expand_add_(dx2, dts, A, transposed=True)
            dx = dx2.view(x.shape)
        db = dy2.sum(0) if (ctx.has_bias and ctx.needs_input_grad[4]) else None
        dres = dy if (ctx.has_resid and ctx.needs_input_grad[5]) else None
        return dx, None, dA, dB, db, dres, None


def _lora_linear_composition(x, weight, A, B, scale, bias, resid, dropout):
    """Plain-autograd composition, adapter dropout included (F.dropout feeds the adapter branch
    only); the rounding points are those of the formula of record."""
    y0 = F.linear(x, weight, bias)
    if resid is not None:
        y0 = y0 + resid
    xd = F.dropout(x, dropout, training=True) if dropout > 0.0 else x
    t = (float(scale) * F.linear(xd.float(), A.float())).to(x.dtype)
    return (y0.float() + F.linear(t.float(), B.float())).to(x.dtype)


def lora_linear(x: torch.Tensor, weight: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: float,
                bias=None, resid=None, dropout: float = 0.0, training: bool = False) -> torch.Tensor:
    """linear(x, weight, bias) [+ resid] + scale * (x A^T) B^T with a frozen `weight`
    ([N, K]; A [r, K], B [N, r]). `dropout` > 0 in training mode runs the torch composition end
    to end; the kernels serve dropout == 0."""
    if weight.requires_grad:
        raise ValueError("lora_linear: the base weight must be frozen (requires_grad=False)")
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != x.shape[-1] or B.shape[1] != A.shape[0] \
            or B.shape[0] != weight.shape[0] or weight.shape[1] != x.shape[-1]:
        raise ValueError(f"lora_linear: shapes x {tuple(x.shape)} W {tuple(weight.shape)} A {tuple(A.shape)} "
                         f"B {tuple(B.shape)} do not fit y = x W^T + s (x A^T) B^T")
    if bias is not None and resid is not None:
        raise ValueError("lora_linear: bias and resid are exclusive (the residual GEMM has no bias)")
    if dropout > 0.0 and training:
        return _lora_linear_composition(x, weight, A, B, scale, bias, resid, float(dropout))
    return _LoRALinearFn.apply(x, weight, A, B, bias, resid, float(scale))
