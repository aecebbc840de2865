"""fp64 reference, closed-form gradient and case builders for the generalised JSD(beta) distillation
loss (test_gkd_cpu.py, test_gkd_gpu.py).

Written from the docstring of `ops.generalized_jsd` and the README section "On-policy distillation
(GKD)"; nothing here imports the package's ops and nothing needs a GPU. With i = inv_temp,
q = softmax(i s), p = (1/K) sum_k softmax(i t_k), m = beta p + (1 - beta) q:

    beta = 0      L = sum_v p (log p - log q)
    beta = 1      L = A,  A = sum_v q (log q - log p)
    0 < beta < 1  L = beta sum_v p (log p - log m) + (1 - beta) A,  A = sum_v q (log q - log m)
    dL/ds_v = g i (q_v - p_v)                       beta = 0
    dL/ds_v = g i c q_v (log q_v - log m_v - A)     beta > 0, c = 1 - beta (beta = 1: c = 1, m = p)

q_v = 0 adds exactly 0 to A and has gradient exactly 0; p_v = 0 adds exactly 0 to the p sums. The
gradient is the closed form, not autograd: on a row with -inf logits fp64 autograd returns NaN (the
`_refs64` convention for branch conventions). `forward` is dtype-generic: `_branch32_gkd` runs the
same closed-form gradient in fp32.

Scalars follow the `_refs64` rule: `inv32(T)` is the fp32 inv_temp the kernel receives, widened;
beta is the stated constant.

Builders: bf16 logits, scale 2-3; row DEAD carries -inf student entries (one of R.DEAD_PATTERNS),
the last teacher carries -inf at 5::7 and :16 on every row, the GAP row has student +100 at index 10
and every teacher +100 at index 20. The -inf sets are placed so that the mathematics stays finite:
beta = 0: the teachers' dead set contains the student's (the student has none of its own);
beta = 1: the student's contains the teachers' (the teachers have none); 0 < beta < 1: both free.
Each builder asserts in fp64 that its own L is finite.
"""
import math

import torch

import _refs64 as R

F64 = torch.float64
BETAS = [0.0, 0.1, 0.5, 0.9, 1.0]
TEMPS = [1.0, 0.9, 0.5]
DEAD = 2  # the row with -inf student logits (cases with N > DEAD)
GAP_V = 1003


def inv32(tau):
    """float(1.0 / tau): the divide in double, rounded once to fp32 (returned as a Python float)."""
    return torch.tensor(1.0 / float(tau), dtype=F64).float().item()


def _logs(s, t, it, dt):
    i = torch.tensor(it, dtype=dt)
    lq = torch.log_softmax(s.to(dt) * i, -1)
    lpk = torch.log_softmax(t.to(dt) * i, -1)
    K = t.shape[0]
    lp = lpk[0] if K == 1 else torch.logsumexp(lpk, 0) - math.log(K)
    return lq, lp, lpk


def _zsum(w, a, b):
    """sum_v w (a - b) with the entries of w = 0 (a = -inf) adding exactly 0."""
    dead = a == R.NINF
    z = torch.zeros_like(a)
    return torch.where(dead, z, w * (torch.where(dead, z, a) - b)).sum(-1)


def _logm(lp, lq, beta):
    if beta == 1.0:
        return lp
    both = (lp == R.NINF) & (lq == R.NINF)
    z = torch.zeros_like(lp)
    lm = torch.logaddexp(torch.where(both, z, lp + math.log(beta)), torch.where(both, z, lq + math.log1p(-beta)))
    return torch.where(both, torch.full_like(lp, R.NINF), lm)


def forward(s, t, beta, it, mask=None, dt=F64):
    """{"loss", "aux", "s_lse", "t_lse"} in dtype dt; masked rows 0 everywhere."""
    lq, lp, _ = _logs(s, t, it, dt)
    i = torch.tensor(it, dtype=dt)
    out = {"s_lse": torch.logsumexp(s.to(dt) * i, -1), "t_lse": torch.logsumexp(t.to(dt) * i, -1)}
    if beta == 0.0:
        out["loss"] = _zsum(lp.exp(), lp, lq)
        out["aux"] = torch.zeros_like(out["loss"])
    else:
        lm = _logm(lp, lq, beta)
        A = _zsum(lq.exp(), lq, lm)
        out["aux"] = A
        out["loss"] = A if beta == 1.0 else beta * _zsum(lp.exp(), lp, lm) + (1.0 - beta) * A
    if mask is not None:
        live = mask.to(dt) != 0
        out = {k: v * live for k, v in out.items()}
    return out


def grad(s, t, beta, it, g, mask=None, dt=F64, aux=None):
    """Closed-form dL/ds [N, V] for the upstream gradient g [N]; `aux`: the row scalar A to use
    (default: this dtype's own)."""
    lq, lp, _ = _logs(s, t, it, dt)
    q = lq.exp()
    gi = g.to(dt).unsqueeze(-1) * torch.tensor(it, dtype=dt)
    if beta == 0.0:
        out = gi * (q - lp.exp())
    else:
        A = forward(s, t, beta, it, None, dt)["aux"] if aux is None else aux.to(dt)
        lm = _logm(lp, lq, beta)
        dead = lq == R.NINF
        z = torch.zeros_like(lq)
        c = 1.0 if beta == 1.0 else 1.0 - beta
        out = torch.where(dead, z, gi * c * q * (torch.where(dead, z, lq) - torch.where(dead, z, lm) - A.unsqueeze(-1)))
    if mask is not None:
        out = out * (mask.to(dt) != 0).unsqueeze(-1)
    return out


def case(N, V, K, beta, seed=0, pattern="scattered", ld=None, t_ld=None):
    """{"s" [N, V], "t" [K, N, V] bf16, "g" [N] fp32}. `ld` / `t_ld`: the operand is the [:, 8:8+V]
    column slice of a buffer that wide (row stride != V)."""
    g = R.gen(14000 + V + 17 * K + int(100 * beta) + seed)

    def buf(shape, width, scale):
        if width is None:
            return (scale * torch.randn(*shape, V, generator=g)).bfloat16()
        return (scale * torch.randn(*shape, width, generator=g)).bfloat16()[..., 8:8 + V]

    s = buf((N,), ld, 3.0)
    t = buf((K, N), t_ld, 2.0)
    if beta < 1.0:  # teacher -inf: allowed unless the reverse KL would divide by it
        t[K - 1, :, 5::7] = R.NINF
        t[K - 1, :, :16] = R.NINF
    if N > DEAD and beta > 0.0:  # student -inf: allowed unless the forward KL would divide by it
        s[DEAD, R.dead_mask(V, pattern)] = R.NINF
    if N > DEAD and beta == 0.0 and K == 1:  # contained in the teacher's dead set: still finite
        s[DEAD, 5::14] = R.NINF
    out = {"s": s, "t": t, "g": torch.randn(N, generator=g)}
    assert torch.isfinite(forward(s, t, beta, 1.0)["loss"]).all()
    return out


def gap_case(K, beta, seed=0, V=GAP_V):
    """One row: randn logits, student +100 at index 10, every teacher +100 at index 20."""
    g = R.gen(15000 + K + seed)
    s = torch.randn(1, V, generator=g).bfloat16()
    t = torch.randn(K, 1, V, generator=g).bfloat16()
    s[0, 10] = 100.0
    t[:, 0, 20] = 100.0
    assert torch.isfinite(forward(s, t, beta, 2.0)["loss"]).all()
    return {"s": s, "t": t, "g": torch.randn(1, generator=g)}
