"""fp64 references for the temperature-aware LM-head row kernels, wrappers and sampler log-prob
(test_logprob_temperature_cpu.py, test_logprob_temperature_gpu.py).

Written from the formulas of the README section "Log-probs at the sampling temperature"; nothing
here imports the package's ops and nothing needs a GPU. With i = inv_temp = 1 / tau and y = i z for
the bf16 logits z:

    lse  = logsumexp_v y_v            logp = y_t - lse           H = -sum_v p_v (y_v - lse)
    dz_v = i [ g (1[v = t] - p_v) - e p_v (y_v - lse + H) ],     p_v = exp(y_v - lse)

Rows with tgt < 0 give logp 0 and gradient 0; a -inf logit has p = 0, adds exactly 0 to every sum
and receives gradient exactly 0.

Scalar arguments follow the `_refs64` rule: the reference uses the fp32 `inv_temp` the kernel
receives (`inv32`: 1 / tau divided in double, rounded once to fp32), widened to fp64. 0.5 and 2.0
have exact inverses; 0.7 does not.

`rows32` / `bwd32` are the fp32 CPU formula of record, log_softmax(logits.float() * i), on the same
logits: the E32 of the `_refs64` bound.
"""
import torch

import _refs64 as R

F64 = torch.float64
TEMPS = [0.5, 0.7, 2.0]


def inv32(tau):
    """float(1.0 / tau): the divide in double, rounded once to fp32 (returned as a Python float)."""
    return torch.tensor(1.0 / float(tau), dtype=F64).float().item()


def _rows(y, tgt):
    lse = torch.logsumexp(y, -1)
    lsm = y - lse.unsqueeze(-1)
    lp = lsm.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    ent = -(lsm.exp() * lsm.masked_fill(y == R.NINF, 0.0)).sum(-1)
    return {"logp": torch.where(tgt >= 0, lp, torch.zeros_like(lp)), "lse": lse, "ent": ent}


def rows64(x, tgt, it):
    """lse, logp (0 on ignored rows) and entropy (every row) of softmax(it * x), fp64."""
    return _rows(R.d(x) * float(it), tgt)


def rows32(x, tgt, it):
    """The same through the fp32 CPU formula: fp32 logits times the fp32 scalar, fp32 log-softmax."""
    return _rows(x.float() * torch.tensor(it, dtype=torch.float32), tgt)


def _bwd(y, tgt, g, e, it, lse, H):
    lsm = y - lse.unsqueeze(-1)
    p = lsm.exp()
    onehot = torch.zeros_like(y)
    onehot.scatter_(-1, tgt.clamp(min=0).unsqueeze(-1), 1.0)
    live = (tgt >= 0).to(y.dtype).unsqueeze(-1)
    out = g.unsqueeze(-1) * (onehot - p)
    if e is not None:
        out = out - e.unsqueeze(-1) * p * (lsm + H.unsqueeze(-1)).masked_fill(y == R.NINF, 0.0)
    return (it * out * live).masked_fill(y == R.NINF, 0.0)


def bwd64(x, tgt, g, e, it):
    """dz (e = None: the plain backward), fp64, from the fp64 lse and H of the same row."""
    y = R.d(x) * float(it)
    r = _rows(y, tgt)
    return _bwd(y, tgt, R.d(g), None if e is None else R.d(e), float(it), r["lse"], r["ent"])


def bwd32(x, tgt, g, e, it):
    t = torch.tensor(it, dtype=torch.float32)
    y = x.float() * t
    r = _rows(y, tgt)
    return _bwd(y, tgt, g.float(), None if e is None else e.float(), t, r["lse"], r["ent"])


def linear64(h, W, tgt, it, g=None, e=None):
    """The wrapper's formula in fp64 on bf16-rounded logits (the model's logits are bf16): values
    (logp, ent; 0 on ignored rows) and, with g (and e), the gradients of sum(g logp + e ent) with
    respect to hidden and weight."""
    hr = R.d(h).requires_grad_(True)
    Wr = R.d(W).requires_grad_(True)
    z = hr @ Wr.t()
    z = z + (z.detach().to(torch.bfloat16).to(F64) - z.detach())  # bf16 rounding, straight-through
    r = _rows(z * float(it), tgt)
    ent = torch.where(tgt >= 0, r["ent"], torch.zeros_like(r["ent"]))
    out = {"logp": r["logp"].detach(), "ent": ent.detach()}
    if g is not None:
        loss = (r["logp"] * R.d(g)).sum()
        if e is not None:
            loss = loss + (ent * R.d(e)).sum()
        out["dh"], out["dW"] = torch.autograd.grad(loss, (hr, Wr))
    return out


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-30)).item()
