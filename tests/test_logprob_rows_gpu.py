"""GPU tier: the plain LM-head row kernels of csrc/logprob.hip (logprob_fwd, row_lse, logprob_bwd,
ensemble_kl) against fp64, elementwise, on finite rows and on rows with -inf logits (masked
vocabulary entries; never a whole row).

-inf patterns on one row: indices 0..15 (a lane's whole first 8-vector on the vector path, the
first element of 16 threads on the scalar path), a scattered 37::5 pattern, and index V - 1.
That row's target sits on a -inf logit: logp = -inf there, lse stays finite.

Bound (see _refs64): 8 * E32 + 4 ulp32(max |ref|), E32 from the fp32 log-softmax of the same
bf16 logits (the package's CPU formula); bf16 outputs add one bf16 ulp of the reference element.
The exponent arguments are not small here (x - lse reaches -30 at V = 50264, so the hardware exp
is good to about 3e-6 relative on the smallest terms), but those terms carry no weight in the
sums; no case needed a term beyond the margin.
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext

import _branch32 as B32
import _refs64 as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _rows(kind, pattern):
    x = R.rows_case(kind).clone()
    N, V = x.shape
    tgt = R.rows_targets(N, V)
    dead = None
    if pattern is not None:
        dead = R.dead_mask(V, pattern)
        x[R.DEAD_ROW, dead] = R.NINF
        tgt[R.DEAD_ROW] = int(dead.nonzero()[0])  # this row's target sits on a -inf logit
    if kind == "sliced":  # the same strided view on the device
        xd = torch.zeros(N, 2112, dtype=torch.bfloat16)
        xd[:, 8:2056] = x
        xd = xd.to(DEV)[:, 8:2056]
        assert xd.stride(0) == 2112
    else:
        xd = x.to(DEV)
    return x, xd, tgt, dead


@pytest.mark.parametrize("pattern", [None] + R.DEAD_PATTERNS)
@pytest.mark.parametrize("kind", R.ROW_V + ["sliced"])
def test_logprob_rows(kind, pattern):
    k = _ext.require()
    x, xd, tgt, dead = _rows(kind, pattern)
    N, V = x.shape
    td = tgt.to(DEV)
    ref = R.logprob64(x, tgt)
    cpu = B32.logprob(x, tgt)
    assert torch.isfinite(ref["lse"]).all()

    lp, lse = k.logprob_fwd(xd, td)
    lp2, lse2 = k.logprob_fwd(xd, td)
    assert torch.equal(lse, lse2) and torch.equal(lp, lp2)  # (NaN != NaN: a NaN lse fails here too)
    assert torch.isfinite(lse).all(), f"logprob_fwd lse not finite: {lse.tolist()}"
    R.check("logprob_fwd", "lse", lse, ref["lse"], R.e32_of(cpu["lse"], ref["lse"]))
    # logp = x_t - lse: the same error; -inf where the target is a -inf logit, 0 on the ignored row
    R.check("logprob_fwd", "logp", lp, ref["logp"], R.e32_of(cpu["logp"], ref["logp"]))
    assert lp[3].item() == 0
    if pattern is not None:
        assert lp[R.DEAD_ROW].item() == R.NINF

    rl = k.row_lse(xd)
    assert torch.isfinite(rl).all(), f"row_lse not finite: {rl.tolist()}"
    R.check("row_lse", "lse", rl, ref["lse"], R.e32_of(cpu["lse"], ref["lse"]))
    assert torch.equal(rl, k.row_lse(xd))

    # the entropy twin promises logprob_fwd's logp and lse bit for bit, on these rows too
    lpe, lsee, ent = k.logprob_entropy_fwd(xd, td)
    assert torch.equal(lsee, lse) and torch.equal(lpe, lp)
    assert torch.isfinite(ent).all()

    # backward, fed the fp64 lse rounded to fp32 (so it does not depend on the forward above)
    g = torch.randn(N, generator=R.gen(5))
    want = R.logprob_bwd64(x, tgt, g)
    e32 = R.e32_of(B32.logprob_bwd(x, tgt, g), want)
    a = xd.clone()
    k.logprob_bwd(a, td, ref["lse"].float().to(DEV), g.to(DEV))
    b = xd.clone()
    k.logprob_bwd(b, td, ref["lse"].float().to(DEV), g.to(DEV))
    assert torch.equal(a, b)
    assert a.stride(0) == V  # (clone of the sliced view is dense; the strided write is below)
    R.check("logprob_bwd", "dlogits", a, want, e32, bf16=True)
    assert (a[3] == 0).all()  # ignored row
    if pattern is not None:
        got_dead = a[R.DEAD_ROW].cpu()[dead]
        assert (got_dead == 0).all(), f"-inf positions must receive exact 0, got {got_dead[got_dead != 0][:4].tolist()}"
    if kind == "sliced":  # in place on the strided view; the columns outside stay untouched
        big = torch.zeros(N, 2112, dtype=torch.bfloat16, device=DEV)
        big[:, 8:2056] = xd
        big[:, :8] = 7.0
        big[:, 2056:] = 7.0
        k.logprob_bwd(big[:, 8:2056], td, ref["lse"].float().to(DEV), g.to(DEV))
        assert torch.equal(big[:, 8:2056], a)
        assert (big[:, :8] == 7.0).all() and (big[:, 2056:] == 7.0).all()


@pytest.mark.parametrize("pattern", R.DEAD_PATTERNS)
def test_logprob_bwd_t_inf_rows(pattern):
    """The transposing backward shares the element formula: on rows with -inf logits it writes
    logprob_bwd's bits in place (exact 0 at the -inf positions) and their transpose."""
    k = _ext.require()
    N, V = 16, 2048
    x = R.rows_case(V, N=N, seed=4)
    tgt = R.rows_targets(N, V)
    dead = R.dead_mask(V, pattern)
    x[R.DEAD_ROW, dead] = R.NINF
    tgt[R.DEAD_ROW] = int(dead.nonzero()[0])
    lse = R.logprob64(x, tgt)["lse"].float().to(DEV)
    g = torch.randn(N, generator=R.gen(6)).to(DEV)
    a, b = x.to(DEV), x.to(DEV)
    k.logprob_bwd(a, tgt.to(DEV), lse, g)
    bt = k.logprob_bwd_t(b, tgt.to(DEV), lse, g)
    assert bt.shape == (V, N)
    assert torch.equal(a, b) and torch.equal(bt, a.t())
    assert (b[R.DEAD_ROW].cpu()[dead] == 0).all()


@pytest.mark.parametrize("K", R.ENS_K)
@pytest.mark.parametrize("N,V", R.ENS_SHAPES)
def test_ensemble_kl(N, V, K):
    """Forward and in-place gradient through the public op (row_lse of student and teachers, then
    the KL kernel); the last teacher has -inf logits, so with K = 1 p_bar is 0 at some positions."""
    c = R.ensemble_case(N, V, K)
    ref = R.ensemble_kl64(**c)
    cpu = B32.ensemble_kl(**c)
    sd = c["s"].to(DEV).requires_grad_(True)
    tdv = c["t"].to(DEV)
    kl = ops.ensemble_kl(sd, tdv)
    (grad,) = torch.autograd.grad(kl, sd, c["g"].to(DEV))
    sd2 = c["s"].to(DEV).requires_grad_(True)
    kl2 = ops.ensemble_kl(sd2, tdv)
    (grad2,) = torch.autograd.grad(kl2, sd2, c["g"].to(DEV))
    assert torch.equal(kl, kl2) and torch.equal(grad, grad2)
    assert grad.dtype == torch.bfloat16
    R.check("ensemble_kl", f"kl K={K}", kl.detach(), ref["kl"], R.e32_of(cpu["kl"], ref["kl"]))
    R.check("ensemble_kl", f"grad K={K}", grad, ref["grad"], R.e32_of(cpu["grad"], ref["grad"]), bf16=True)
