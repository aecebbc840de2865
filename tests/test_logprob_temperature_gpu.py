"""GPU tier: the tempered LM-head row kernels (`*_temp` ops of csrc/logprob.hip) and the autograd
wrappers on top of them, against the fp64 formulas of _refs64_temp.

Bound: the `_refs64` rule, MARGIN * E32 + FLOOR_ULPS ulp32(max |ref|) + extra, plus one bf16 ulp on
bf16 outputs. E32 is the error of the fp32 CPU formula log_softmax(logits.float() * i) on the same
logits. No case takes an `extra`: the exponent arguments double at tau = 0.5, and the hardware exp
on them stays inside MARGIN * E32 + the floor.

At inv_temp = 1.0 every tempered op must give its plain twin's bits (a multiply by 1.0f is exact).
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext

import _refs64 as R
import _refs64_temp as RT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = R.ROW_V + ["sliced"]
PATTERNS = [None] + R.DEAD_PATTERNS


def _rows(kind, pattern, N=R.ROW_N, seed=0):
    x = R.rows_case(kind, N=N, seed=seed).clone()
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


def _ge(N):
    return torch.randn(N, generator=R.gen(5)), torch.randn(N, generator=R.gen(7))


# ------------------------------------------------------------------ row kernels against fp64
@pytest.mark.parametrize("tau", RT.TEMPS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", KINDS)
def test_tempered_rows(kind, pattern, tau):
    k = _ext.require()
    it = RT.inv32(tau)
    x, xd, tgt, dead = _rows(kind, pattern)
    N, V = x.shape
    td = tgt.to(DEV)
    ref = RT.rows64(x, tgt, it)
    cpu = RT.rows32(x, tgt, it)
    assert torch.isfinite(ref["lse"]).all() and torch.isfinite(ref["ent"]).all()

    lp, lse = k.logprob_fwd_temp(xd, td, it)
    lp2, lse2 = k.logprob_fwd_temp(xd, td, it)
    assert torch.equal(lse, lse2) and torch.equal(lp, lp2)
    lpe, lsee, ent = k.logprob_entropy_fwd_temp(xd, td, it)
    lpe2, lsee2, ent2 = k.logprob_entropy_fwd_temp(xd, td, it)
    assert torch.equal(lsee, lsee2) and torch.equal(lpe, lpe2) and torch.equal(ent, ent2)
    for name, a, b, e in (("fwd", lp, lse, None), ("entropy_fwd", lpe, lsee, ent)):
        assert torch.isfinite(b).all(), f"{name} lse not finite: {b.tolist()}"
        R.check(f"logprob_{name}_temp tau={tau}", "lse", b, ref["lse"], R.e32_of(cpu["lse"], ref["lse"]))
        R.check(f"logprob_{name}_temp tau={tau}", "logp", a, ref["logp"], R.e32_of(cpu["logp"], ref["logp"]))
        assert a[3].item() == 0  # the ignored row
        if pattern is not None:
            assert a[R.DEAD_ROW].item() == R.NINF
        if e is not None:
            R.check(f"logprob_{name}_temp tau={tau}", "ent", e, ref["ent"], R.e32_of(cpu["ent"], ref["ent"]))

    # backward, fed the fp64 lse / H rounded to fp32 (so it does not depend on the forward above)
    g, e = _ge(N)
    lse_d, ent_d = ref["lse"].float().to(DEV), ref["ent"].float().to(DEV)
    gd, ed = g.to(DEV), e.to(DEV)

    def plain(buf):
        k.logprob_bwd_temp(buf, td, lse_d, gd, it)

    def entropy(buf):
        k.logprob_entropy_bwd_temp(buf, td, lse_d, ent_d, gd, ed, it)

    for name, run, ee in (("bwd", plain, None), ("entropy_bwd", entropy, e)):
        want = RT.bwd64(x, tgt, g, ee, it)
        e32 = R.e32_of(RT.bwd32(x, tgt, g, ee, it), want)
        a, b = xd.clone(), xd.clone()
        run(a)
        run(b)
        assert torch.equal(a, b)
        R.check(f"logprob_{name}_temp tau={tau}", "dlogits", a, want, e32, bf16=True)
        assert (a[3] == 0).all()  # ignored row
        if pattern is not None:
            got_dead = a[R.DEAD_ROW].cpu()[dead]
            assert (got_dead == 0).all(), f"-inf positions must receive exact 0, got {got_dead[got_dead != 0][:4]}"
        if kind == "sliced":  # in place on the strided view; the columns outside stay untouched
            big = torch.zeros(N, 2112, dtype=torch.bfloat16, device=DEV)
            big[:, 8:2056] = xd
            big[:, :8] = 7.0
            big[:, 2056:] = 7.0
            run(big[:, 8:2056])
            assert torch.equal(big[:, 8:2056], a)
            assert (big[:, :8] == 7.0).all() and (big[:, 2056:] == 7.0).all()


# -------------------------------------------------------------------- transposing kernels
def _t_case(pattern):
    N, V = 16, 2048
    x = R.rows_case(V, N=N, seed=4)
    tgt = R.rows_targets(N, V)
    dead = None
    if pattern is not None:
        dead = R.dead_mask(V, pattern)
        x[R.DEAD_ROW, dead] = R.NINF
        tgt[R.DEAD_ROW] = int(dead.nonzero()[0])
    return x, tgt, dead


@pytest.mark.parametrize("tau", RT.TEMPS)
@pytest.mark.parametrize("pattern", R.DEAD_PATTERNS)
def test_tempered_bwd_t(pattern, tau):
    """The tempered transposing kernels write the tempered in-place kernel's bits and their exact
    transpose."""
    k = _ext.require()
    it = RT.inv32(tau)
    x, tgt, dead = _t_case(pattern)
    N, V = x.shape
    ref = RT.rows64(x, tgt, it)
    lse, ent = ref["lse"].float().to(DEV), ref["ent"].float().to(DEV)
    g, e = (t.to(DEV) for t in _ge(N))
    td = tgt.to(DEV)
    a, b = x.to(DEV), x.to(DEV)
    k.logprob_bwd_temp(a, td, lse, g, it)
    bt = k.logprob_bwd_t_temp(b, td, lse, g, it)
    assert bt.shape == (V, N)
    assert torch.equal(a, b) and torch.equal(bt, a.t())
    assert (b[R.DEAD_ROW].cpu()[dead] == 0).all()
    a, b = x.to(DEV), x.to(DEV)
    k.logprob_entropy_bwd_temp(a, td, lse, ent, g, e, it)
    bt = k.logprob_entropy_bwd_t_temp(b, td, lse, ent, g, e, it)
    assert torch.equal(a, b) and torch.equal(bt, a.t())
    assert (b[R.DEAD_ROW].cpu()[dead] == 0).all()


# --------------------------------------------------------------------- bit for bit at tau = 1
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", KINDS)
def test_unit_temperature_is_bitwise_the_plain_ops(kind, pattern):
    k = _ext.require()
    x, xd, tgt, dead = _rows(kind, pattern)
    N, V = x.shape
    td = tgt.to(DEV)
    lp, lse = k.logprob_fwd(xd, td)
    lpt, lset = k.logprob_fwd_temp(xd, td, 1.0)
    assert torch.equal(lse, lset), (lse - lset).abs().max().item()
    assert torch.equal(lp, lpt)
    lp, lse, ent = k.logprob_entropy_fwd(xd, td)
    lpt, lset, entt = k.logprob_entropy_fwd_temp(xd, td, 1.0)
    assert torch.equal(lse, lset), (lse - lset).abs().max().item()
    assert torch.equal(lp, lpt)
    assert torch.equal(ent, entt), (ent - entt).abs().max().item()
    g, e = (t.to(DEV) for t in _ge(N))
    a, b = xd.clone(), xd.clone()
    k.logprob_bwd(a, td, lse, g)
    k.logprob_bwd_temp(b, td, lse, g, 1.0)
    assert torch.equal(a, b)
    a, b = xd.clone(), xd.clone()
    k.logprob_entropy_bwd(a, td, lse, ent, g, e)
    k.logprob_entropy_bwd_temp(b, td, lse, ent, g, e, 1.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_unit_temperature_transposed_is_bitwise_the_plain_ops(pattern):
    k = _ext.require()
    x, tgt, dead = _t_case(pattern)
    N, V = x.shape
    td = tgt.to(DEV)
    _, lse, ent = k.logprob_entropy_fwd(x.to(DEV), td)
    g, e = (t.to(DEV) for t in _ge(N))
    a, b = x.to(DEV), x.to(DEV)
    at = k.logprob_bwd_t(a, td, lse, g)
    bt = k.logprob_bwd_t_temp(b, td, lse, g, 1.0)
    assert torch.equal(a, b) and torch.equal(at, bt)
    a, b = x.to(DEV), x.to(DEV)
    at = k.logprob_entropy_bwd_t(a, td, lse, ent, g, e)
    bt = k.logprob_entropy_bwd_t_temp(b, td, lse, ent, g, e, 1.0)
    assert torch.equal(a, b) and torch.equal(at, bt)


def test_inv_temp_must_be_finite_and_positive():
    k = _ext.require()
    x, xd, tgt, _ = _rows(2048, None)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError):
            k.logprob_fwd_temp(xd, tgt.to(DEV), bad)


# ------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("tau", RT.TEMPS)
def test_tempered_shards_compose(tau):
    """V = 2048 split at 1024 through vocab_offset: lse = logsumexp_l lse_l, the target logit is
    logp_l + lse_l of the owner, H = lse - sum_l w_l (lse_l - H_l); the shard backward with the
    global lse / H gives the full backward's columns bitwise."""
    k = _ext.require()
    it = RT.inv32(tau)
    x, xd, tgt, _ = _rows(2048, None)
    N, V = x.shape
    td = tgt.to(DEV)
    ref = RT.rows64(x, tgt, it)
    cpu = RT.rows32(x, tgt, it)
    shards = [(xd[:, :1024], 0), (xd[:, 1024:], 1024)]
    outs = [k.logprob_entropy_fwd_temp(xs, td, it, off) for xs, off in shards]
    lse_l = torch.stack([o[1] for o in outs]).double()
    H_l = torch.stack([o[2] for o in outs]).double()
    own = torch.stack([(td >= off) & (td < off + 1024) for _, off in shards])
    tl = torch.where(own, torch.stack([o[0] for o in outs]).double() + lse_l, torch.zeros_like(lse_l)).sum(0)
    lse = torch.logsumexp(lse_l, 0)
    H = lse - ((lse_l - lse).exp() * (lse_l - H_l)).sum(0)
    logp = torch.where(td >= 0, tl - lse, torch.zeros_like(lse))
    R.check(f"shards tau={tau}", "lse", lse, ref["lse"], R.e32_of(cpu["lse"], ref["lse"]))
    R.check(f"shards tau={tau}", "logp", logp, ref["logp"], R.e32_of(cpu["logp"], ref["logp"]))
    R.check(f"shards tau={tau}", "ent", H, ref["ent"], R.e32_of(cpu["ent"], ref["ent"]))
    for o in outs:  # a shard that does not own the target writes logp 0
        assert o[0][3].item() == 0
    assert (outs[0][0][(~own[0]).nonzero().flatten()] == 0).all()

    g, e = (t.to(DEV) for t in _ge(N))
    lse_d, ent_d = ref["lse"].float().to(DEV), ref["ent"].float().to(DEV)
    full, full_e = xd.clone(), xd.clone()
    k.logprob_bwd_temp(full, td, lse_d, g, it)
    k.logprob_entropy_bwd_temp(full_e, td, lse_d, ent_d, g, e, it)
    for (xs, off) in shards:
        a, b = xs.clone(), xs.clone()
        assert a.stride(0) == 1024
        k.logprob_bwd_temp(a, td, lse_d, g, it, off)
        k.logprob_entropy_bwd_temp(b, td, lse_d, ent_d, g, e, it, off)
        assert torch.equal(a, full[:, off:off + 1024])
        assert torch.equal(b, full_e[:, off:off + 1024])


# ------------------------------------------------------------------------------ autograd
def _bf(x):
    return x.to(device=DEV, dtype=torch.bfloat16)


@pytest.mark.parametrize("main_grad", [False, True])
@pytest.mark.parametrize("entropy", [False, True])
@pytest.mark.parametrize("tau", RT.TEMPS)
def test_linear_logprob_temperature(tau, entropy, main_grad, monkeypatch):
    """`linear_logprob(_entropy)(temperature=tau)` on [64, 128] x [2048, 128] against the fp64
    formula, to the bounds test_entropy_gpu.py gives the temperature-1 twin (2e-2 on the values,
    3e-2 rel-L2 on the gradients). With a main_grad on the weight the backward runs the
    transposing kernels; this weight is below the size from which the TN weight-gradient path is
    taken by default (ops.linear.TN_WGRAD_MIN_ELEMS), so the threshold is lowered for the test."""
    import importlib

    linmod = importlib.import_module("distributed_llm_alignment_amd.ops.linear")  # (ops.linear is the function)
    monkeypatch.setattr(linmod, "TN_WGRAD_MIN_ELEMS", 0)
    N, H, V = 64, 128, 2048
    gen = R.gen(40)
    h0 = torch.randn(N, H, generator=gen).bfloat16()
    W0 = (torch.randn(V, H, generator=gen) * 0.05).bfloat16()
    tgt = torch.randint(0, V, (N,), generator=gen)
    tgt[5] = -100
    g, e = torch.randn(N, generator=gen), torch.randn(N, generator=gen)
    ref = RT.linear64(h0, W0, tgt, RT.inv32(tau), g, e if entropy else None)

    calls = []
    k = _ext.require()
    names = ["logprob_bwd_temp", "logprob_bwd_t_temp", "logprob_entropy_bwd_temp", "logprob_entropy_bwd_t_temp",
             "logprob_bwd", "logprob_bwd_t", "logprob_entropy_bwd", "logprob_entropy_bwd_t"]

    class Spy:
        def __getattr__(self, name):
            fn = getattr(k, name)
            if name not in names:
                return fn

            def wrapped(*a, **kw):
                calls.append(name)
                return fn(*a, **kw)
            return wrapped

    h = h0.to(DEV).requires_grad_()
    W = W0.to(DEV).requires_grad_()
    if main_grad:
        W.main_grad = torch.zeros(V, H, device=DEV, dtype=torch.float32)
    td = tgt.to(DEV)
    orig = _ext.require
    _ext.require = lambda: Spy()
    try:
        if entropy:
            lp, ent = ops.linear_logprob_entropy(h, W, td, temperature=tau)
            (lp * g.to(DEV) + ent * e.to(DEV)).sum().backward()
        else:
            lp = ops.linear_logprob(h, W, td, temperature=tau)
            (lp * g.to(DEV)).sum().backward()
    finally:
        _ext.require = orig
    want_op = ("logprob_entropy_bwd" if entropy else "logprob_bwd") + ("_t" if main_grad else "") + "_temp"
    assert calls == [want_op], calls
    err = (lp.detach().double().cpu() - ref["logp"]).abs().max().item()
    print(f"FIG linear_logprob tau={tau} logp: err {err:.3e}")
    assert err < 2e-2 and lp[5] == 0
    if entropy:
        err = (ent.detach().double().cpu() - ref["ent"]).abs().max().item()
        print(f"FIG linear_logprob tau={tau} ent: err {err:.3e}")
        assert err < 2e-2 and ent[5] == 0
    dW = W.main_grad if main_grad else W.grad
    assert (W.grad is None) == main_grad
    eh, ew = RT.rel_l2(h.grad, ref["dh"]), RT.rel_l2(dW, ref["dW"])
    print(f"FIG linear_logprob tau={tau} rel-L2 dh {eh:.3e} dW {ew:.3e}")
    assert eh < 3e-2 and ew < 3e-2


def test_linear_logprob_unit_temperature_runs_the_plain_ops():
    """temperature=1.0 is the call without the keyword: the same ops, the same bits."""
    N, H, V = 64, 128, 2048
    gen = R.gen(41)
    h = _bf(torch.randn(N, H, generator=gen))
    W = _bf(torch.randn(V, H, generator=gen) * 0.05)
    tgt = torch.randint(0, V, (N,), generator=gen).to(DEV)
    g = torch.randn(N, generator=gen).to(DEV)
    outs = []
    for kw in ({}, {"temperature": 1.0}):
        h1, W1 = h.clone().requires_grad_(), W.clone().requires_grad_()
        lp, ent = ops.linear_logprob_entropy(h1, W1, tgt, **kw)
        (lp * g + ent * g).sum().backward()
        outs.append((lp.detach(), ent.detach(), h1.grad, W1.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_grad_chunks_carry_the_temperature():
    from distributed_llm_alignment_amd.ops import logprob as lpmod

    N, H, V = lpmod._NO_GRAD_CHUNK + 8, 64, 512
    gen = R.gen(42)
    h0 = torch.randn(N, H, generator=gen).bfloat16()
    W0 = (torch.randn(V, H, generator=gen) * 0.1).bfloat16()
    tgt = torch.randint(0, V, (N,), generator=gen)
    tgt[N - 3] = -100
    ref = RT.linear64(h0, W0, tgt, RT.inv32(0.7))
    with torch.no_grad():
        lp, ent = ops.linear_logprob_entropy(h0.to(DEV), W0.to(DEV), tgt.to(DEV), temperature=0.7)
        lp2 = ops.linear_logprob(h0.to(DEV), W0.to(DEV), tgt.to(DEV), temperature=0.7)
    assert (lp.double().cpu() - ref["logp"]).abs().max().item() < 2e-2
    assert (ent.double().cpu() - ref["ent"]).abs().max().item() < 2e-2
    assert torch.equal(lp, lp2)
    assert lp[N - 3] == 0 and ent[N - 3] == 0


# ==================================================================================== sampler
# `sample_tokens_logp_tempered`: logp[r] = log softmax(x_r * inv_temp)[token_r] over the full
# vocabulary, inv_temp the fp32 the kernel forms (float(1 / T)), NaN logits counted as -inf.
# Bound 2^-14, derived as in test_rollout_logprobs_gpu.py: the fp32 mass sum is within 2^-15
# relative (its accounting: chains of <= 128 adds per thread, 10 reduction levels, 32 chunk adds,
# __expf), at most 2^-15 absolute after the log; a drawn token has |z| <= 64 (the sampler's window),
# and z = (x - max) * inv_temp carries two fp32 roundings, 2^-24 * 128 = 7.6e-6; the fp32 log of a
# value in [1, V] adds under 3e-6; together about 4.2e-5 < 2^-14 = 6.1e-5.
import math  # noqa: E402

import _sampler_ref as S  # noqa: E402
import test_rollout_logprobs_gpu as RL  # noqa: E402  (its model / prompt builders and layouts)

LOGP_TOL = 2.0 ** -14
INF = float("inf")
SAMPLER_GRID = [(4099, torch.float32, "single-scalar"), (4096, torch.bfloat16, "single-vec"),
                (32768, torch.bfloat16, "split"), (128256, torch.bfloat16, "split")]
SAMPLER_MODES = (("plain", "dense", 0, 1.0), ("k50", "dense", 50, 1.0), ("p0.9", "peaked", 0, 0.9),
                 ("k50-p0.9", "peaked", 50, 0.9))
SAMPLER_TEMPS = (0.7, 1.3)


@pytest.fixture(scope="module", autouse=True)
def _graphs():
    yield
    from distributed_llm_alignment_amd.models.generation import clear_graph_cache

    clear_graph_cache()


def _ref_tempered(x, T):
    xd = x.double()
    xd = torch.where(torch.isnan(xd), torch.full_like(xd, -INF), xd)
    return torch.log_softmax(xd * RT.inv32(T), -1)


def check_tempered(x, T, k, p, seed=7, counters=(0, 1, 2), mode=""):
    """Tokens bitwise `sample_tokens`', two launches bitwise equal, logp within LOGP_TOL of fp64 on
    defined rows and exactly 0 on rows whose max is not finite."""
    from distributed_llm_alignment_amd.ops import decode

    ref = _ref_tempered(x, T)
    xf = x.float()
    rowmax = torch.where(torch.isnan(xf), torch.full_like(xf, -INF), xf).max(-1).values
    defined = torch.isfinite(rowmax)
    toks, lps, worst = [], [], 0.0
    for c in counters:
        rng = torch.tensor([seed, c], dtype=torch.long, device=x.device)
        plain = decode.sample_tokens(x, T, k, p, False, rng)
        tok, lp = decode.sample_tokens_logp_tempered(x, T, k, p, False, rng)
        tok2, lp2 = decode.sample_tokens_logp_tempered(x, T, k, p, False, rng)
        assert tok.dtype == torch.long and lp.dtype == torch.float32 and lp.shape == tok.shape == (x.shape[0],)
        assert torch.equal(tok, plain), "tokens differ from sample_tokens"
        assert torch.equal(tok, tok2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))
        want = ref.gather(1, tok.unsqueeze(1)).squeeze(1)
        if bool(defined.any()):
            worst = max(worst, float((lp.double() - want).abs()[defined].max()))
        assert torch.equal(lp[~defined], torch.zeros_like(lp[~defined])), "undefined rows must write exactly 0.0"
        toks.append(tok)
        lps.append(lp)
    print(f"FIG sampler_tempered path={RL.path_of(x)} mode={mode} T={T} V={x.shape[1]} rows={x.shape[0]} "
          f"worst_err={worst:.3e} tol={LOGP_TOL:.3e}")
    assert worst <= LOGP_TOL, worst
    return torch.stack(toks, 1), torch.stack(lps, 1)


@pytest.mark.parametrize("T", SAMPLER_TEMPS)
@pytest.mark.parametrize("mode", SAMPLER_MODES, ids=lambda m: m[0])
@pytest.mark.parametrize("V,dtype,path", SAMPLER_GRID, ids=lambda v: str(v).replace("torch.", ""))
def test_sampler_tempered_logp_matches_fp64(V, dtype, path, mode, T):
    name, builder, k, p = mode
    x = S.grid_logits(builder, V, dtype).to(DEV)
    if RL.SPLIT_ON:
        assert RL.path_of(x) == path
    tok, lp = check_tempered(x, T, k, p, mode=name)
    assert bool((lp <= 0).all()) and bool(torch.isfinite(lp).all())
    # not the temperature-1 value: the two ops differ where the temperature is not 1
    from distributed_llm_alignment_amd.ops import decode

    _, lp1 = decode.sample_tokens_logp(x, T, k, p, False, torch.tensor([7, 0], dtype=torch.long, device=DEV))
    assert not torch.equal(lp1, lp[:, 0])


@pytest.mark.parametrize("V", [4096, 32768])
def test_sampler_tempered_edges(V):
    from distributed_llm_alignment_amd.ops import decode

    draws = ((0, 1.0), (50, 1.0), (0, 0.9), (50, 0.9))
    # NaN counts as -inf
    g = torch.Generator().manual_seed(31)
    x = S.peaked(64, V, 31)
    r = torch.rand(64, V, generator=g)
    x[r < 0.1] = float("nan")
    x[(r >= 0.1) & (r < 0.2)] = -INF
    x[:, 0] = float("nan")
    x[:, V - 1] = -INF
    x = x.to(torch.bfloat16).to(DEV)
    for y in RL.layouts(x):
        for k, p in draws:
            _, lp = check_tempered(y, 0.7, k, p, mode="nan-inf")
            assert bool(torch.isfinite(lp).all())
    # undefined rows (a +inf, or no finite logit) write exactly 0; a finite row beside them is unaffected
    x = S.dense(7, V, 37)
    x[0, 7] = INF
    x[1, V - 1] = INF
    x[1, 3] = float("nan")
    x[2, 2 * 1024] = x[2, 2 * 1024 + 9] = INF
    x[3] = -INF
    x[4] = float("nan")
    x[5, ::2] = -INF
    x[5, 1::2] = float("nan")
    x = x.to(torch.bfloat16).to(DEV)
    for y in RL.layouts(x):
        for k, p in draws:
            tok, lp = check_tempered(y, 0.7, k, p, seed=5, mode="undefined-rows")
            assert tok[:6, 0].tolist() == [7, V - 1, 2 * 1024, 0, 0, 0]
            assert torch.equal(lp[:6], torch.zeros_like(lp[:6])) and bool((lp[6] < 0).all())
    # one finite logit: log-prob 0
    pos = [0, 7, V - 1, 2 * 1024, 2 * 1024 + 1023, V // 2 + 3]
    x = torch.full((len(pos), V), -INF, dtype=torch.bfloat16, device=DEV)
    for i, j in enumerate(pos):
        x[i, j] = -3.0
    for y in RL.layouts(x):
        for k, p in draws:
            tok, lp = check_tempered(y, 0.7, k, p, seed=5, mode="one-finite")
            assert tok[:, 0].tolist() == pos and bool((lp.abs() <= LOGP_TOL).all())
    # all logits equal: -log V at any temperature
    x = torch.full((64, V), -2.5, dtype=torch.bfloat16, device=DEV)
    for k, p in ((0, 1.0), (5, 1.0), (0, 0.5)):
        _, lp = check_tempered(x, 0.7, k, p, mode="equal")
        assert bool(((lp.double() + math.log(V)).abs() <= LOGP_TOL).all())
    # greedy / temperature <= 0: no draw temperature, sample_tokens_logp's bits
    x = S.grid_logits("dense", V, torch.bfloat16).to(DEV)
    rng = torch.tensor([7, 0], dtype=torch.long, device=DEV)
    for T, greedy in ((0.7, True), (0.0, False)):
        a = decode.sample_tokens_logp_tempered(x, T, 0, 1.0, greedy, rng)
        b = decode.sample_tokens_logp(x, T, 0, 1.0, greedy, rng)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# =================================================================================== generate
def _gen_kw(**kw):
    return dict(eos_token_id=-1, return_mask=True, **{**RL.GEN, **kw})


@pytest.mark.parametrize("G,group_attention", [(1, False), (4, False), (4, True)],
                         ids=["rows", "group4", "group4-attention"])
def test_generate_tempered_logprobs(G, group_attention):
    """logprob_temperature = temperature = 0.7 on tiny-llama-d128: eager and graph bitwise equal,
    the tokens of the call without log-probs, log-probs that are not the temperature-1 ones."""
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = RL.model_of(1024)
    ids, am = RL.prompts(1024)
    assert RL.GEN["temperature"] == 0.7
    kw = _gen_kw(num_return_sequences=G, group_attention=group_attention)
    base = generate(m, ids, am, use_graph=False, **kw)
    a = generate(m, ids, am, use_graph=False, return_logprobs=True, logprob_temperature=0.7, **kw)
    b = generate(m, ids, am, use_graph=True, return_logprobs=True, logprob_temperature=0.7, **kw)
    assert a[2].shape == (RL.B * G, RL.NEW) and bool((a[2] < 0).all())
    assert torch.equal(a[0], base[0]) and torch.equal(a[1], base[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    one = generate(m, ids, am, use_graph=False, return_logprobs=True, **kw)
    assert torch.equal(one[0], a[0]) and not torch.equal(one[2], a[2])
    with pytest.raises(ValueError, match="logprob_temperature"):
        generate(m, ids, am, return_logprobs=True, logprob_temperature=0.9, **kw)
    gen.clear_graph_cache()


def test_graph_of_the_unit_temperature_sampler_is_not_replayed():
    from distributed_llm_alignment_amd import ops as pops
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = RL.model_of(1024)
    ids, am = RL.prompts(1024)
    kw = _gen_kw()
    a = generate(m, ids, am, use_graph=True, return_logprobs=True, **kw)
    first = gen._GRAPH_SLOT[id(m)][3]
    assert first.graph is not None and first.logp_op is pops.decode.sample_tokens_logp
    b = generate(m, ids, am, use_graph=True, return_logprobs=True, logprob_temperature=0.7, **kw)
    second = gen._GRAPH_SLOT[id(m)][3]
    assert second is not first and second.graph is not None and second.graph is not first.graph
    assert second.logp_op is pops.decode.sample_tokens_logp_tempered
    assert torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])
    c = generate(m, ids, am, use_graph=True, return_logprobs=True, logprob_temperature=0.7, **kw)
    assert gen._GRAPH_SLOT[id(m)][3] is second  # the same call again replays it
    assert torch.equal(c[2].view(torch.int32), b[2].view(torch.int32))
    d = generate(m, ids, am, use_graph=True, return_logprobs=True, **kw)
    assert gen._GRAPH_SLOT[id(m)][3] is not second
    assert torch.equal(d[2].view(torch.int32), a[2].view(torch.int32))
    gen.clear_graph_cache()


# ======================================================================== engine against trainer
def test_tempered_rollout_grid_against_token_logprobs():
    """The same rollouts scored twice: gap_1 = max |grid - token_logprobs| at temperature 1 (the
    existing pair, code this change does not touch) and gap_tau for the tempered pair. Both sides
    scale the same bf16 logit differences by 1 / tau, so gap_tau <= 4 * gap_1 / tau, 4 being the
    margin test_rollout_logprobs_gpu.py gives its own measured gap."""
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen
    from distributed_llm_alignment_amd.objectives import action_mask, rollout_logp_grid

    gen.clear_graph_cache()
    m = RL.model_of(1024)
    tau = RL.GEN["temperature"]
    for seed in (0, 1, 2):
        ids, am = RL.prompts(1024, seed=20 + seed)
        kw = _gen_kw(seed=seed)
        seqs, mask, lp1 = generate(m, ids, am, return_logprobs=True, **kw)
        seqs2, mask2, lpt = generate(m, ids, am, return_logprobs=True, logprob_temperature=tau, **kw)
        assert torch.equal(seqs, seqs2) and torch.equal(mask, mask2)
        act = action_mask(mask, RL.TP)
        T = seqs.shape[1]
        with torch.no_grad():
            own1 = m.token_logprobs(seqs, mask)
            ownt = m.token_logprobs(seqs, mask, temperature=tau)
        gap_1 = float(((rollout_logp_grid(lp1, RL.TP, T) - own1) * act).abs().max())
        gap_tau = float(((rollout_logp_grid(lpt, RL.TP, T) - ownt) * act).abs().max())
        print(f"FIG rollout-vs-trainer seed={seed} gap_1={gap_1:.4e} gap_tau={gap_tau:.4e} "
              f"bound={4 * gap_1 / tau:.4e}")
        assert gap_tau <= 4 * gap_1 / tau, (gap_tau, gap_1)
    gen.clear_graph_cache()
