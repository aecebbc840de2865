"""MI355X: the kept-set ("keep sampling mask") kernels. The LM-head row kernels read a packed mask
next to the logits (`logprob_*_keep`, the MASK instantiations of csrc/logprob.hip); the fused sampler
writes that mask and the log-prob under the filtered draw distribution (`sample_tokens_keep`, the
KEEP instantiations of csrc/sampling.hip).

Row kernels: bit for bit the `*_temp` ops on a copy of the logits with the dropped entries at -inf,
and within the `_refs64` bound (MARGIN * E32 + FLOOR_ULPS ulp32 + one bf16 ulp on bf16 outputs, no
`extra`) of the fp64 formulas of _refs64_keep. Sampler: the tokens of `sample_tokens` bit for bit,
the mask between the oracle's K_min and K_max, logp within LOGP_TOL = 2^-14 of
z_t - log sum_{mask} exp z in fp64 with the kernel's own mask (the derivation of
test_rollout_logprobs_gpu.py covers the kept-mass sum: the same chains with fewer terms)."""
import functools
import math

import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext

import _refs64 as R
import _refs64_keep as RK
import _refs64_temp as RT
import _sampler_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LOGP_TOL = 2.0 ** -14  # tests/test_rollout_logprobs_gpu.py
ROW_KINDS = [64, 2048, 50264, "sliced"]
TAUS = RT.TEMPS + [1.0]


@pytest.fixture(scope="module", autouse=True)
def _native():
    _ext.require()
    yield
    from distributed_llm_alignment_amd.models.generation import clear_graph_cache

    clear_graph_cache()


def _dev_view(kind, x):
    """x on the device; `sliced`: as a 2048-column view of a 2112-stride buffer."""
    if kind == "sliced":
        big = torch.zeros(x.shape[0], 2112, dtype=torch.bfloat16)
        big[:, 8:2056] = x
        xd = big.to(DEV)[:, 8:2056]
        assert xd.stride(0) == 2112
        return xd
    return x.to(DEV)


@functools.lru_cache(maxsize=None)
def _row_case(kind, pattern):
    x = R.rows_case(kind).clone()
    mask, kr, kept, tgt = RK.case(pattern, x)
    return x, mask, kr, kept, tgt


# ------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("pattern", RK.PATTERNS)
@pytest.mark.parametrize("kind", ROW_KINDS)
def test_keep_rows(kind, pattern, tau):
    k = _ext.require()
    it = RT.inv32(tau)
    x, mask, kr, kept, tgt = _row_case(kind, pattern)
    N, V = x.shape
    assert kr.tolist() != list(range(N)) and int((kr < 0).sum()) == 1 and kr[N - 2] == kr[0]
    xd, xm = _dev_view(kind, x), _dev_view(kind, RK.masked(x, kept))  # the twin's input: -inf written
    td, krd = tgt.to(DEV), kr.to(DEV)
    keep = RK.pack(mask).to(DEV)
    assert torch.equal(ops.logprob.pack_keep(mask), RK.pack(mask))

    # forward: the twin's bits, twice the same, and the fp64 bound
    lp, lse = k.logprob_fwd_keep(xd, td, keep, krd, it)
    lp2, lse2 = k.logprob_fwd_keep(xd, td, keep, krd, it)
    assert torch.equal(lp, lp2) and torch.equal(lse, lse2)
    lpt, lset = k.logprob_fwd_temp(xm, td, it)
    assert torch.equal(lse, lset), (lse - lset).abs().max().item()
    assert torch.equal(lp, lpt)
    if tau == 1.0:
        lpp, lsep = k.logprob_fwd(xm, td)
        assert torch.equal(lse, lsep) and torch.equal(lp, lpp)
    ref, cpu = RK.rows64(x, tgt, it, kept), RK.rows32(x, tgt, it, kept)
    assert torch.isfinite(ref["lse"]).all()
    R.check(f"logprob_fwd_keep {pattern} tau={tau}", "lse", lse, ref["lse"], R.e32_of(cpu["lse"], ref["lse"]))
    R.check(f"logprob_fwd_keep {pattern} tau={tau}", "logp", lp, ref["logp"], R.e32_of(cpu["logp"], ref["logp"]))
    assert lp[3].item() == 0  # the ignored row
    if pattern != "ones":
        assert lp[5].item() == R.NINF  # a target outside its kept set
    if pattern == "one":
        live = [r for r in range(N) if r not in (3, 5, N - 1)]
        assert (lp[live] == 0).all(), lp.tolist()  # a one-entry set: logp exactly 0

    # backward, fed the fp64 lse rounded to fp32
    g = torch.randn(N, generator=R.gen(5))
    gd, lse_d = g.to(DEV), ref["lse"].float().to(DEV)
    a, b, c = xd.clone(), xd.clone(), xm.clone()
    k.logprob_bwd_keep(a, td, lse_d, gd, keep, krd, it)
    k.logprob_bwd_keep(b, td, lse_d, gd, keep, krd, it)
    k.logprob_bwd_temp(c, td, lse_d, gd, it)
    assert torch.equal(a, b) and torch.equal(a, c)
    if tau == 1.0:
        c = xm.clone()
        k.logprob_bwd(c, td, lse_d, gd)
        assert torch.equal(a, c)
    want = RK.bwd64(x, tgt, g, it, kept)
    R.check(f"logprob_bwd_keep {pattern} tau={tau}", "dlogits", a, want,
            R.e32_of(RK.bwd32(x, tgt, g, it, kept), want), bf16=True)
    ac = a.cpu()
    assert (ac[~kept] == 0).all(), "dropped entries must receive exact 0"
    assert (ac[3] == 0).all()  # ignored row
    if kind == "sliced":  # in place on the strided view; the columns outside stay untouched
        big = torch.zeros(N, 2112, dtype=torch.bfloat16, device=DEV)
        big[:, 8:2056] = xd
        big[:, :8] = 7.0
        big[:, 2056:] = 7.0
        k.logprob_bwd_keep(big[:, 8:2056], td, lse_d, gd, keep, krd, it)
        assert torch.equal(big[:, 8:2056], a)
        assert (big[:, :8] == 7.0).all() and (big[:, 2056:] == 7.0).all()


@pytest.mark.parametrize("tau", [0.7, 1.0])
@pytest.mark.parametrize("pattern", RK.PATTERNS)
@pytest.mark.parametrize("N", [16, 72])
def test_keep_bwd_t(N, pattern, tau):
    """The transposing kernel gives `logprob_bwd_keep`'s bits in place and their exact transpose."""
    k = _ext.require()
    it = RT.inv32(tau)
    V = 2048
    x = R.rows_case(V, N=N, seed=4)
    mask, kr, kept, tgt = RK.case(pattern, x)
    lse = RK.rows64(x, tgt, it, kept)["lse"].float().to(DEV)
    g = torch.randn(N, generator=R.gen(5)).to(DEV)
    td, krd, keep = tgt.to(DEV), kr.to(DEV), RK.pack(mask).to(DEV)
    a, b = x.to(DEV), x.to(DEV)
    k.logprob_bwd_keep(a, td, lse, g, keep, krd, it)
    bt = k.logprob_bwd_t_keep(b, td, lse, g, keep, krd, it)
    assert bt.shape == (V, N)
    assert torch.equal(a, b) and torch.equal(bt, a.t())
    assert (b.cpu()[~kept] == 0).all()


def test_keep_bwd_t_outside_its_shapes_and_host_checks():
    k = _ext.require()
    x = R.rows_case(2048)  # 9 rows: not a multiple of 8
    mask, kr, kept, tgt = RK.case("half", x)
    N, V = x.shape
    it = RT.inv32(0.7)
    lse = RK.rows64(x, tgt, it, kept)["lse"].float().to(DEV)
    g = torch.randn(N, generator=R.gen(5)).to(DEV)
    td, krd, keep = tgt.to(DEV), kr.to(DEV), RK.pack(mask).to(DEV)
    b = x.to(DEV)
    assert k.logprob_bwd_t_keep(b, td, lse, g, keep, krd, it).numel() == 0
    assert torch.equal(b, x.to(DEV))  # nothing written
    bad = [
        (x.to(DEV)[:, :1004].contiguous(), keep[:, :125].contiguous(), krd, it),  # V % 8 != 0
        (x.to(DEV), keep[:, :-1].contiguous(), krd, it),                          # keep.size(1) * 8 != V
        (x.to(DEV), keep.to(torch.int8), krd, it),                                # not uint8
        (x.to(DEV), keep.t().contiguous().t(), krd, it),                          # not contiguous
        (x.to(DEV), keep, krd[:-1], it),                                          # keep_rows not [N]
        (x.to(DEV), keep, krd.int(), it),                                         # keep_rows not int64
        (x.to(DEV), keep, krd, 0.0), (x.to(DEV), keep, krd, float("nan")),        # inv_temp
    ]
    for lg, kp, rows, inv in bad:
        with pytest.raises(RuntimeError):
            k.logprob_fwd_keep(lg, td, kp, rows, inv)


# ------------------------------------------------------------------------------ autograd wrapper
@pytest.mark.parametrize("main_grad", [False, True])
def test_linear_logprob_keep(main_grad):
    """`ops.linear_logprob(keep=)` on [64, 128] x [2048, 128] against the fp64 formula on the
    bf16-rounded logits, to the bounds test_logprob_temperature_gpu.py gives the tempered wrapper
    (2e-2 on the values, 3e-2 rel-L2 on the gradients). With a main_grad on the weight the backward
    runs the transposing kernel, without one the in-place kernel; the no-grad path is chunked."""
    N, H, V, tau = 64, 128, 2048, 0.7
    gn = R.gen(91)
    h0 = (torch.randn(N, H, generator=gn) * 0.5).bfloat16()
    W0 = (torch.randn(V, H, generator=gn) * 0.2).bfloat16()
    z = (h0.float() @ W0.float().t()).bfloat16()
    mask, kr, kept, tgt = RK.case("top37", z)
    g = torch.randn(N, generator=gn)
    it = RT.inv32(tau)
    hr, Wr = R.d(h0).requires_grad_(True), R.d(W0).requires_grad_(True)
    zz = hr @ Wr.t()
    zz = zz + (zz.detach().to(torch.bfloat16).double() - zz.detach())
    y = (zz * it).masked_fill(~kept, R.NINF)
    lp64 = torch.log_softmax(y, -1).gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    lp64 = torch.where(tgt >= 0, lp64, torch.zeros_like(lp64))
    fin = torch.isfinite(lp64)
    dh64, dW64 = torch.autograd.grad((lp64[fin] * R.d(g)[fin]).sum(), (hr, Wr))

    h = h0.to(DEV).requires_grad_(True)
    W = torch.nn.Parameter(W0.to(DEV))
    if main_grad:
        W.main_grad = torch.zeros(V, H, dtype=torch.float32, device=DEV)
    keep = ops.logprob.pack_keep(mask.to(DEV))
    lp = ops.linear_logprob(h, W, tgt.to(DEV), temperature=tau, keep=keep, keep_rows=kr.to(DEV))
    assert torch.equal(torch.isfinite(lp).cpu(), fin)
    assert (lp.cpu().double() - lp64)[fin].abs().max().item() <= 2e-2
    gd = torch.where(fin, g, torch.zeros_like(g)).to(DEV)
    (lp.masked_fill(~fin.to(DEV), 0.0) * gd).sum().backward()
    dW = W.main_grad if main_grad else W.grad
    assert RT.rel_l2(h.grad, dh64) <= 3e-2 and RT.rel_l2(dW, dW64) <= 3e-2
    with torch.no_grad():  # the chunked no-grad path gives the same values
        lp_ng = ops.linear_logprob(h.detach(), W.detach(), tgt.to(DEV), temperature=tau, keep=keep,
                                   keep_rows=kr.to(DEV))
    assert torch.equal(lp_ng, lp.detach())


# ------------------------------------------------------------------------------------ sampler
SAMPLER_V = (32760, 32768, 128256)
SAMPLER_MODES = [m for m in S.MODES if m[0] == "peaked"] + [("dense", 50, 1.0)]
T_DRAW = 0.7


@functools.lru_cache(maxsize=2)
def _grid(builder, V, dtype):
    return S.grid_logits(builder, V, dtype).to(DEV)


def _check_sampler(x, mode, counters=S.COUNTERS, seed=7):
    from distributed_llm_alignment_amd.ops import decode

    builder, top_k, top_p = mode
    B, V = x.shape
    kept = S.kept_sets(x, T_DRAW, top_k, top_p)
    z = kept.z
    assert float(kept.ambiguous.double().mean()) <= S.AMBIGUOUS_CAP
    worst = 0.0
    for c in counters:
        rng = torch.tensor([seed, c], dtype=torch.long, device=DEV)
        plain = decode.sample_tokens(x, T_DRAW, top_k, top_p, False, rng)
        tok, lp, keep = decode.sample_tokens_keep(x, T_DRAW, top_k, top_p, False, rng)
        tok2, lp2, keep2 = decode.sample_tokens_keep(x, T_DRAW, top_k, top_p, False, rng)
        assert keep.dtype == torch.uint8 and keep.shape == (B, V // 8) and lp.dtype == torch.float32
        assert torch.equal(tok, plain), "tokens differ from sample_tokens"
        assert torch.equal(tok, tok2) and torch.equal(keep, keep2)
        assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)), "two launches gave different bits"
        m = ops.logprob.unpack_keep(keep)
        amb = kept.ambiguous
        assert torch.equal(m[~amb], kept.kmin[~amb]), "unambiguous rows: the mask is the exact kept set"
        assert not bool((kept.kmin & ~m).any()) and not bool((m & ~kept.kmax).any())
        assert bool(m.gather(1, tok.unsqueeze(1)).all()), "a token outside its own mask"
        mass = torch.where(m, z.exp(), torch.zeros_like(z)).sum(-1)
        want = z.gather(1, tok.unsqueeze(1)).squeeze(1) - mass.log()
        worst = max(worst, float((lp.double() - want).abs().max()))
    print(f"LOGP_STAT keep dtype={x.dtype} mode={S.mode_id(mode)} T={T_DRAW} V={V} rows={B} "
          f"draws={len(counters) * B} worst_err={worst:.3e} tol={LOGP_TOL:.3e}")
    assert worst <= LOGP_TOL, worst
    return tok, lp, keep


@pytest.mark.parametrize("mode", SAMPLER_MODES, ids=S.mode_id)
@pytest.mark.parametrize("V", SAMPLER_V)
def test_sampler_keep(V, mode):
    """V = 32760: the single-block kernel; 32768 and 128256: the row-split path."""
    _check_sampler(_grid(mode[0], V, torch.bfloat16), mode)


def test_sampler_keep_fp32_logits():
    _check_sampler(_grid("peaked", 32768, torch.float32), ("peaked", 0, 0.9))


@pytest.mark.parametrize("V", [4096, 32768], ids=["single-block", "split"])
def test_sampler_keep_edges(V):
    """A NaN logit is never kept; without a filter the mask is the z >= -64 window; a row without a
    finite max writes logp 0 and an all-ones mask row."""
    from distributed_llm_alignment_amd.ops import decode

    x = S.peaked(8, V, 31)
    g = torch.Generator().manual_seed(31)
    nan = torch.rand(8, V, generator=g) < 0.1
    nan[:, 0] = True
    x[nan] = float("nan")
    x[6] = float("-inf")
    x[7, 5] = float("inf")
    x = x.bfloat16().to(DEV)
    rng = torch.tensor([3, 0], dtype=torch.long, device=DEV)
    for top_k, top_p in ((0, 1.0), (0, 0.9), (20, 1.0)):
        tok, lp, keep = decode.sample_tokens_keep(x, T_DRAW, top_k, top_p, False, rng)
        assert torch.equal(tok, decode.sample_tokens(x, T_DRAW, top_k, top_p, False, rng))
        m = ops.logprob.unpack_keep(keep)
        assert not bool((m[:6] & nan[:6].to(DEV)).any()), "a NaN logit was kept"
        assert bool(m[6:].all()) and lp[6:].tolist() == [0.0, 0.0]
        assert bool(m[:6].gather(1, tok[:6].unsqueeze(1)).all())
        if top_k == 0 and top_p == 1.0:
            assert torch.equal(m[:6], (S.z_scores(x[:6], T_DRAW) >= -S.RANGE))


def test_sampler_keep_rejections():
    from distributed_llm_alignment_amd.ops import decode

    k = _ext.require()
    rng = torch.tensor([3, 0], dtype=torch.long, device=DEV)
    x = S.dense(2, 4099, 1).bfloat16().to(DEV)
    with pytest.raises(ValueError):
        decode.sample_tokens_keep(x, 0.7, 0, 0.9, False, rng)
    with pytest.raises(RuntimeError, match="V % 8"):
        k.sample_tokens_keep(x, 0.7, 0, 0.9, rng)
    y = S.dense(2, 4096, 1).bfloat16().to(DEV)
    with pytest.raises(ValueError):
        decode.sample_tokens_keep(y, 0.7, 0, 0.9, True, rng)  # greedy
    with pytest.raises(RuntimeError, match="temperature"):
        k.sample_tokens_keep(y, 0.0, 0, 0.9, rng)
    big = torch.zeros(2, 4104, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="aligned"):
        k.sample_tokens_keep(big[:, 1:4097], 0.7, 0, 0.9, rng)
    with pytest.raises(RuntimeError, match="stride"):
        k.sample_tokens_keep(torch.zeros(2, 4100, dtype=torch.bfloat16, device=DEV)[:, :4096], 0.7, 0, 0.9, rng)


@pytest.mark.parametrize("V", SAMPLER_V)
def test_sampler_and_lm_head_share_one_action_space(V):
    """The LM-head kernel over the sampler's own mask gives the sampler's log-prob: both sides on K."""
    from distributed_llm_alignment_amd.ops import decode

    k = _ext.require()
    x = _grid("peaked", V, torch.bfloat16)
    rng = torch.tensor([7, 0], dtype=torch.long, device=DEV)
    tok, lp, keep = decode.sample_tokens_keep(x, T_DRAW, 0, 0.9, False, rng)
    rows = torch.arange(x.shape[0], device=DEV)
    head, _ = k.logprob_fwd_keep(x, tok, keep, rows, RT.inv32(T_DRAW))
    err = float((head.double() - lp.double()).abs().max())
    print(f"LOGP_STAT keep sampler-vs-head V={V} worst_err={err:.3e} tol={2 * LOGP_TOL:.3e}")
    assert err <= 2 * LOGP_TOL


# ----------------------------------------------------------------------------------- generation
B, TP, NEW = 3, 20, 24
GEN = dict(max_new_tokens=NEW, do_sample=True, top_p=0.9, temperature=0.7, seed=11)


@functools.lru_cache(maxsize=2)
def model_of(vocab):
    import dataclasses

    from distributed_llm_alignment_amd.models import build_model, get_config

    cfg = get_config("tiny-llama-d128")
    if vocab != cfg.vocab_size:
        cfg = dataclasses.replace(cfg, vocab_size=vocab)
    return build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0).eval()


def prompts(vocab, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ids = torch.randint(3, vocab, (B, TP), device=DEV, generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0  # left padding
    ids[1, :5] = 0
    return ids, am


def check_generation(m, vocab, monkeypatch, G=1):
    """Eager generate with `ops.decode.sample_tokens_keep` wrapped to keep the logits it was given:
    masks and logp are a replay of the op on those logits; the captured graph gives the same bits."""
    from distributed_llm_alignment_amd.models import generate

    ids, am = prompts(vocab)
    free = generate(m, ids, am, eos_token_id=-1, use_graph=False, num_return_sequences=G, **GEN)[:, TP:]
    eos = next(t for t in free[:, 2:NEW // 2].flatten().tolist()
               if bool((free == t).any(1).any()) and not bool((free == t).any(1).all()))
    seen, real = [], ops.decode.sample_tokens_keep

    def spy(logits, *a, **k):
        seen.append((logits.detach().clone(), a[4].clone()))
        return real(logits, *a, **k)

    kw = dict(eos_token_id=eos, pad_token_id=0, return_mask=True, return_logprobs=True, logprob_temperature=0.7,
              return_keep_mask=True, num_return_sequences=G, **GEN)
    with monkeypatch.context() as mp:
        mp.setattr(ops.decode, "sample_tokens_keep", spy)
        seqs, mask, logp, keep = generate(m, ids, am, use_graph=False, **kw)
    n = seqs.shape[1] - TP
    assert keep.shape == (B * G, n, vocab // 8) and keep.dtype == torch.uint8 and logp.shape == (B * G, n)
    assert len(seen) == n
    gm = mask[:, TP:]
    assert 0 < int((gm == 0).sum()) < gm.numel(), "want finished and running rows"
    assert torch.equal(logp[gm == 0], torch.zeros_like(logp[gm == 0]))
    for j, (lg, rng) in enumerate(seen):
        tok, lp, kp = real(lg, 0.7, 0, 0.9, False, rng)
        live = gm[:, j] == 1
        assert torch.equal(tok[live], seqs[live, TP + j])
        assert torch.equal(kp, keep[:, j])  # finished rows too: whatever the sampler wrote
        assert torch.equal(lp[live].view(torch.int32), logp[live, j].view(torch.int32))
        assert bool(ops.logprob.unpack_keep(kp)[live].gather(1, tok[live].unsqueeze(1)).all())
    gs, gmask, glp, gkeep = generate(m, ids, am, use_graph=True, **kw)
    assert torch.equal(gs, seqs) and torch.equal(gmask, mask) and torch.equal(gkeep, keep)
    assert torch.equal(glp.view(torch.int32), logp.view(torch.int32))


@pytest.mark.parametrize("vocab", [1024, 65536], ids=["single-block", "split"])
def test_generate_keep_mask_is_the_samplers(vocab, monkeypatch):
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(vocab)
    check_generation(m, vocab, monkeypatch)
    assert gen._GRAPH_SLOT[id(m)][3].keep is not None
    gen.clear_graph_cache()


def test_group_rollouts_return_keep_mask(monkeypatch):
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    check_generation(model_of(1024), 1024, monkeypatch, G=4)
    gen.clear_graph_cache()


def test_graph_without_the_mask_is_not_replayed_for_a_call_with_it():
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(1024)
    ids, am = prompts(1024)
    kw = dict(eos_token_id=-1, return_mask=True, use_graph=True, **GEN)
    a_seqs, _ = generate(m, ids, am, **kw)
    first = gen._GRAPH_SLOT[id(m)][3]
    assert first.graph is not None and first.keep is None
    b_seqs, _, b_keep = generate(m, ids, am, return_keep_mask=True, **kw)
    second = gen._GRAPH_SLOT[id(m)][3]
    assert second is not first and second.graph is not first.graph and second.keep is not None
    assert torch.equal(b_seqs, a_seqs)  # the KEEP kernels: the same tokens
    # the tempered log-prob graph is a third one: another sampler op
    generate(m, ids, am, return_logprobs=True, logprob_temperature=0.7, **kw)
    third = gen._GRAPH_SLOT[id(m)][3]
    assert third is not second and third.keep is None and third.logp is not None
    c_seqs, _, c_lp, c_keep = generate(m, ids, am, return_logprobs=True, logprob_temperature=0.7,
                                       return_keep_mask=True, **kw)
    assert gen._GRAPH_SLOT[id(m)][3] is not third
    assert torch.equal(c_seqs, a_seqs) and torch.equal(c_keep, b_keep) and bool((c_lp < 0).all())
    gen.clear_graph_cache()


# -------------------------------------------------------------------------------------- trainer
def _rollouts(pol, G):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.objectives import action_mask, keep_row_grid, rollout_logp_grid

    Tp, n, P = 16, 16, 2
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, pol.cfg.vocab_size, (P, Tp), generator=g).to(DEV)
    seqs, mask, logp, keep = generate(pol, ids, torch.ones_like(ids), max_new_tokens=n, do_sample=True,
                                      temperature=0.7, top_p=0.9, eos_token_id=-1, seed=5, return_mask=True,
                                      return_logprobs=True, logprob_temperature=0.7, return_keep_mask=True,
                                      num_return_sequences=G)
    pol.train()
    scores = torch.randn(P * G, generator=g).to(DEV)
    rows = keep_row_grid(action_mask(mask, Tp), Tp, keep.shape[1])
    return seqs, mask, scores, Tp, n, rollout_logp_grid(logp, Tp, seqs.shape[1]), keep, rows


def _finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values() if isinstance(v, torch.Tensor))


def test_grpo_step_with_the_sampling_mask():
    """generate(return_keep_mask) -> grpo_rollout_stats(rollout_logp=, keep=) -> grpo_loss(keep=) with
    `correct`'s importance weights: finite, the weights near 1 (both sides on the kept set), and the
    loss is `ops.grpo_loss` on `token_logprobs(keep=)`. Without the mask the same calls give the
    loss of `ops.grpo_loss` on the plain tempered `token_logprobs`: the parent formula."""
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.objectives import (grpo_loss, grpo_rollout_stats, keep_fraction,
                                                          rollout_mismatch)
    from distributed_llm_alignment_amd.parallel.data_parallel import DataParallelEngine

    cfg = get_config("tiny-llama-d128", num_layers=2)
    pol = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    eng = DataParallelEngine(pol, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01, max_grad_norm=1.0)
    ref = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=1).requires_grad_(False).eval()
    G = 4
    seqs, mask, scores, Tp, n, rlp, keep, rows = _rollouts(pol, G)
    kw = dict(is_cap=2.0, is_floor=None, is_level="token", is_mode="truncate", temperature=0.7)
    stats = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, G, beta=0.04, rollout_logp=rlp, keep=keep,
                               keep_rows=rows, **kw)
    act = stats["act"]
    assert torch.equal(stats["keep_rows"], rows) and _finite(stats) and _finite(stats["rollout_is"])
    mism = rollout_mismatch(rlp, stats["old_logp"], act)
    with torch.no_grad():
        full = pol.token_logprobs(seqs, mask, temperature=0.7)
    frac = keep_fraction(full, stats["old_logp"], act).item()
    print(f"KEEP_STAT gpu grpo rollout_kl={mism['rollout_kl'].item():.3e} "
          f"absdiff_max={mism['rollout_logp_absdiff_max'].item():.3e} keep_fraction={frac:.4f} "
          + " ".join(f"{k}={v.item():.4e}" for k, v in stats["rollout_is"].items()))
    assert math.isfinite(mism["rollout_kl"].item()) and 0.85 <= frac <= 1.0
    assert abs(stats["rollout_is"]["rollout_is_mean"].item() - 1.0) < 0.1
    loss, m = grpo_loss(pol, seqs, mask, stats, 0.2, 0.28, 0.04, "token", n, temperature=0.7, keep=keep)
    with torch.no_grad():
        lp = pol.token_logprobs(seqs, mask, temperature=0.7, keep=keep.reshape(-1, keep.shape[-1]), keep_rows=rows)
        want, _ = ops.grpo_loss(lp, stats["old_logp"], stats["ref_logp"], stats["advantages"], act, 0.2, 0.28,
                                0.04, "token", n, None, is_weight=stats["is_weight"])
    assert torch.equal(loss.detach(), want) and _finite(m)
    loss.backward()
    assert bool(torch.isfinite(eng.grad_buf).all()) and float(eng.grad_buf.float().abs().sum()) > 0
    # the key off: today's calls
    off = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, G, beta=0.04, need_old=True, temperature=0.7)
    assert "keep_rows" not in off
    loss0, _ = grpo_loss(pol, seqs, mask, off, 0.2, 0.28, 0.04, "token", n, temperature=0.7)
    with torch.no_grad():
        want0, _ = ops.grpo_loss(full, off["old_logp"], off["ref_logp"], off["advantages"], act, 0.2, 0.28, 0.04,
                                 "token", n, None)
    assert torch.equal(loss0.detach(), want0) and torch.equal(off["old_logp"], full)


def test_ppo_step_with_the_sampling_mask():
    from distributed_llm_alignment_amd.models import build_model, build_value_model, get_config
    from distributed_llm_alignment_amd.objectives import ppo_backward, ppo_loss, ppo_rollout_stats, rollout_mismatch

    cfg = get_config("tiny-llama-d128", num_layers=2)
    pol = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    ref = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=1).requires_grad_(False).eval()
    critic, _ = build_value_model("tiny-llama-d128", device=DEV, seed=2)
    seqs, mask, scores, Tp, n, rlp, keep, rows = _rollouts(pol, 1)
    kw = dict(is_cap=2.0, is_floor=None, is_level="token", is_mode="truncate", temperature=0.7)
    stats = ppo_rollout_stats(pol, ref, critic, seqs, mask, Tp, scores, rollout_logp=rlp, keep=keep, keep_rows=rows,
                              **kw)
    assert torch.equal(stats["keep_rows"], rows) and _finite(stats) and _finite(stats["rollout_is"])
    mism = rollout_mismatch(rlp, stats["old_logp"], stats["act"])
    print(f"KEEP_STAT gpu ppo rollout_kl={mism['rollout_kl'].item():.3e} "
          f"absdiff_max={mism['rollout_logp_absdiff_max'].item():.3e}")
    assert math.isfinite(mism["rollout_kl"].item())
    loss, m = ppo_loss(pol, critic, seqs, mask, stats, temperature=0.7, keep=keep)
    ppo_backward(loss)
    assert bool(torch.isfinite(loss)) and _finite(m)
    # on-policy and on one action space: the ratio is 1 to rounding
    assert m["approx_kl"].abs().item() < 1e-3
    with pytest.raises(ValueError, match="entropy"):
        ppo_loss(pol, critic, seqs, mask, stats, entropy_coef=0.01, temperature=0.7, keep=keep)
    # the key off: the parent formula on the plain tempered log-probs
    off = ppo_rollout_stats(pol, ref, critic, seqs, mask, Tp, scores, temperature=0.7)
    assert "keep_rows" not in off
    with torch.no_grad():
        assert torch.equal(off["old_logp"], pol.token_logprobs(seqs, mask, temperature=0.7))
        lp = pol.token_logprobs(seqs, mask, temperature=0.7)
        want, _ = ops.ppo_policy_loss(lp, off["old_logp"], off["advantages"], off["act"], 0.2)
    loss0, m0 = ppo_loss(pol, critic, seqs, mask, off, temperature=0.7)
    assert torch.equal(m0["policy_loss"], want)
