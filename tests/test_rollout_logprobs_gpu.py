"""MI355X: the fused sampler's `logp` output (`torch.ops.dla.sample_tokens_logp`, csrc/sampling.hip
LOGP instantiations: single block scalar / vectorised, row split) against fp64, and its way through
`generate(return_logprobs=True)` (eager, captured graph, group rollouts) to the trainer's action
grid.

logp[r] = log softmax(x_r)[token_r] at temperature 1 over the full vocabulary, NaN logits counted
as -inf. Every case checks three things: the tokens are bitwise those of `sample_tokens`, the same
launch twice gives the same bits, and every row is within LOGP_TOL = 2^-14 of the fp64 value. The
bound is derived, not measured: an fp32 mass sum is within 2^-15 relative (the accounting of
_sampler_ref.py: chains of <= 128 adds per thread, 10 reduction levels, 32 chunk adds, __expf),
which is at most 2^-15 absolute after the log; the fp32 rounding of x_t - max adds
2^-24 * |x_t - max| <= 2^-24 * 64 * T <= 5e-6 for a drawn token at T <= 1.3; the fp32 log of a
value in [1, V] adds under 3e-6; together below 2^-14.6. Each check prints `LOGP_STAT` with the
worst error it saw before it asserts."""
import dataclasses
import functools
import math
import os

import pytest
import torch

import _sampler_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SPLIT_ON = os.environ.get("DLA_SAMPLER_SPLIT", "1")[:1] != "0"
LOGP_TOL = 2.0 ** -14
INF = float("inf")
COUNTERS = (0, 1, 2)
# (name, builder, top_k, top_p, greedy)
MODES = (("plain", "dense", 0, 1.0, False), ("k50", "dense", 50, 1.0, False), ("p0.9", "peaked", 0, 0.9, False),
         ("k50-p0.9", "peaked", 50, 0.9, False), ("greedy", "dense", 0, 1.0, True))
TEMPS = (0.7, 1.0, 1.3)


@pytest.fixture(scope="module", autouse=True)
def _native():
    from distributed_llm_alignment_amd.ops import _ext

    _ext.require()
    yield
    from distributed_llm_alignment_amd.models.generation import clear_graph_cache

    clear_graph_cache()


def dtype_id(dtype) -> str:
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dtype]


def path_of(x: torch.Tensor, greedy: bool = False) -> str:
    V = x.shape[1]
    if not (V % 8 == 0 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0):
        return "single-scalar"
    return "split" if V >= 32768 and SPLIT_ON and not greedy else "single-vec"


def ref_logsoftmax(x: torch.Tensor) -> torch.Tensor:
    """fp64 log-softmax of the rows as the kernel reads them, NaN -> -inf. Rows whose maximum is
    not finite come out NaN: they are `undefined` below."""
    xd = x.double()
    return torch.log_softmax(torch.where(torch.isnan(xd), torch.full_like(xd, -INF), xd), -1)


def check_logp(x, T, k, p, greedy=False, seed=7, counters=COUNTERS, mode="", ref=None):
    """The three checks on logits x [B, V]; returns (tokens [B, C], logp [B, C], worst error)."""
    from distributed_llm_alignment_amd.ops import decode

    ref = ref_logsoftmax(x) if ref is None else ref
    xf = x.float()
    rowmax = torch.where(torch.isnan(xf), torch.full_like(xf, -INF), xf).max(-1).values
    defined = torch.isfinite(rowmax)
    toks, lps, worst = [], [], 0.0
    for c in counters:
        rng = torch.tensor([seed, c], dtype=torch.long, device=x.device)
        plain = decode.sample_tokens(x, T, k, p, greedy, rng)
        tok, lp = decode.sample_tokens_logp(x, T, k, p, greedy, rng)
        tok2, lp2 = decode.sample_tokens_logp(x, T, k, p, greedy, rng)
        assert tok.dtype == torch.long and lp.dtype == torch.float32 and lp.shape == tok.shape == (x.shape[0],)
        assert torch.equal(tok, plain), "tokens differ from sample_tokens"
        assert torch.equal(tok, tok2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32)), \
            "the same launch twice gave different bits"
        want = ref.gather(1, tok.unsqueeze(1)).squeeze(1)
        err = (lp.double() - want).abs()
        if bool(defined.any()):
            worst = max(worst, float(err[defined].max()))
        assert torch.equal(lp[~defined], torch.zeros_like(lp[~defined])), "undefined rows must write exactly 0.0"
        toks.append(tok)
        lps.append(lp)
    print(f"LOGP_STAT path={path_of(x, greedy)} dtype={dtype_id(x.dtype)} mode={mode} T={T} V={x.shape[1]} "
          f"rows={x.shape[0]} draws={len(counters) * x.shape[0]} worst_err={worst:.3e} tol={LOGP_TOL:.3e}")
    assert worst <= LOGP_TOL, worst
    return torch.stack(toks, 1), torch.stack(lps, 1), worst


# ------------------------------------------------------------------------------------ the grid
@functools.lru_cache(maxsize=4)
def grid_case(builder, V, dtype):
    x = S.grid_logits(builder, V, dtype).to(DEV)
    return x, ref_logsoftmax(x)


GRID = [(V, dt) for V in (4099, 4096, 32768, 32776) for dt in S.DTYPES] + [(128256, torch.bfloat16)]


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[0])
@pytest.mark.parametrize("V,dtype", GRID, ids=lambda v: dtype_id(v) if isinstance(v, torch.dtype) else str(v))
def test_kernel_logp_matches_fp64(V, dtype, mode, T):
    """64 rows x 3 counters. V: 4099 single block, scalar; 4096 single block, vectorised; 32768
    split, chunks of exactly 128 vectors; 32776 split with a short last chunk; 128256 the
    workload's vocabulary. Greedy rows take the single-block kernel's extra S1 pass at every V."""
    name, builder, k, p, greedy = mode
    x, ref = grid_case(builder, V, dtype)
    want_path = "single-scalar" if V % 8 else ("split" if V >= 32768 and SPLIT_ON and not greedy else "single-vec")
    assert path_of(x, greedy) == want_path
    tok, lp, _ = check_logp(x, T, k, p, greedy, mode=name, ref=ref)
    assert bool((lp <= 0).all()) and bool(torch.isfinite(lp).all())
    if greedy:
        assert torch.equal(tok[:, 0], x.float().argmax(-1))


# ------------------------------------------------------------------------------------ row layout
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("layout", ["strided", "misaligned"])
@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", [4096, 32768])
def test_row_layouts(V, dtype, layout, B):
    """Rows of a [B, V + 8] buffer: `[:, :V]` (aligned rows, row stride != V: vectorised / split)
    and `[:, 1:V + 1]` (misaligned: the scalar single-block kernel). A pad column that entered the
    mass sum would move logp by far more than the bound."""
    for builder, k, p, greedy in (("dense", 0, 1.0, False), ("peaked", 0, 0.9, False), ("dense", 0, 1.0, True)):
        src = {"dense": S.dense, "peaked": S.peaked}[builder](B, V, 100 + B).to(dtype)
        big = torch.full((B, V + 8), 50.0, dtype=dtype, device=DEV)
        x = big[:, :V] if layout == "strided" else big[:, 1:V + 1]
        x.copy_(src)
        assert path_of(x, greedy) == ("single-scalar" if layout == "misaligned" else
                                      "split" if V >= 32768 and SPLIT_ON and not greedy else "single-vec")
        check_logp(x, 0.9, k, p, greedy, mode=f"{layout}-{builder}-k{k}-p{p}{'-greedy' if greedy else ''}")


# ------------------------------------------------------------------------------------ edges
EDGE_V = [4096, 32768]
DRAWS = ((0, 1.0, False), (50, 1.0, False), (0, 0.9, False), (50, 0.9, False), (0, 1.0, True))


def layouts(x):
    """The same rows on each kernel the width admits: as they are, and misaligned (scalar)."""
    big = torch.zeros((x.shape[0], x.shape[1] + 8), dtype=x.dtype, device=x.device)
    mis = big[:, 1:x.shape[1] + 1]
    mis.copy_(x)
    return [x, mis]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_nan_counts_as_neg_inf(V, dtype):
    """10 % NaN and 10 % -inf per row, first and last index included: same bound, NaN as -inf."""
    g = torch.Generator().manual_seed(31)
    x = S.peaked(64, V, 31)
    r = torch.rand(64, V, generator=g)
    x[r < 0.1] = float("nan")
    x[(r >= 0.1) & (r < 0.2)] = -INF
    x[:, 0] = float("nan")
    x[:, V - 1] = -INF
    x = x.to(dtype).to(DEV)
    for y in layouts(x):
        for k, p, greedy in DRAWS:
            _, lp, _ = check_logp(y, 1.0, k, p, greedy, mode=f"nan-inf-k{k}-p{p}{'-greedy' if greedy else ''}")
            assert bool(torch.isfinite(lp).all())


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_one_finite_logit_has_logp_zero(V, dtype):
    pos = [0, 7, V - 1, 2 * 1024, 2 * 1024 + 1023, V // 2 + 3]
    x = torch.full((len(pos), V), -INF, dtype=dtype, device=DEV)
    for r, i in enumerate(pos):
        x[r, i] = -3.0
    for y in layouts(x):
        for k, p, greedy in DRAWS:
            tok, lp, _ = check_logp(y, 0.9, k, p, greedy, seed=5, mode="one-finite")
            assert tok[:, 0].tolist() == pos and bool((lp.abs() <= LOGP_TOL).all())


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_undefined_rows_write_exactly_zero(V, dtype):
    """A +inf in the row, or no finite logit at all: logp is exactly 0.0, the tokens are those of
    `sample_tokens` (first +inf index / token 0), and a finite row next to them is unaffected."""
    x = S.dense(7, V, 37)
    x[0, 7] = INF
    x[1, V - 1] = INF
    x[1, 3] = float("nan")
    x[2, 2 * 1024] = x[2, 2 * 1024 + 9] = INF
    x[3] = -INF
    x[4] = float("nan")
    x[5, ::2] = -INF
    x[5, 1::2] = float("nan")
    x = x.to(dtype).to(DEV)
    for y in layouts(x):
        for k, p, greedy in DRAWS:
            tok, lp, _ = check_logp(y, 0.9, k, p, greedy, seed=5, mode="undefined-rows")
            assert tok[:6, 0].tolist() == [7, V - 1, 2 * 1024, 0, 0, 0]
            assert torch.equal(lp[:6], torch.zeros_like(lp[:6])) and bool((lp[6] < 0).all())


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V + [4099])
def test_all_logits_equal_is_minus_log_v(V, dtype):
    x = torch.full((64, V), -2.5, dtype=dtype, device=DEV)
    for k, p, greedy in ((0, 1.0, False), (5, 1.0, False), (0, 0.5, False), (0, 1.0, True)):
        _, lp, _ = check_logp(x, 0.8, k, p, greedy, mode="equal")
        assert bool(((lp.double() + math.log(V)).abs() <= LOGP_TOL).all())


# ----------------------------------------------------------------------------------- generation
B, TP, NEW = 3, 20, 24
GEN = dict(max_new_tokens=NEW, do_sample=True, top_p=0.9, temperature=0.7, seed=11)


@functools.lru_cache(maxsize=2)
def model_of(vocab, **over):
    from distributed_llm_alignment_amd.models import build_model, get_config

    cfg = get_config("tiny-llama-d128")
    if vocab != cfg.vocab_size or over:
        cfg = dataclasses.replace(cfg, vocab_size=vocab, **over)
    return build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0).eval()


def prompts(vocab, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ids = torch.randint(3, vocab, (B, TP), device=DEV, generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0  # left padding
    ids[1, :5] = 0
    return ids, am


def an_eos_that_occurs(m, ids, am, G=1):
    """A token some row emits in the first half of an unconstrained run and some row does not:
    with it as EOS (same seed, so the same draws up to there) rows finish early."""
    from distributed_llm_alignment_amd.models import generate

    free = generate(m, ids, am, eos_token_id=-1, use_graph=False, num_return_sequences=G, **GEN)[:, TP:]
    for t in free[:, 2:NEW // 2].flatten().tolist():
        hit = (free == t).any(1)
        if bool(hit.any()) and not bool(hit.all()):
            return t
    raise AssertionError("no token splits the rows")


def eager_recorded(m, ids, am, eos, monkeypatch, G=1):
    """Eager generate with `ops.decode.sample_tokens_logp` wrapped to keep the logits it was given."""
    from distributed_llm_alignment_amd import ops
    from distributed_llm_alignment_amd.models import generate

    seen, real = [], ops.decode.sample_tokens_logp

    def spy(logits, *a, **k):
        seen.append(logits.detach().clone())
        return real(logits, *a, **k)

    with monkeypatch.context() as mp:
        mp.setattr(ops.decode, "sample_tokens_logp", spy)
        out = generate(m, ids, am, eos_token_id=eos, pad_token_id=0, use_graph=False, return_mask=True,
                       return_logprobs=True, num_return_sequences=G, **GEN)
    return out, seen


def check_generation(m, vocab, monkeypatch, G=1, tag=""):
    from distributed_llm_alignment_amd.models import generate

    ids, am = prompts(vocab)
    eos = an_eos_that_occurs(m, ids, am, G)
    (seqs, mask, logp), seen = eager_recorded(m, ids, am, eos, monkeypatch, G)
    n = seqs.shape[1] - TP
    assert seqs.shape[0] == B * G and logp.shape == (B * G, n) and logp.dtype == torch.float32 and len(seen) == n
    gm = mask[:, TP:]
    assert 0 < int((gm == 0).sum()) < gm.numel(), "want finished and running rows"
    assert torch.equal(logp[gm == 0], torch.zeros_like(logp[gm == 0]))  # exactly 0 once finished
    worst = 0.0
    for j, lg in enumerate(seen):
        want = ref_logsoftmax(lg).gather(1, seqs[:, TP + j:TP + j + 1]).squeeze(1)
        live = gm[:, j] == 1
        if bool(live.any()):
            worst = max(worst, float((logp[:, j].double() - want).abs()[live].max()))
    print(f"LOGP_STAT generate{tag} V={vocab} rows={B * G} steps={n} worst_err={worst:.3e} tol={LOGP_TOL:.3e}")
    assert worst <= LOGP_TOL, worst
    # the captured graph: bitwise the eager result
    gs, gmask, glp = generate(m, ids, am, eos_token_id=eos, pad_token_id=0, use_graph=True, return_mask=True,
                              return_logprobs=True, num_return_sequences=G, **GEN)
    assert torch.equal(gs, seqs) and torch.equal(gmask, mask)
    assert torch.equal(glp.view(torch.int32), logp.view(torch.int32))
    return ids, am, eos, seqs, mask, logp


@pytest.mark.parametrize("vocab", [1024, 65536], ids=["single-block", "split"])
def test_generate_logprobs_are_the_samplers(vocab, monkeypatch):
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(vocab)
    check_generation(m, vocab, monkeypatch)
    assert gen._GRAPH_SLOT[id(m)][3].logp is not None
    gen.clear_graph_cache()


def test_graph_without_logprobs_is_not_replayed_for_a_call_with_them(monkeypatch):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(1024)
    ids, am = prompts(1024)
    kw = dict(eos_token_id=-1, return_mask=True, **GEN)
    e_seqs, e_mask = generate(m, ids, am, use_graph=False, **kw)
    a_seqs, a_mask = generate(m, ids, am, use_graph=True, **kw)
    first = gen._GRAPH_SLOT[id(m)][3]
    assert first.graph is not None and first.logp is None
    assert torch.equal(a_seqs, e_seqs) and torch.equal(a_mask, e_mask)
    b_seqs, b_mask, b_lp = generate(m, ids, am, use_graph=True, return_logprobs=True, **kw)
    second = gen._GRAPH_SLOT[id(m)][3]
    assert second is not first and second.graph is not None and second.graph is not first.graph
    assert second.logp is not None
    assert torch.equal(b_seqs, e_seqs) and torch.equal(b_mask, e_mask)  # LOGP kernels: the same tokens
    c_seqs, c_mask, c_lp = generate(m, ids, am, use_graph=False, return_logprobs=True, **kw)
    assert torch.equal(c_seqs, e_seqs) and torch.equal(c_lp.view(torch.int32), b_lp.view(torch.int32))
    assert bool((b_lp < 0).all())
    # and back: a call without them does not replay the graph that writes them
    d_seqs, _ = generate(m, ids, am, use_graph=True, **kw)
    third = gen._GRAPH_SLOT[id(m)][3]
    assert third is not second and third.logp is None and torch.equal(d_seqs, e_seqs)
    gen.clear_graph_cache()


@pytest.mark.parametrize("group_attention", [False, True], ids=["per-row", "group-attention"])
def test_group_rollouts_return_logprobs(group_attention, monkeypatch):
    """num_return_sequences=4 on the shared prefill: [B*4, n], the same checks."""
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(1024)
    if not group_attention:
        check_generation(m, 1024, monkeypatch, G=4, tag="-group4")
    else:
        ids, am = prompts(1024)
        kw = dict(eos_token_id=-1, return_mask=True, return_logprobs=True, num_return_sequences=4,
                  group_attention=True, **GEN)
        a = generate(m, ids, am, use_graph=False, **kw)
        b = generate(m, ids, am, use_graph=True, **kw)
        assert a[2].shape == (B * 4, NEW) and bool((a[2] < 0).all())
        assert torch.equal(a[0], b[0]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    gen.clear_graph_cache()


# ------------------------------------------------------------------- against the trainer, measured
# No bound can be derived for the gap between the bf16 decode kernels (skinny GEMMs, split-KV
# attention over the cache) and the bf16 training forward: both are correct roundings of the same
# mathematics. It is measured against `token_logprobs`, whose kernels the fp64 tier pins:
# max over seeds 0, 1, 2 of |rollout grid - token_logprobs| on the action tokens, first GPU run
# (profiles/rollout_logprobs.md). The assertion allows 4x it: another draw hits other roundings.
# Measured: 7.8478e-03, 1.0304e-02, 8.1038e-03 (rollout_kl 1.4e-04 .. 2.4e-04).
MEASURED_GAP = 1.0304e-02


def _gap(m, seed, weight_dtype="bf16"):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.objectives import action_mask, rollout_logp_grid, rollout_mismatch

    ids, am = prompts(m.cfg.vocab_size, seed=20 + seed)
    seqs, mask, logp = generate(m, ids, am, eos_token_id=-1, return_mask=True, return_logprobs=True,
                                weight_dtype=weight_dtype, **{**GEN, "seed": seed})
    grid = rollout_logp_grid(logp, TP, seqs.shape[1])
    act = action_mask(mask, TP)
    with torch.no_grad():
        own = m.token_logprobs(seqs, mask)
    assert torch.equal(grid[act == 0], torch.zeros_like(grid[act == 0]))
    return float(((grid - own) * act).abs().max()), rollout_mismatch(grid, own, act)


def test_rollout_grid_against_token_logprobs():
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(1024)
    gaps, kls = zip(*[_gap(m, s) for s in (0, 1, 2)])
    print(f"LOGP_STAT rollout-vs-trainer bf16 max_abs_gap per seed={['%.4e' % g for g in gaps]} "
          f"rollout_kl={['%.3e' % float(k['rollout_kl']) for k in kls]} measured={MEASURED_GAP}")
    assert MEASURED_GAP is not None and max(gaps) <= 4 * MEASURED_GAP, (gaps, MEASURED_GAP)
    gen.clear_graph_cache()


def test_fp8_rollouts_show_in_the_monitor_metric():
    """`train/rollout_kl` of monitor mode (objectives.rollout_mismatch) on fp8 rollouts: finite,
    and larger in magnitude than on bf16 rollouts of the same model. The model is
    tiny-llama-d128 widened to the smallest shape the fp8 decode kernels take (H and F multiples
    of 1024, as in test_decode_gpu.py): at H = 512 no projection meets their shape rules, fp8
    rollouts are bitwise the bf16 ones (rollout_kl 1.4069e-04 for both, measured) and there is
    nothing to see."""
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    m = model_of(4096, hidden_size=1024, num_heads=8, num_kv_heads=2, head_dim=128, intermediate_size=2048,
                 num_layers=3)
    _, bf = _gap(m, 0)
    _, f8 = _gap(m, 0, weight_dtype="fp8")
    assert getattr(m.layers[0].mlp.down_proj, "_dla_f8", None) is not None  # the fp8 kernels ran
    kb, k8 = float(bf["rollout_kl"]), float(f8["rollout_kl"])
    print(f"LOGP_STAT rollout-vs-trainer rollout_kl bf16={kb:.4e} fp8={k8:.4e} "
          f"absdiff_max bf16={float(bf['rollout_logp_absdiff_max']):.4e} fp8={float(f8['rollout_logp_absdiff_max']):.4e}")
    assert math.isfinite(k8) and abs(k8) > abs(kb)
    gen.clear_graph_cache()
