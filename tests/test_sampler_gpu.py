"""MI355X: the fused sampler (csrc/sampling.hip: single-block kernel, scalar and vectorised, and
the row-split path for V >= 32768) against the exact fp64 inverse-CDF oracle of _sampler_ref.py,
draw by draw.

Every launch is issued twice and must give the same bits; every token lies in [0, V); on every row
whose kept set the oracle can pin down the token's CDF interval holds u within EPS_U = 2^-15, and
on the others (at most 5 % where top-k / top-p is on) the token lies in the widest admissible set.
Each check prints `SAMPLER_STAT` (path, dtype, mode, draws, ambiguous share, worst excess over the
exact interval, draws that needed any tolerance) before it asserts.

Finite-input tokens of the grid are also compared bitwise with tests/golden/sampler_tokens.npz,
recorded from the kernels before the no-finite-row clamp went in."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import _sampler_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SPLIT_ON = os.environ.get("DLA_SAMPLER_SPLIT", "1")[:1] != "0"  # read once per process, as the op does
CHILD = "DLA_SAMPLER_TEST_CHILD"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_tokens.npz")
INF = float("inf")
PLAIN, TOPK, TOPP, BOTH = (0, 1.0), (50, 1.0), (0, 0.9), (50, 0.9)


@pytest.fixture(scope="module", autouse=True)
def _native():
    from distributed_llm_alignment_amd.ops import _ext

    _ext.require()


def dtype_id(dtype) -> str:
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dtype]


def path_of(x: torch.Tensor) -> str:
    """The kernel sample_tokens picks for these logits (launch_sample / sample_split_chunks)."""
    V = x.shape[1]
    if not (V % 8 == 0 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0):
        return "single-scalar"
    return "split" if V >= 32768 and SPLIT_ON else "single-vec"


def sample(x, T, k, p, seed, counter, greedy=False):
    from distributed_llm_alignment_amd.ops import decode

    rng = torch.tensor([seed, counter], dtype=torch.long, device=x.device)
    a = decode.sample_tokens(x, T, k, p, greedy, rng)
    b = decode.sample_tokens(x, T, k, p, greedy, rng)
    assert torch.equal(a, b), "the same launch twice gave different tokens"
    assert a.dtype == torch.long and a.shape == (x.shape[0],)
    assert bool(((a >= 0) & (a < x.shape[1])).all()), a[(a < 0) | (a >= x.shape[1])][:4]
    return a


def draws(x, T, k, p, seed=7, counters=S.COUNTERS):
    return torch.stack([sample(x, T, k, p, seed, c) for c in counters], 1)


def check(x, T, k, p, seed=7, counters=S.COUNTERS, mode=None, cap=True):
    """Draw [B, len(counters)] tokens and hold each against the oracle."""
    tok = draws(x, T, k, p, seed, counters)
    kept = S.kept_sets(x, T, k, p)
    u = S.u_grid(seed, x.shape[0], counters, x.device)
    c = S.check_draws(kept, tok, u)
    print(f"SAMPLER_STAT path={path_of(x)} dtype={dtype_id(x.dtype)} mode={mode or f'k{k}-p{p}'} T={T} "
          f"V={x.shape[1]} draws={tok.numel()} ambiguous={c.ambiguous_share:.4f} "
          f"worst_excess={c.worst_excess:.3e} needed={c.needed}")
    if not bool(c.ok.all()):
        r, j = (~c.ok).nonzero()[0].tolist()
        t = int(tok[r, j])
        pytest.fail(f"{int((~c.ok).sum())} of {tok.numel()} draws fail; first: row {r} counter {counters[j]} "
                    f"token {t} u {float(u[r, j])!r} interval [{float(kept.Fex[r, t])!r}, {float(kept.F[r, t])!r}) "
                    f"in K_min {bool(kept.kmin[r, t])} in K_max {bool(kept.kmax[r, t])} "
                    f"ambiguous {bool(kept.ambiguous[r])} exact token {int(S.exact_tokens(kept, u)[r, j])}")
    if cap and (0 < k < x.shape[1] or p < 1.0):
        assert c.ambiguous_share <= S.AMBIGUOUS_CAP, c.ambiguous_share
    return kept, tok, c


# ------------------------------------------------------------------------------------ the grid
@functools.lru_cache(maxsize=4)
def grid_logits(builder, V, dtype):
    return S.grid_logits(builder, V, dtype).to(DEV)


def grid_key(x, V, dtype, mode, T) -> str:
    return f"{path_of(x)}/{V}/{dtype_id(dtype)}/{S.mode_id(mode)}/T{T}"


@functools.lru_cache(maxsize=1)
def golden():
    import numpy as np

    return np.load(GOLDEN)


@pytest.mark.parametrize("T", S.TEMPS)
@pytest.mark.parametrize("mode", S.MODES, ids=S.mode_id)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", S.VOCABS)
def test_grid_matches_oracle(V, dtype, mode, T):
    """64 rows x 8 counters per case. V: 4099 single block, scalar (V % 8 != 0); 32760 single block,
    vectorised, the last V below the split; 32768 split, chunks of exactly 128 vectors; 32776 split,
    129-vector chunks and a short last one of 98; 50264 split, 197 / 176; 128256 the workload's
    vocabulary; 50257 the scalar path at a large V."""
    x = grid_logits(mode[0], V, dtype)
    _, tok, _ = check(x, T, mode[1], mode[2], mode=S.mode_id(mode))
    key = grid_key(x, V, dtype, mode, T)
    assert key in golden().files, key
    assert torch.equal(tok.cpu(), torch.from_numpy(golden()[key]).long()), key


def test_single_block_kernel_at_large_vocab():
    """DLA_SAMPLER_SPLIT is read once per process: one fresh child pytest runs this module's grid
    at V = 128256 with the split path off (the single-block kernel, 128 logits per thread)."""
    if os.environ.get(CHILD):
        pytest.skip("the launcher itself is not run in its child")
    env = dict(os.environ, DLA_SAMPLER_SPLIT="0", **{CHILD: "1"})
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s",
           "-k", "test_grid_matches_oracle and 128256"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    stats = [ln[ln.index("SAMPLER_STAT"):] for ln in r.stdout.splitlines() if "SAMPLER_STAT" in ln]
    print("\n".join(stats))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    n = len(S.DTYPES) * len(S.MODES) * len(S.TEMPS)
    assert f"{n} passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
    assert len(stats) == n and all("path=single-vec" in ln for ln in stats)


# ------------------------------------------------------------------------------------ row layout
@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("layout", ["strided", "misaligned"])
@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", [4096, 32768])
def test_row_layouts(V, dtype, layout, B):
    """Rows of a [B, V + 8] buffer: `[:, :V]` keeps 16-byte aligned rows with a row stride that is not
    V (vectorised / split); `[:, 1:V + 1]` is misaligned and must take the scalar single-block
    kernel, at every batch size."""
    counters = S.COUNTERS if B < 300 else (0, 5)
    for builder, (k, p) in (("dense", PLAIN), ("peaked", TOPP)):
        src = {"dense": S.dense, "peaked": S.peaked}[builder](B, V, 100 + B).to(dtype)
        big = torch.full((B, V + 8), 50.0, dtype=dtype, device=DEV)  # a drawn pad column would show
        x = big[:, :V] if layout == "strided" else big[:, 1:V + 1]
        x.copy_(src)
        assert path_of(x) == ("single-scalar" if layout == "misaligned" else "split" if V >= 32768 and SPLIT_ON else "single-vec")
        check(x, 0.9, k, p, counters=counters, mode=f"{layout}-{builder}-k{k}-p{p}", cap=B >= 64)


# ------------------------------------------------------------------------------------ edges
EDGE_V = [4096, 32768]


def spread(V, n):
    """n positions across the row, chunk and segment edges included."""
    return [0, 7, V - 1, 2 * 1024, 2 * 1024 + 1023, V // 2 + 3][:n]


@pytest.mark.parametrize("V", EDGE_V)
def test_ties_across_the_k_boundary_are_all_kept(V):
    """k = 5 with values 10 9 8 7 and three 6s: the kept set is all seven, in every draw."""
    g = torch.Generator().manual_seed(V)
    B = 64
    x = torch.randn(B, V, generator=g) * 0.5 - 3.0
    pos = torch.rand(B, V, generator=g).topk(7, dim=-1).indices
    x.scatter_(1, pos, torch.tensor([10.0, 9.0, 8.0, 7.0, 6.0, 6.0, 6.0]).expand(B, 7).contiguous())
    x = x.to(DEV)
    for p in (1.0, 0.9999):
        kept, tok, _ = check(x, 4.0, 5, p, mode=f"ties-k5-p{p}")
        assert bool((kept.kmin.sum(-1) == 7).all()) and not bool(kept.ambiguous.any())
        tied = (tok.unsqueeze(-1) == pos.to(DEV)[:, None, 4:]).any(-1)
        assert 0.2 < float(tied.double().mean()) < 0.5  # the three 6s hold 0.28 of the mass at T = 4


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V + [4099])
def test_edge_token_a_hair_below_a_coarse_bin_edge(V, dtype):
    """Logits on a 9/16 ladder at T = 0.9: z = -0.625 n up to one fp32 rounding, on or a hair
    below the coarse histogram edges at multiples of 1/32, where z + 64 rounds onto the edge.
    k = 4 and p = 0.9 both end on the fourth rung (cumulative shares 0.468 0.718 0.852 0.924 of
    the eight rungs): it is kept and drawn. (bf16 logits at a temperature like 0.9 put whole rows on such a ladder.)"""
    g = torch.Generator().manual_seed(V)
    x = torch.full((64, V), -30.0)
    pos = torch.rand(64, V, generator=g).topk(8, dim=-1).indices
    x.scatter_(1, pos, (-0.5625 * torch.arange(8.0)).expand(64, 8).contiguous())
    x = x.to(dtype).to(DEV)
    z = S.z_scores(x, 0.9).gather(1, pos.to(DEV)[:, 3:4])
    assert bool(((z < -1.875) & (z > -1.875 - 1e-6)).all())  # the fourth rung: below the edge
    # the renormalised top-4 mass puts the nucleus edge one rung higher: 0.9 * 1.975 < 1.822
    for k, p, n in ((4, 1.0, 4), (0, 0.9, 4), (6, 0.9, 4), (4, 0.9, 3), (3, 1.0, 3), (5, 1.0, 5)):
        kept, tok, _ = check(x, 0.9, k, p, mode=f"bin-edge-k{k}-p{p}")
        assert bool((kept.kmin.sum(-1) == n).all()) and not bool(kept.ambiguous.any())
        last = (tok == pos.to(DEV)[:, n - 1:n]).double().mean()  # the lowest kept rung is drawn
        assert 0.5 * float(last) < [0, 0, 0, 0.157, 0.0777, 0.0399][n] < 2 * float(last)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V + [4099])
def test_all_logits_equal_is_the_segment_layout(V, dtype):
    """Uniform rows: token = floor(u * V) up to the fp32 rounding of u * V, with and without
    top-k / top-p (every token ties with the k-th and has no mass strictly above it)."""
    x = torch.full((64, V), -2.5, dtype=dtype, device=DEV)
    for k, p in (PLAIN, (5, 1.0), (0, 0.5)):
        kept, tok, _ = check(x, 0.8, k, p, mode=f"equal-k{k}-p{p}")
        assert bool(kept.kmin.all())
        u = S.u_grid(7, 64, S.COUNTERS, DEV)
        assert bool(((tok.double() - u * V).abs() <= S.EPS_U * V + 1).all())


@pytest.mark.parametrize("k,p", [PLAIN, (5, 1.0), TOPP, (5, 0.9)])
@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_one_finite_logit_is_always_drawn(V, dtype, k, p):
    """The rest is -inf; the finite one at index 0, 7, V - 1 and in the first and last vector of a
    chunk."""
    pos = spread(V, 6)
    x = torch.full((len(pos), V), -INF, dtype=dtype, device=DEV)
    for r, i in enumerate(pos):
        x[r, i] = -3.0
    expect = torch.tensor(pos, device=DEV)
    for c in (0, 1, 2):
        assert torch.equal(sample(x, 0.9, k, p, 5, c), expect)
    assert torch.equal(sample(x, 1.0, 0, 1.0, 5, 0, greedy=True), expect)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V + [4099])
def test_max_at_the_first_and_last_index(V, dtype):
    x = S.dense(64, V, 9)
    top = x.max(-1).values + 2.0
    x[:32, 0] = top[:32]
    x[32:, V - 1] = top[32:]
    x = x.to(dtype).to(DEV)
    am = torch.where(torch.arange(64, device=DEV) < 32, 0, V - 1)
    assert torch.equal(sample(x, 1.0, 0, 1.0, 5, 0, greedy=True), am)
    assert torch.equal(sample(x, 0.0, 0, 1.0, 5, 0), am)  # temperature 0 is greedy
    assert torch.equal(sample(x, 0.7, 1, 1.0, 5, 0), am)
    for k, p in (PLAIN, TOPK):
        _, tok, _ = check(x, 1.0, k, p, mode=f"max-at-ends-k{k}-p{p}")
        assert 0.15 < float((tok == am[:, None]).double().mean()) < 1.0  # drawn, and not always


@pytest.mark.parametrize("V", EDGE_V)
def test_k_and_p_extremes(V):
    """k = 1 without the greedy flag, k = V - 1, k >= V (inactive), p = 1e-6 (the argmax and its
    ties only)."""
    x = S.dense(64, V, 13).to(DEV)
    am = x.argmax(-1)
    for c in (0, 1, 2):
        assert torch.equal(sample(x, 1.3, 1, 1.0, 5, c), am)
        assert torch.equal(sample(x, 1.3, 0, 1e-6, 5, c), am)
    check(x, 1.0, V - 1, 1.0, mode="k=V-1")
    for k in (V, V + 7):
        kept, tok, _ = check(x, 1.0, k, 1.0, mode="k>=V")
        assert bool(kept.kmin.all())
        assert torch.equal(tok, draws(x, 1.0, 0, 1.0))
    xt = x.clone()
    xt[:, 5] = xt[:, V - 9] = x.max(-1).values + 1.0  # two tied maxima
    tok = draws(xt, 1.3, 0, 1e-6)
    assert bool(((tok == 5) | (tok == V - 9)).all()) and 0.3 < float((tok == 5).double().mean()) < 0.7
    kept, _, _ = check(xt, 1.3, 0, 1e-6, mode="p=1e-6-ties")
    assert bool((kept.kmin.sum(-1) == 2).all())
    assert bool((draws(xt, 1.3, 1, 1.0) == tok).all())  # k = 1 keeps both ties too


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_temperature_extremes(V, dtype):
    """T = 0.05: most of the row is below the -64 window and must never be drawn. T = 5 on
    `peaked`: a flat head over a heavy tail."""
    x = S.dense(64, V, 17).to(dtype).to(DEV)
    for k, p in (PLAIN, TOPK, TOPP):
        kept, _, _ = check(x, 0.05, k, p, mode=f"T0.05-dense-k{k}-p{p}")
    assert float(S.kept_sets(x, 0.05, 0, 1.0).kmin.double().mean()) < 0.2
    x = S.peaked(64, V, 19).to(dtype).to(DEV)
    for k, p in (PLAIN, BOTH, (20, 1.0)):
        check(x, 5.0, k, p, mode=f"T5-peaked-k{k}-p{p}")


SEEDS = (0, 1, 2 ** 31, 2 ** 32 + 5, 2 ** 62, -1, -2 ** 63)


@pytest.mark.parametrize("V", EDGE_V)
def test_seed_and_counter_words(V):
    """Seeds and counters with high words and the sign bit set: the int64 -> uint64
    reinterpretation and the (lo, hi) word order match the reference."""
    x = S.peaked(16, V, 23).to(torch.bfloat16).to(DEV)
    kept = S.kept_sets(x, 1.0, 0, 0.9)
    assert not bool(kept.ambiguous.any())
    seen = set()
    for seed in SEEDS:
        tok = draws(x, 1.0, 0, 0.9, seed, SEEDS)
        u = S.u_grid(seed, 16, SEEDS, DEV)
        c = S.check_draws(kept, tok, u)
        assert bool(c.ok.all()), (seed, (~c.ok).nonzero()[:4])
        seen.add(tuple(tok.flatten().tolist()))
    assert len(seen) == len(SEEDS)


@pytest.mark.parametrize("V", EDGE_V)
def test_identical_rows_draw_per_row_uniforms(V):
    """A contiguous repeat of one row (a GRPO group): every row draws at its own u."""
    x = S.peaked(1, V, 29).to(torch.bfloat16).to(DEV).repeat(64, 1)
    for k, p in (PLAIN, TOPP):
        _, tok, _ = check(x, 1.0, k, p, mode=f"identical-rows-k{k}-p{p}")
        assert all(len(set(tok[:, j].tolist())) > 3 for j in range(tok.shape[1]))


# ------------------------------------------------------------------------------------ non-finite
# Only the sampler op is called here; its tokens go nowhere else.
def layouts(x):
    """The same rows on each kernel the width admits: as they are, and misaligned (scalar)."""
    big = torch.zeros((x.shape[0], x.shape[1] + 8), dtype=x.dtype, device=x.device)
    mis = big[:, 1:x.shape[1] + 1]
    mis.copy_(x)
    return [x, mis]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_nan_and_neg_inf_are_never_drawn(V, dtype):
    g = torch.Generator().manual_seed(31)
    x = S.peaked(64, V, 31)
    r = torch.rand(64, V, generator=g)
    x[r < 0.1] = float("nan")
    x[(r >= 0.1) & (r < 0.2)] = -INF
    x[:, 0] = float("nan")
    x[:, V - 1] = -INF
    x = x.to(dtype).to(DEV)
    finite = torch.isfinite(x)
    for y in layouts(x):
        for k, p in (PLAIN, TOPK, TOPP, BOTH):
            kept, tok, _ = check(y, 1.0, k, p, mode=f"nan-inf-k{k}-p{p}")
            assert bool(finite.gather(1, tok).all())
        g_tok = sample(y, 1.0, 0, 1.0, 5, 0, greedy=True)
        assert torch.equal(g_tok, torch.where(finite, x.float(), torch.full_like(x, -INF, dtype=torch.float32)).argmax(-1))


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_pos_inf_returns_its_first_index(V, dtype):
    x = S.dense(6, V, 37)
    first = spread(V, 6)
    for r, i in enumerate(first):
        x[r, i] = INF
        if i + 9 < V:
            x[r, i + 9] = INF  # a second one later in the row
    x[3, 1] = float("nan")
    x = x.to(dtype).to(DEV)
    expect = torch.tensor(first, device=DEV)
    for y in layouts(x):
        for k, p in (PLAIN, TOPK, TOPP, BOTH):
            assert torch.equal(sample(y, 0.9, k, p, 5, 1), expect), (k, p)
        assert torch.equal(sample(y, 1.0, 0, 1.0, 5, 0, greedy=True), expect)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=dtype_id)
@pytest.mark.parametrize("V", EDGE_V)
def test_row_without_a_finite_logit_returns_token_zero(V, dtype):
    """All -inf, all NaN, and a mix: token 0, which is what torch.argmax gives for an all -inf
    row; greedy, single-block (vectorised and scalar) and split. Finite rows next to them are
    unaffected."""
    x = S.dense(5, V, 41)
    x[0] = -INF
    x[1] = float("nan")
    x[2, ::2] = -INF
    x[2, 1::2] = float("nan")
    x[3, 1:] = -INF  # one finite logit, at 0
    x = x.to(dtype).to(DEV)
    am4 = int(x[4].float().argmax())
    for y in layouts(x):
        for k, p in (PLAIN, TOPK, TOPP, BOTH):
            tok = sample(y, 0.9, k, p, 5, 1)
            assert tok[:4].tolist() == [0, 0, 0, 0], (path_of(y), k, p, tok.tolist())
        assert sample(y, 1.0, 0, 1.0, 5, 0, greedy=True).tolist() == [0, 0, 0, 0, am4]
        assert sample(y, 0.0, 0, 1.0, 5, 0).tolist() == [0, 0, 0, 0, am4]
