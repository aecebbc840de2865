"""CPU tier: the fp64 inverse-CDF oracle of tests/_sampler_ref.py is right and has teeth.

Philox against the published known-answer vectors; the ambiguity cap on every case the GPU module
(test_sampler_gpu.py) parametrises; agreement with the package's CPU sampling branch
(models.generation.sample_next); and the draw checker rejecting samplers that are wrong in the
ways a kernel can be wrong."""
import math

import pytest
import torch

import _sampler_ref as S

KAT = [  # Random123 kat_vectors, philox4x32 10 rounds
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((S.M32,) * 4, (S.M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
EDGE_INTS = (0, 1, 2 ** 31, 2 ** 32 + 5, 2 ** 62, -1, -2 ** 63)


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert S.philox4x32_10(ctr, key) == out


def test_philox_word_layout_and_u01_range():
    # counter words (row_lo, row_hi, ctr_lo, ctr_hi), key (seed_lo, seed_hi), int64 as uint64
    assert S.philox_words(-1, -1, -1) == KAT[1][2]
    seed = (0x299f31d0 << 32 | 0xa4093822) - 2 ** 64  # a negative int64
    assert S.philox_words(seed, 0x85a308d3 << 32 | 0x243f6a88, 0x03707344 << 32 | 0x13198a2e) == KAT[2][2]
    us = [S.philox_u01(s, r, c) for s in EDGE_INTS for r in (0, 1, 63, 299) for c in EDGE_INTS]
    assert all(0.0 <= u < 1.0 for u in us)
    assert all(u * 2 ** 24 == int(u * 2 ** 24) for u in us)  # a 24-bit fraction, exact
    assert S.philox_u01(0, 0, 0) == (0x6627e8d5 >> 8) * 2.0 ** -24


def test_philox_distinct_row_counter_give_distinct_words():
    words = {S.philox_words(7, r, c) for r in range(64) for c in range(64)}
    assert len(words) == 64 * 64
    # the high words count: 2^32 + 5 is not 5, and the seed's two words are not interchangeable
    assert S.philox_words(7, 5, 0) != S.philox_words(7, 2 ** 32 + 5, 0)
    assert S.philox_words(7, 0, 5) != S.philox_words(7, 0, 2 ** 32 + 5)
    assert S.philox_words(5, 0, 0) != S.philox_words(5 << 32, 0, 0)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", S.VOCABS)
def test_ambiguity_cap_on_the_gpu_grid(V, dtype):
    """A condition of the grid, not a measurement of the kernel: wherever top-k or top-p is active,
    at most 5 % of the rows may fall back to the weak check."""
    for builder in ("dense", "peaked"):
        x = S.grid_logits(builder, V, dtype)
        for mode in S.MODES:
            if mode[0] != builder or (mode[1] == 0 and mode[2] >= 1.0):
                continue
            for T in S.TEMPS:
                share = float(S.kept_sets(x, T, mode[1], mode[2]).ambiguous.double().mean())
                print(f"ambiguous V={V} {dtype} {S.mode_id(mode)} T={T}: {share:.4f}")
                assert share <= S.AMBIGUOUS_CAP, (mode, T, share)


def test_plain_sampling_is_never_ambiguous_and_keeps_the_window():
    x = torch.tensor([[0.0, -10.0, -44.0, -45.5, float("-inf"), float("nan")]])
    k = S.kept_sets(x, 0.7, 0, 1.0)  # z = x / 0.7: -44 -> -62.9 inside, -45.5 -> -65 outside
    assert k.kmin.tolist() == [[True, True, True, False, False, False]]
    assert torch.equal(k.kmin, k.kmax) and not bool(k.ambiguous.any())


def test_kept_set_definitions_on_a_hand_example():
    # weights 8 4 2 1 1 (base-2 logits): exact nucleus and tie handling, checked by hand
    x = (torch.tensor([[1.0, 3.0, 0.0, 2.0, 0.0]]) * math.log(2.0)).double()
    k = S.kept_sets(x, 1.0, 0, 0.49)  # mass above 8 is 0: kept; above 4 is 8 > 7.84: not
    assert k.kmin.tolist() == [[False, True, False, False, False]]
    k = S.kept_sets(x, 1.0, 0, 0.51)
    assert k.kmin.tolist() == [[False, True, False, True, False]]
    k = S.kept_sets(x, 1.0, 4, 1.0)   # the 4th value is tied with the 5th: both kept
    assert k.kmin.tolist() == [[True] * 5]
    k = S.kept_sets(x, 1.0, 3, 0.9)   # top-3 mass 14, 0.9 * 14 = 12.6 > 12: all three
    assert k.kmin.tolist() == [[True, True, False, True, False]]
    k = S.kept_sets(x, 1.0, 0, 0.8)   # un-renormalised the same p would stop at 12 < 12.8 too...
    assert k.kmin.tolist() == [[True, True, False, True, False]]
    k = S.kept_sets(x, 1.0, 3, 0.85)  # ...but 0.85 * 14 = 11.9 <= 12 drops the third token
    assert k.kmin.tolist() == [[False, True, False, True, False]]
    k = S.kept_sets(x, 1.0, 5, 1.0)   # k >= V: inactive
    assert k.kmin.all()
    # the CDF is in index order
    k = S.kept_sets(x, 1.0, 0, 1.0)
    assert torch.allclose(k.F[0], torch.tensor([2, 10, 11, 15, 16], dtype=torch.float64) / 16)
    u = torch.tensor([[0.0, 0.124, 0.126, 0.63, 0.93, 0.9999]], dtype=torch.float64)
    assert S.exact_tokens(k, u).tolist() == [[0, 0, 1, 2, 3, 4]]


CPU_BRANCH_MODES = [(0, 0.9, 1.0), (0, 0.5, 0.7), (5, 1.0, 1.3), (20, 0.9, 5.0), (8, 0.7, 1.3)]


@pytest.mark.parametrize("top_k,top_p,T", CPU_BRANCH_MODES)
def test_reference_agrees_with_cpu_branch(top_k, top_p, T):
    """models.generation.sample_next (sort + multinomial) on a 64-token peaked vocabulary: over
    4000 seeded draws per row the set of drawn tokens is K_min and the frequencies match
    w / sum(w) within 4 sigma binomial."""
    from distributed_llm_alignment_amd.models.generation import sample_next

    N = 4000
    x = S.peaked(8, 64, 11)
    kept = S.kept_sets(x, T, top_k, top_p)
    rows = [r for r in range(8) if not bool(kept.ambiguous[r])][:4]
    assert len(rows) == 4
    g = torch.Generator().manual_seed(1234)
    for r in rows:
        tok = sample_next(x[r].expand(N, -1).contiguous(), True, T, top_p, top_k, g)
        freq = torch.bincount(tok, minlength=64).double() / N
        p = kept.F[r] - kept.Fex[r]
        members = kept.kmin[r]
        assert float(p[members].min()) * N >= 30  # every member is drawn (misses: e^-30)
        assert torch.equal(freq > 0, members), (r, freq.nonzero().flatten(), members.nonzero().flatten())
        sigma = (p * (1 - p) / N).sqrt()
        assert bool(((freq - p).abs() <= 4 * sigma + 1e-12).all()), (r, (freq - p).abs() / sigma)


# ------------------------------------------------------------------------------------ teeth
MB, MV, MSEED = 64, 4099, 77


def _fail_share(kept, tokens, u):
    return 1.0 - float(S.check_draws(kept, tokens, u).ok.double().mean())


@pytest.fixture(scope="module")
def mut():
    x = S.peaked(MB, MV, 5)
    u = S.u_grid(MSEED, MB, S.COUNTERS)
    return x, u


def test_checker_accepts_the_exact_sampler(mut):
    x, u = mut
    for k, p, T in ((0, 1.0, 1.0), (0, 0.9, 1.0), (20, 0.9, 5.0), (3, 1.0, 1.0)):
        kept = S.kept_sets(x, T, k, p)
        c = S.check_draws(kept, S.exact_tokens(kept, u), u)
        assert bool(c.ok.all()) and c.worst_excess == 0.0 and c.needed == 0
        assert c.ambiguous_share <= S.AMBIGUOUS_CAP


def test_checker_rejects_next_kept_token(mut):
    x, u = mut
    kept = S.kept_sets(x, 1.0, 0, 0.9)
    tok = S.exact_tokens(kept, u)
    idx = torch.arange(MV).expand(MB, MV)
    nxt = torch.empty_like(tok)
    for r in range(MB):  # the next kept index, cyclically
        members = idx[r][kept.kmin[r]]
        pos = torch.searchsorted(members, tok[r])
        nxt[r] = members[(pos + 1) % len(members)]
    assert _fail_share(kept, nxt, u) >= 0.95


@pytest.mark.parametrize("which", ["row+1", "counter+1", "seed-words-swapped"])
def test_checker_rejects_wrong_uniform(mut, which):
    x, u = mut
    kept = S.kept_sets(x, 1.0, 0, 0.9)
    if which == "row+1":
        u2 = S.u_grid(MSEED, MB + 1, S.COUNTERS)[1:]
    elif which == "counter+1":
        u2 = S.u_grid(MSEED, MB, [c + 1 for c in S.COUNTERS])
    else:
        seed = (3 << 32) | 9
        u = S.u_grid(seed, MB, S.COUNTERS)
        u2 = S.u_grid((9 << 32) | 3, MB, S.COUNTERS)
    assert _fail_share(kept, S.exact_tokens(kept, u2), u) >= 0.25


def test_checker_rejects_top_p_on_unrenormalised_mass(mut):
    """k = 20, p = 0.9 at T = 5, where the top-20 hold well under 90 % of the row's mass: p taken
    of the whole row's mass keeps all 20 instead of the nucleus of the renormalised top-20."""
    x, u = mut
    T, k, p = 5.0, 20, 0.9
    kept = S.kept_sets(x, T, k, p)
    z = kept.z
    sz, _ = z.sort(-1, descending=True)
    topk = z >= sz[:, k - 1:k]
    w = sz.exp()
    before = w.cumsum(-1) - w
    keep_sorted = (before < p * w.sum(-1, keepdim=True)) & (sz >= sz[:, k - 1:k])  # un-renormalised
    edge = torch.where(keep_sorted, sz, torch.full_like(sz, float("inf"))).min(-1, keepdim=True).values
    wrong = topk & (z >= edge)
    assert bool((wrong != kept.kmin).any(-1).all())
    bad = kept._replace(kmin=wrong, **dict(zip(("F", "Fex"), S.cdf(z, wrong))))
    assert _fail_share(kept, S.exact_tokens(bad, u), u) >= 0.25


def test_checker_rejects_k_plus_one(mut):
    x, u = mut
    kept = S.kept_sets(x, 1.0, 3, 1.0)
    assert _fail_share(kept, S.exact_tokens(S.kept_sets(x, 1.0, 4, 1.0), u), u) >= 0.25


def test_checker_rejects_cdf_in_sorted_order(mut):
    x, u = mut
    kept = S.kept_sets(x, 1.0, 0, 0.9)
    w = torch.where(kept.kmin, kept.z.exp(), torch.zeros_like(kept.z))
    sw, si = w.sort(-1, descending=True)
    F = sw.cumsum(-1) / sw.sum(-1, keepdim=True)
    pos = torch.searchsorted(F, u.contiguous(), right=True).clamp(max=MV - 1)
    tok = si.gather(1, pos)
    assert bool(kept.kmin.gather(1, tok).all())  # the right set, the wrong order
    assert _fail_share(kept, tok, u) >= 0.25
