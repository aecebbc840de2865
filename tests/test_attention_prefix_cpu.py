"""Prefix-shared attention on the CPU: the two forms of the mask agree on the layouts
`shared_prefix_pack` produces, the mask is what a per-rollout construction gives, the inputs of
_attn_prefix_ref64.py are sensitive to every off-by-one of the new edges, and
`ops.attention.ref_attention(prefix=)` (the CPU formula of record) matches the fp64 reference."""
import pytest
import torch

import _attn_prefix_ref64 as PR
import _attn_ref64 as R
from _attn_ref64 import F64

CORE = [c for c in PR.cases() if c.entry == "core"]


def _grid(S, T, P, G, lpad=(), seed=0):
    """[S, T] rollouts of S / G prompts (equal columns 0:P inside a group); lpad: per group, the
    number of left-padding columns."""
    g = torch.Generator().manual_seed(seed)
    B = S // G
    prompts = torch.randint(3, 400, (B, P), generator=g)
    seqs = torch.cat([prompts.repeat_interleave(G, 0), torch.randint(3, 400, (S, T - P), generator=g)], 1)
    mask = torch.ones(S, T, dtype=torch.long)
    for b, n in enumerate(lpad):
        mask[b * G:(b + 1) * G, :n] = 0
    return seqs, mask


@pytest.mark.parametrize("S,T,P,G,lpad", [(6, 11, 6, 3, (2, 0)), (8, 110, 70, 4, (0, 5)), (4, 9, 2, 2, (0, 1)),
                                          (3, 8, 7, 1, (3, 0, 0)), (4, 40, 33, 4, (32,))])
def test_pack_masks_agree_and_match_per_rollout(S, T, P, G, lpad):
    from distributed_llm_alignment_amd.models.transformer import attention_layout, shared_prefix_pack
    from distributed_llm_alignment_amd.ops.attention import _visibility, prefix_masks_agree

    seqs, mask = _grid(S, T, P, G, lpad)
    ids, pos, segs, prefix, slot_map = shared_prefix_pack(seqs, mask, P, G)
    B, Lp, n1 = S // G, P - 1, T - P + 1
    L = Lp + G * n1
    assert ids.shape == (B, L) and segs.shape == (2, B, L) and prefix.shape == (B, 3) and segs.dtype == torch.int32
    assert prefix_masks_agree(segs, prefix)
    # brute force: slot -> (rollout, column); slot x sees slot y iff they are cells of one rollout
    # (a prefix slot stands for that column of every rollout of its group), y's column is real and
    # not after x's, and x is not a prefix slot looking at a segment slot
    first, _, pos_grid = attention_layout(mask)
    vis = _visibility(B, L, L, True, 0, 0, None, None, "cpu", segs, prefix)
    for b in range(B):
        cell = [(None, s) for s in range(Lp)] + [(g, Lp + k) for g in range(G) for k in range(n1)]
        f = int(first[b * G])
        for x, (gx, cx) in enumerate(cell):
            for y, (gy, cy) in enumerate(cell):
                want = cy <= cx and cy >= f and (gy is None or gy == gx) and cx >= f
                if gx is None and cx < f:
                    want = False
                assert bool(vis[b, x, y]) == want, (b, x, y)
            r = b * G + (gx or 0)
            assert ids[b, x] == seqs[r, cx] and pos[b, x] == pos_grid[r, cx]
            assert slot_map[b, x] == (-1 if gx is None else r * T + cx)


def test_pack_rejects_bad_shapes():
    from distributed_llm_alignment_amd.models.transformer import shared_prefix_pack

    seqs, mask = _grid(6, 11, 6, 3)
    for P, G in ((6, 4), (1, 3), (11, 3)):
        with pytest.raises(ValueError):
            shared_prefix_pack(seqs, mask, P, G)


@pytest.mark.parametrize("c", PR.cases(), ids=lambda c: c.name)
def test_case_masks_agree_and_budget(c):
    """The hand-built cases: both forms are one set, and max e_ij <= EMAX (asserted by build)."""
    from distributed_llm_alignment_amd.ops.attention import _visibility, prefix_masks_agree

    inp = PR.built(c)[0]
    assert inp["emax"] <= R.EMAX
    assert prefix_masks_agree(inp["segs"], inp["prefix"])
    assert torch.equal(PR.visibility(c, inp), PR.backward_form(c, inp))
    assert torch.equal(PR.visibility(c, inp),
                       _visibility(c.B, c.Tk, c.Tk, True, 0, 0, None, None, "cpu", inp["segs"], inp["prefix"]))


@pytest.mark.parametrize("mut", PR.MUTATIONS)
def test_inputs_sensitive_to_mutation(mut):
    """Every mutation of the mask that changes it on a case moves at least one output of the fp64
    reference past the unmutated bound there; and every mutation changes the mask of some case."""
    from distributed_llm_alignment_amd.ops.attention import _visibility

    hit = 0
    for c in CORE:
        inp, r, bnd, _ = PR.built(c)
        # the unmutated mask is the library's own forward form, not only the helper's
        base = _visibility(c.B, c.Tk, c.Tk, True, 0, 0, None, None, "cpu", inp["segs"], inp["prefix"])
        assert torch.equal(base, PR.visibility(c, inp))
        if torch.equal(PR.visibility(c, inp, mut), base):
            continue
        hit += 1
        rm = PR.reference(inp, c, mut=mut)
        res = R.ratios({k: rm[k] for k in R.OUTPUTS}, r, bnd)
        print(f"FIG prefix mutation {mut} {c.name}: {R.fmt(res)}")
        assert max(res.values()) > 1.0, f"{c.name}: {mut} stays inside the bound ({R.fmt(res)})"
    assert hit > 0, f"{mut} changes no case's mask"


@pytest.mark.parametrize("c", CORE, ids=lambda c: c.name)
def test_ref_attention_prefix_against_fp64(c):
    from distributed_llm_alignment_amd.ops.attention import ref_attention

    inp, r, bnd, _ = PR.built(c)
    o = ref_attention(inp["q"], inp["k"], inp["v"], c.scale, True, 0, 0, None, None, inp["segs"], inp["prefix"])
    err = (o.to(F64) - r["o"]).abs()
    # fp32 math on the bf16 inputs, one bf16 rounding of the output
    tol = R.bf16_ulp(r["o"]) + 1e-4 * r["o"].abs().max()
    print(f"FIG prefix ref_attention {c.name}: max err {err.max().item():.3e}")
    assert (err <= tol).all()
    assert (o[r["nokey"].transpose(1, 2)] == 0).all()


def test_prefix_needs_segs_and_no_window():
    from distributed_llm_alignment_amd.ops.attention import ref_attention

    c = CORE[0]
    inp = PR.built(c)[0]
    with pytest.raises(ValueError):
        ref_attention(inp["q"], inp["k"], inp["v"], c.scale, True, 0, 0, None, None, None, inp["prefix"])
    with pytest.raises(ValueError):
        ref_attention(inp["q"], inp["k"], inp["v"], c.scale, True, 0, 16, None, None, inp["segs"], inp["prefix"])
