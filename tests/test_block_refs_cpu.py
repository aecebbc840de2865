"""CPU tier of the block-kernel pins (norm, SwiGLU / GELU, RoPE, embedding, reward head).

1. Each fp64 reference of tests/_refs64_block.py agrees with the package's CPU branch in fp32
   (_branch32_block.py: ops.add_norm, ops.swiglu, ops.gelu_new, _ref_rope, F.embedding with
   autograd, the reward model's PyTorch head) on every case of the GPU module's grids. Bound as in
   test_refs64_cpu.py: a short fp32 formula on well-scaled inputs must agree to 1e-4 of the
   output's largest magnitude; a wrong formula is off by percents.
2. Planted defects: the fp32 branch's output with one defect of the kind these kernels can have
   (a dropped partial, a wrong row, an unwritten chunk ...), rounded to the kernel's output type,
   must be REJECTED by the very check and bound the GPU module applies, while the unchanged branch
   output passes it. A defect that passes fails the test: the bound would be too wide to see it.
3. The builders assert their own edge placement (which runs cross which chunk boundaries, which
   grid sizes leave stage-1 splits empty, which shapes cross a block cap).
"""
import pytest
import torch

import _branch32_block as B32
import _refs64 as R
import _refs64_block as RB
from _refs64 import F64, d

from distributed_llm_alignment_amd import ops


def agree(name, cpu, ref, keys=None, rel=1e-4):
    for k in keys or ref:
        a, b = d(cpu[k]).reshape(-1), d(ref[k]).reshape(-1)
        assert a.shape == b.shape, f"{name}/{k}"
        e32 = R.e32_of(cpu[k], ref[k])
        scale = b.abs().max().item() if b.numel() else 0.0
        print(f"E32 {name} {k}: {e32:.3e} (scale {scale:.3e})")
        assert torch.isfinite(a).all() and e32 <= rel * scale + 1e-30, f"{name}/{k}: {e32:.3e} vs scale {scale:.3e}"


def rejected(kernel, name, bad, ref, e32, extra=0.0, bf16=False):
    """The check must fail on `bad`."""
    with pytest.raises(AssertionError):
        RB.check(kernel, name + "/defect", bad, ref, e32, extra, bf16)


def as_bf16(x):
    return x.to(RB.BF)


# ------------------------------------------------------------------------------------------ norm
@pytest.mark.parametrize("rows,H,rms,res,bias,eps", RB.norm_grid_cases())
def test_norm_fwd_reference(rows, H, rms, res, bias, eps):
    c, groups = RB.norm_case(rows, H, rms, res, bias)
    ref = RB.norm64(c["x"], c["res"], c["w"], c["b"], eps, rms)
    b32 = B32.norm(c["x"], c["res"], c["w"], c["b"], eps, rms)
    assert torch.equal(ref["s"], d(b32["s"]))
    for gname, idx in groups.items():
        if idx.numel():
            agree(f"norm_fwd[{gname}]", {k: v[idx] for k, v in b32.items()}, {k: v[idx] for k, v in ref.items()},
                  keys=["y", "rstd"] + ([] if rms else ["mean"]))
    if res:  # the package's own stream (bf16 add) is the contract's stream
        _, s = ops.add_norm(c["x"], c["res"], c["w"], c["b"], eps, rms)
        assert torch.equal(s, RB.stream(c["x"], c["res"]))


@pytest.mark.parametrize("rows,H,rms,dres,bias,eps", RB.norm_bwd_cases())
def test_norm_bwd_reference(rows, H, rms, dres, bias, eps):
    c, groups = RB.norm_case(rows, H, rms, False, bias)
    f = RB.norm64(c["x"], None, c["w"], c["b"], eps, rms)
    dr = c["dres"] if dres else None
    ref, _ = RB.norm_bwd64(c["dy"], c["x"], c["w"], f["rstd"].float(), f["mean"].float(), dr, eps, rms, bias)
    b32 = B32.norm_bwd(c["dy"], c["x"], c["w"], dr, eps, rms, bias)
    for gname, idx in groups.items():
        if idx.numel():
            agree(f"norm_bwd[{gname}]", {"ds": b32["ds"][idx]}, {"ds": ref["ds"][idx]})
    agree("norm_bwd", b32, ref, keys=["dw"] + (["db"] if bias else []))


def test_norm_grid_covers_the_dispatch_edges():
    fwd = RB.norm_grid_cases()
    assert {RB.norm_fwd_nc(H) for r, H, *_ in fwd if r >= 512} == {1, 2, 4, 8, 16}
    assert any(r >= 512 and r % 4 for r, *_ in fwd) and any(r < 512 for r, *_ in fwd)
    assert any(r >= 512 and (H // 8) % 64 for r, H, *_ in fwd)  # a partial last chunk
    assert {(rms, res, b) for _, _, rms, res, b, _ in fwd} == set(RB.NORM_FLAGS)
    for kern in (lambda r: r < 512, lambda r: r >= 512):
        assert {(rms, res, b) for r, _, rms, res, b, _ in fwd if kern(r)} == set(RB.NORM_FLAGS)
    bwd = RB.norm_bwd_cases()
    assert {r for r, *_ in bwd} == set(RB.NORM_BWD_ROWS) and {H for _, H, *_ in bwd} == set(RB.NORM_BWD_H)
    assert {(rms, dr, b) for _, _, rms, dr, b, _ in bwd} == set(RB.NORM_FLAGS)
    # 5 rows: per = 1, splits 5..15 empty; 769: block 0 takes a second row; 1537: a third (parity back to 0)
    assert min(5, RB.NORM_BWD_GRID) < RB.K_SPLIT
    assert (769 - 1) // RB.NORM_BWD_GRID == 1 and (1537 - 1) // RB.NORM_BWD_GRID == 2


def test_rms_norm_with_bias_is_rejected():
    x, w = torch.randn(4, 16), torch.ones(16)
    with pytest.raises(ValueError):
        ops.add_norm(x, None, w, torch.zeros(16), 1e-5, True)
    with pytest.raises(ValueError):
        ops.add_norm(x.bfloat16(), x.bfloat16(), w.bfloat16(), torch.zeros(16).bfloat16(), 1e-6, True)
    ops.add_norm(x, None, w, torch.zeros(16), 1e-5, False)  # LayerNorm with a bias stays valid
    ops.add_norm(x, None, w, None, 1e-5, True)


def _bwd_setup(rows, H, rms, bias, eps=1e-5):
    c, groups = RB.norm_case(rows, H, rms, False, bias)
    f = RB.norm64(c["x"], None, c["w"], c["b"], eps, rms)
    ref, xh = RB.norm_bwd64(c["dy"], c["x"], c["w"], f["rstd"].float(), f["mean"].float(), None, eps, rms, bias)
    b32 = B32.norm_bwd(c["dy"], c["x"], c["w"], None, eps, rms, bias)
    ex = RB.norm_bwd_extra(c["dy"], c["w"], xh, f["rstd"], H, rows, groups, rms)
    return c, groups, f, ref, xh, b32, ex


def test_defect_dw_missing_one_row_of_769():
    c, groups, f, ref, xh, b32, ex = _bwd_setup(769, 2056, True, False)
    e32 = R.e32_of(b32["dw"], ref["dw"])
    RB.check("norm_bwd", "dw/clean", as_bf16(b32["dw"]), ref["dw"], e32, ex["dw"], True)
    bad = b32["dw"] - (c["dy"][768].float() * xh[768].float())  # the row of block 0's second trip
    rejected("norm_bwd", "dw", as_bf16(bad), ref["dw"], e32, ex["dw"], True)


@pytest.mark.parametrize("which", ["dw", "db"])
def test_defect_wgrad_from_15_of_16_splits(which):
    c, groups, f, ref, xh, b32, ex = _bwd_setup(769, 2056, False, True)
    per = (RB.NORM_BWD_GRID + RB.K_SPLIT - 1) // RB.K_SPLIT
    blocks = torch.arange(15 * per, 768)  # the partial rows of stage-1 split 15
    term = c["dy"].float() * (xh.float() if which == "dw" else 1.0)
    e32 = R.e32_of(b32[which], ref[which])
    RB.check("norm_bwd", which + "/clean", as_bf16(b32[which]), ref[which], e32, ex[which], True)
    rejected("norm_bwd", which, as_bf16(b32[which] - term[blocks].sum(0)), ref[which], e32, ex[which], True)


def test_defect_layernorm_ds_without_sum_g():
    c, groups, f, ref, xh, b32, ex = _bwd_setup(300, 2048, False, False)
    mg = (c["dy"].float() * c["w"].float()).mean(-1, keepdim=True)
    bad = b32["ds"] + f["rstd"].float()[:, None] * mg
    for gname, idx in groups.items():
        e32 = R.e32_of(b32["ds"][idx], ref["ds"][idx])
        RB.check("norm_bwd", f"ds[{gname}]/clean", as_bf16(b32["ds"][idx]), ref["ds"][idx], e32, ex["ds"][gname], True)
        rejected("norm_bwd", f"ds[{gname}]", as_bf16(bad[idx]), ref["ds"][idx], e32, ex["ds"][gname], True)


def _fwd_setup(rows, H, rms, res, bias, eps=1e-5):
    c, groups = RB.norm_case(rows, H, rms, res, bias)
    ref = RB.norm64(c["x"], c["res"], c["w"], c["b"], eps, rms)
    b32 = B32.norm(c["x"], c["res"], c["w"], c["b"], eps, rms)
    ex = RB.norm_fwd_extra(ref, c["w"], H, rows, groups, eps)
    return c, groups, ref, b32, ex


def test_defect_bias_dropped():
    c, groups, ref, b32, ex = _fwd_setup(515, 520, False, True, True)
    idx = groups["bulk"]
    e32 = R.e32_of(b32["y"][idx], ref["y"][idx])
    RB.check("norm_fwd", "y/clean", as_bf16(b32["y"][idx]), ref["y"][idx], e32, ex["y"]["bulk"], True)
    rejected("norm_fwd", "y", as_bf16(b32["y"] - c["b"].float())[idx], ref["y"][idx], e32, ex["y"]["bulk"], True)


@pytest.mark.parametrize("rows,H", [(5, 4096), (513, 8192)])
def test_defect_one_pass_variance_on_large_mean_rows(rows, H):
    """E[x^2] - mean^2 in fp32 on the mean-30, std-0.5 rows: the cancellation costs ~1e-4 of the
    variance, which the fp32 output rstd shows (y, rounded to bf16, cannot)."""
    eps = 1e-5
    c, groups, ref, b32, ex = _fwd_setup(rows, H, False, False, True, eps)
    idx = groups["mean30"]
    assert idx.numel() >= 1
    s = c["x"].float()[idx]
    onepass = torch.rsqrt((s * s).mean(-1) - s.mean(-1) ** 2 + eps)
    e32 = R.e32_of(b32["rstd"][idx], ref["rstd"][idx])
    RB.check("norm_fwd", "rstd[mean30]/clean", b32["rstd"][idx], ref["rstd"][idx], e32, ex["rstd"]["mean30"])
    rejected("norm_fwd", "rstd[mean30]", onepass, ref["rstd"][idx], e32, ex["rstd"]["mean30"])


def test_defect_last_chunk_unnormalised():
    c, groups, ref, b32, ex = _fwd_setup(513, 4104, True, True, False)
    idx = groups["bulk"]
    bad = b32["y"].clone()
    bad[:, -8:] = b32["s"][:, -8:]
    e32 = R.e32_of(b32["y"][idx], ref["y"][idx])
    rejected("norm_fwd", "y", as_bf16(bad)[idx], ref["y"][idx], e32, ex["y"]["bulk"], True)


# ----------------------------------------------------------------------------------- activations
@pytest.mark.parametrize("rows,F", RB.ACT_SHAPES)
def test_swiglu_reference(rows, F):
    c, planted = RB.swiglu_case(rows, F)
    agree("swiglu", B32.swiglu(**c), RB.swiglu64(**c))
    assert planted.any()


@pytest.mark.parametrize("numel", RB.GELU_NUMEL)
def test_gelu_reference(numel):
    c, planted = RB.gelu_case(numel)
    agree("gelu_new", B32.gelu_new(**c), RB.gelu_new64(**c))
    assert planted.sum() == min(numel, len(RB.PLANTED))


def test_activation_grid_crosses_the_block_cap():
    rows, F = RB.ACT_SHAPES[-1]
    assert (rows * (F // 8) + 255) // 256 == 2048 + 1
    assert (RB.GELU_NUMEL[-1] // 8 + 255) // 256 == 2048 + 1


# ------------------------------------------------------------------------------------------ RoPE
def _rope_inputs(D, rot, Hq, Hkv, kind, B=2, T=24):
    cos, sin = RB.rope_tables(rot)
    c = RB.rope_case(B * T, Hq, Hkv, D)
    kpos, off, pos = RB.rope_positions(kind, B, T)
    qk = c["buf"][:, :(Hq + Hkv) * D].reshape(B * T, Hq + Hkv, D)
    return cos, sin, pos, qk


@pytest.mark.parametrize("kind", ["off0", "off37", "explicit"])
@pytest.mark.parametrize("D,rot", RB.ROPE_DROT)
def test_rope_reference(D, rot, kind):
    cos, sin, pos, qk = _rope_inputs(D, rot, 3, 1, kind)
    for bwd in (False, True):
        agree(f"rope bwd={bwd}", B32.rope(qk, cos, sin, pos, rot, bwd), RB.rope64(qk, cos, sin, pos, rot, bwd))


@pytest.mark.parametrize("D,rot", RB.ROPE_DROT)
def test_rope_adjoint_fp64(D, rot):
    """<rope(x), g> == <x, rope_bwd(g)> on the references."""
    cos, sin, pos, qk = _rope_inputs(D, rot, 4, 2, "explicit")
    g = torch.randn(qk.shape, generator=R.gen(5), dtype=F64)
    lhs = (RB.rope64(qk, cos, sin, pos, rot)["out"] * g).sum()
    rhs = (d(qk) * RB.rope64(g, cos, sin, pos, rot, True)["out"]).sum()
    assert abs(lhs.item() - rhs.item()) <= 1e-12 * (d(qk).abs() * g.abs()).sum().item()


def test_rope_big_case_crosses_the_block_cap():
    b = RB.ROPE_BIG
    assert b["tokens"] * (b["Hq"] + b["Hkv"]) * (b["D"] // 8 - b["rot"] // 16) > 2048 * 256


@pytest.mark.parametrize("defect", ["bwd_sign", "passthrough_unwritten", "next_cos_row"])
def test_defect_rope(defect):
    D, rot = 80, 32
    cos, sin, pos, qk = _rope_inputs(D, rot, 3, 1, "off37")
    ref = RB.rope64(qk, cos, sin, pos, rot)["out"]
    b32 = B32.rope(qk, cos, sin, pos, rot)["out"]
    e32, ex = R.e32_of(b32, ref), RB.rope_extra(qk)
    RB.check("rope", "out/clean", as_bf16(b32), ref, e32, ex, True)
    if defect == "bwd_sign":
        bad = B32.rope(qk, cos, sin, pos, rot, True)["out"]
    elif defect == "passthrough_unwritten":
        bad = b32.clone()
        bad[..., D - 8:] = 0.0  # the last pass-through chunk of every head
    else:
        cos2 = torch.cat([cos[1:], cos[-1:]])
        bad = B32.rope(qk, cos2, sin, pos, rot)["out"]
    rejected("rope", "out", as_bf16(bad), ref, e32, ex, True)


# ------------------------------------------------------------------------------------- embedding
def test_embedding_layout_edges():
    sid, runs = RB.emb_layout("edges")
    x = {i: (p, q, n) for (i, _), (p, q, n) in zip(runs, RB.emb_crossings(runs))}
    assert x[1][0] == 0  # a run starting at p = 0
    assert x[15] == (16, 32, 0)  # 16 from a chunk boundary: one chunk, summed whole in pass 1
    assert x[24] == (40, 56, 1)  # 16 from offset 8: exactly one boundary, two pieces
    assert x[33] == (64, 97, 2) and (97 - 1) % RB.EMB_CHUNK == 0  # 33 from a boundary: last piece of length 1
    assert x[43][2] >= 9
    assert x[44][1] == sid.numel() and x[44][2] == 1  # ends at N and crosses a boundary
    assert sum(1 for _, n in runs if n == 1) >= 30  # singletons
    sid2, runs2 = RB.emb_layout("edges_oob")
    assert sid2[0] < 0 and sid2[-1] >= RB.EMB_V
    assert any(n > 0 for (i, _), (_, _, n) in zip(runs2, RB.emb_crossings(runs2)) if i < 0 or i >= RB.EMB_V)
    for n in (1, 15, 16, 17):
        s, r = RB.emb_layout(f"one{n}")
        assert s.numel() == n and RB.emb_crossings(r)[0][2] == (1 if n == 17 else 0)
    s, r = RB.emb_layout("last_whole")
    assert RB.emb_crossings(r)[1] == (16, 21, 0)


@pytest.mark.parametrize("kind,H,gdtype", RB.EMB_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_embedding_reference(kind, H, gdtype):
    c = RB.emb_case(kind, H, gdtype)
    args = (c["sid"], c["perm"], c["dy"], c["base"], c["V"])
    agree("embed_bwd", B32.embed_bwd(*args), RB.embed_bwd64(*args))


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("defect", ["piece_skipped", "run_at_N_not_whole"])
def test_defect_embedding(defect, gdtype):
    kind = "edges" if defect == "piece_skipped" else "last_whole"
    c = RB.emb_case(kind, 136, gdtype)
    args = (c["sid"], c["perm"], c["dy"], c["base"], c["V"])
    ref, b32 = RB.embed_bwd64(*args)["grad"], B32.embed_bwd(*args)["grad"]
    e32, ex = R.e32_of(b32, ref), RB.embed_extra(*args)
    bf = gdtype == torch.bfloat16
    RB.check("embed_bwd", "grad/clean", b32.to(gdtype), ref, e32, ex, bf)
    bad = b32.clone()
    if defect == "piece_skipped":  # the middle piece [80, 96) of the run of 33 at [64, 97)
        bad[33] -= c["dy"].float()[c["perm"][80:96]].sum(0)
    else:  # the run [16, 21) ends at N inside one chunk: sent to scratch, never folded
        bad[9] = c["base"].float()[9]
    rejected("embed_bwd", "grad", bad.to(gdtype), ref, e32, ex, bf)


# ----------------------------------------------------------------------------------- reward head
def test_keep_mask_hash_properties():
    """The integer hash on the CPU: deterministic, seed- and row-dependent, keep rate 1 - p."""
    a = RB.rh_keep64(1234, 4, 2048, 0.5)
    assert torch.equal(a, RB.rh_keep64(1234, 4, 2048, 0.5)) and not torch.equal(a, RB.rh_keep64(1235, 4, 2048, 0.5))
    assert not torch.equal(a[0], a[1]) and 0.47 < a.float().mean().item() < 0.53
    assert RB.rh_keep64(7, 2, 16, 0.0).all()
    # one value by hand from the comment of rh_keep: row 0, col 0, seed 0 -> splitmix64 of the golden ratio
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & RB._M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & RB._M64
    z ^= z >> 31
    assert z == 0xE220A8397B1DCDAF  # the first output of splitmix64 seeded with 0
    assert bool(RB.rh_keep64(0, 1, 1, 0.5)[0, 0]) == ((z >> 40) / 2 ** 24 >= 0.5)


@pytest.mark.parametrize("pooling", ["last_token", "mean"])
@pytest.mark.parametrize("T,H", sorted({(T, H) for H, T, *_ in RB.RH_CASES}))
def test_reward_head_reference(pooling, T, H):
    """Against the PyTorch head in fp32 without the contract's rounding (dropout off): the two
    differ by the bf16 rounding of the mean-pooled row, half a bf16 ulp <= 2^-8 relative."""
    c = RB.rh_case(4, T, H, pooling)
    ref = RB.reward_head64(c["hidden"], c["last"], c["mask"], c["w"], c["bias"], 0.0, 0, c["ds"])
    keep = torch.ones(4, H, dtype=torch.bool)
    raw = B32.reward_head(c["hidden"], c["last"], c["mask"], c["w"], c["bias"], keep, 1.0, c["ds"], pooled_round=False)
    rel = 2.0 ** -8 + 1e-4 if pooling == "mean" else 1e-4
    agree("reward_head", raw, ref, keys=["pooled", "dhidden"], rel=rel)
    dws = (d(c["ds"]).abs()[:, None] * ref["pooled"].abs()).sum(0).max().item()  # roundings add up over the batch
    assert (d(raw["dw"]) - ref["dw"]).abs().max().item() <= rel * dws
    sc = (d(raw["score"]) - ref["score"]).abs().max().item()
    assert sc <= rel * (ref["pooled"] * d(c["w"])).abs().sum(1).max().item() + 1e-6
    rnd = B32.reward_head(c["hidden"], c["last"], c["mask"], c["w"], c["bias"], keep, 1.0, c["ds"])
    assert ((d(rnd["pooled"]) - ref["pooled"]).abs() <= ref["flip"] + 1e-12).all()  # only rounding flips at ties
    if pooling == "mean":
        assert (ref["dhidden"][1, 1:] == 0).all() if T > 1 else True


@pytest.mark.parametrize("defect", ["mean_over_T", "other_seed_backward"])
def test_defect_reward_head(defect):
    B, T, H, p, seed = 4, 96, 136, 0.5, 1234
    c = RB.rh_case(B, T, H, "mean")
    ref = RB.reward_head64(c["hidden"], None, c["mask"], c["w"], c["bias"], p, seed, c["ds"])
    b32 = B32.reward_head(c["hidden"], None, c["mask"], c["w"], c["bias"], ref["keep"], 2.0, c["ds"])
    if defect == "mean_over_T":
        R.check("reward_head", "pooled/clean", b32["pooled"], ref["pooled"], 0.0, 0.0, True)
        cnt = c["mask"].sum(1).clamp(min=1)
        bad = (b32["pooled"] * (cnt / T)[:, None]).to(RB.BF).float()
        with pytest.raises(AssertionError):  # a whole ulp here: the fp32 mean may round to the other neighbour
            R.check("reward_head", "pooled/defect", bad, ref["pooled"], 0.0, 0.0, True)
        ex = RB.rh_extra(c["hidden"], c["mask"], c["w"], ref) + ref["score_flip"].max().item()
        e32 = R.e32_of(b32["score"], ref["score"])
        RB.check("reward_head", "score/clean", b32["score"], ref["score"], e32, ex)
        rejected("reward_head", "score", bad @ c["w"].float() + c["bias"].float(), ref["score"], e32, ex)
    else:
        other = RB.rh_keep64(seed + 1, B, H, p)
        assert not torch.equal(other, ref["keep"])
        bad = B32.reward_head(c["hidden"], None, c["mask"], c["w"], c["bias"], other, 2.0, c["ds"])["dhidden"]
        e32 = R.e32_of(b32["dhidden"], ref["dhidden"])
        RB.check("reward_head", "dhidden/clean", as_bf16(b32["dhidden"]), ref["dhidden"], e32, 0.0, True)
        rejected("reward_head", "dhidden", as_bf16(bad), ref["dhidden"], e32, 0.0, True)
