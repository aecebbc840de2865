"""The attention checker of _attn_ref64.py proved without a GPU.

`emulate` is a torch emulation of the kernels' arithmetic with exactly the rounding points of the
bound's derivation (bf16 scaled Q, fp32 lsum against bf16 P, bf16 O feeding delta, p recomputed
from the unscaled Q against the forward's lse2, bf16 P and dS, a bf16 slab per 256 keys, a bf16
partial per head split, bf16 outputs; the rope-kernel roundings of the fused-QKV path). The tile
order is not the kernels' (sums run in fp64 between the rounding points).

  * the emulation is inside the bound on every case of the GPU grid, both families
    (worst error / bound over the grid: o 0.50, lse 0.92, dq 0.43, dk 0.09, dv 0.78; the LSE
    of a row with one visible key is a single rounding of q * scale2, so it comes close to 1);
  * the fp32 `ref_attention` + autograd agrees with the fp64 closed forms on cases whose rows
    all see a key;
  * every mutant of MUTANTS is rejected by a sentinel (peaked) case with error / bound >= 4.
"""
import math

import pytest
import torch

import _attn_ref64 as R
from _attn_ref64 import F64

GRID = R.grid()
_CACHE = {}


def prepared(c):
    """(inputs, numerics, fp64 reference, bounds) of a case, computed once per process."""
    if c.name not in _CACHE:
        if len(_CACHE) > 6:
            _CACHE.pop(next(iter(_CACHE)))
        inp = R.build(c)
        num = c.numerics()
        r = R.reference(inp, c)
        _CACHE[c.name] = (inp, num, r, R.bounds(inp, c, r, num))
    return _CACHE[c.name]


def bf(x):
    return x.float().bfloat16().to(F64)


def f32(x):
    return x.float().to(F64)


def emulate(inp, c, num, mut=None):
    q, k, v, do = (inp[x].to(F64).transpose(1, 2) for x in ("q", "k", "v", "do"))
    B, Hq, Hkv, Tq, Tk, D = c.B, c.Hq, c.Hkv, c.Tq, c.Tk, c.D
    scale = float(torch.tensor(c.scale, dtype=torch.float32))
    scale2 = float(torch.tensor(c.scale * R.LOG2E, dtype=torch.float32))
    cos, sin, pos = inp["cos"], inp["sin"], inp["pos"]
    if c.rot:
        kpos = torch.arange(Tk).expand(B, Tk) if mut == "rope_pos_t" else pos
        qr32 = f32(R.rope(q, cos, sin, pos, c.rot))
        q_rot = bf(qr32)  # rope.hip, or the forward's q_rot side output
        qs = bf(f32((q_rot if num["nf"] == 3 else qr32) * scale2))
        kr = bf(R.rope(k, cos, sin, kpos, c.rot))
    else:
        q_rot, qs, kr = q, bf(f32(q * scale2)), k
    hm = R.head_map(c, q.device, mut)
    ke, ve = kr[:, hm], v[:, hm]
    ok = R.visibility(c, inp, mut).unsqueeze(1)
    # ---- forward: exp2-domain scores from the scaled bf16 Q, fp32 lsum, bf16 P into P.V
    s2 = f32(qs @ ke.transpose(-1, -2)).masked_fill(~ok, float("-inf"))
    m = s2.amax(-1, keepdim=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = f32(torch.exp2(s2 - m0))
    lsum = f32(p.sum(-1, keepdim=True))
    acc = f32(bf(p) @ ve)
    inv = torch.where(lsum > 0, 1.0 / lsum.clamp(min=1e-300), torch.zeros_like(lsum))
    O = bf(f32(acc * inv))
    lse2 = torch.where(lsum > 0, f32(m0 + torch.log2(lsum.clamp(min=1e-300))), torch.full_like(lsum, float("inf")))
    if mut == "nokey_mean_v":
        O = torch.where(lsum > 0, O, bf(ve.mean(-2, keepdim=True)).expand_as(O))
    # ---- backward: p from the unscaled Q and the forward's lse2; delta from the bf16 O
    x = f32(f32(q_rot @ ke.transpose(-1, -2)) * scale2 - lse2)
    pr = torch.where(ok, f32(torch.exp2(x)), torch.zeros_like(x))
    delta = f32((do * (acc if mut == "delta_unnorm" else O)).sum(-1, keepdim=True))
    dP = f32(do @ ve.transpose(-1, -2))
    dS = bf(f32(pr * (dP - delta)))
    Pb = bf(pr)
    dQr = torch.zeros(B, Hq, Tq, D, dtype=F64)
    for kb in range(num["nkb"]):
        if mut == "skip_slab" and kb == num["nkb"] - 1:
            continue
        sl = slice(kb * R.BWD_KEYS, min((kb + 1) * R.BWD_KEYS, Tk))
        slab = f32((dS[..., sl] @ ke[:, :, sl]) * (1.0 if mut == "no_scale_dq" else scale))
        dQr = dQr + (bf(slab) if num["slab16"] else slab)
    group, hs = Hq // Hkv, num["hs"]
    hpb = group // hs
    dKr = torch.zeros(B, Hkv, Tk, D, dtype=F64)
    dV = torch.zeros(B, Hkv, Tk, D, dtype=F64)
    ck = dS.transpose(-1, -2) @ q_rot
    cv = Pb.transpose(-1, -2) @ do
    for s in range(hs):
        if mut == "skip_part" and s == hs - 1:
            continue
        heads = torch.tensor([h for h in range(Hq) if (h % group) // hpb == s])
        pk = f32(torch.zeros_like(dKr).index_add_(1, hm[heads], ck[:, heads]))
        pv = f32(torch.zeros_like(dV).index_add_(1, hm[heads], cv[:, heads]))
        dKr = dKr + (bf(pk) if num["part16"] else pk)
        dV = dV + (bf(pv) if num["part16"] else pv)
    dKr = f32(dKr * (1.0 if mut == "no_scale_dk" else scale))
    dq, dk = dQr, dKr
    if c.rot:
        if num["extra_round"]:
            dq, dk = bf(dq), bf(dk)
        sign = -1.0 if mut == "unrotate_sign" else 1.0
        dq = R.rope(dq, cos, sin, pos, c.rot, inverse=True, sign=sign)
        dk = R.rope(dk, cos, sin, pos, c.rot, inverse=True, sign=sign)
    return {"o": O.transpose(1, 2), "lse": lse2.squeeze(-1) * R.LN2, "dq": bf(dq).transpose(1, 2),
            "dk": bf(dk).transpose(1, 2), "dv": bf(dV).transpose(1, 2)}


WORST = {}


@pytest.mark.parametrize("c", GRID, ids=lambda c: c.name)
def test_emulation_within_bound(c):
    inp, num, r, bnd = prepared(c)
    assert inp["emax"] <= R.EMAX
    res = R.ratios(emulate(inp, c, num), r, bnd)
    print(f"FIG emu {c.name} bwd{c.bwd} emax {inp['emax']:.4f} shrink {inp['shrink']:.3f}: {R.fmt(res)}")
    for k, x in res.items():
        WORST[k] = max(WORST.get(k, 0.0), x)
    assert max(res.values()) <= 1.0, f"{c.name}: emulation outside the bound: {R.fmt(res)}"


def test_grid_covers_every_axis():
    """Every value of every axis with both families; every mask kind against every forward and
    backward variant at a key length past 512."""
    for fam in R.FAMS:
        cs = [c for c in GRID if c.fam == fam]
        assert {c.Tk for c in cs} >= set(R.T_AXIS)
        assert {c.D for c in cs} == {64, 80, 128}
        assert {(c.Hq, c.Hkv) for c in cs} == set(R.HEADS)
        assert {c.mask for c in cs} == set(R.MASKS)
        assert {c.entry for c in cs} == {"core", "qkv"} and {c.layout for c in cs} == {"contig", "qkvview", "do_nc"}
        assert {c.bwd for c in cs} >= set(R.BWD_VARIANTS) and {c.fwd for c in cs} >= set(R.FWD_VARIANTS)
        assert {(c.D, c.rot, c.ropesw, c.pos) for c in cs if c.rot} >= {
            (D, D, sw, p) for D in (64, 128) for sw in [(1, 1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 0), (1, 1, 1)]
            for p in ("default", "leftpad")} | {(80, 32, sw, p) for sw in [(1, 1, 0), (1, 0, 0)] for p in ("default", "leftpad")}
    big = [c for c in GRID if c.Tk > 512 and c.D == 128]
    for mask in R.MASKS:
        assert {c.fwd for c in big if c.mask == mask} >= set(R.FWD_VARIANTS), mask
        assert {c.bwd for c in big if c.mask == mask} >= set(R.BWD_VARIANTS), mask
    assert 150 <= len(GRID) <= 250


def _no_empty_rows(c):
    return c.mask in ("causal", "full", "win1", "win48", "win300", "segs", "cross", "cross0") and c.Tk <= 300


@pytest.mark.parametrize("c", [c for c in GRID if _no_empty_rows(c)][::4], ids=lambda c: c.name)
def test_fp64_closed_forms_match_fp32_autograd(c):
    """Ties the new reference to the one on record: ops.attention.ref_attention (+ _ref_rope) in
    fp32 with autograd, on cases where every query row sees a key (autograd through the
    nan_to_num of an all-masked row is not defined)."""
    from distributed_llm_alignment_amd.ops.attention import _ref_rope, ref_attention

    inp, num, r, _ = prepared(c)
    assert not r["nokey"].any()
    q, k, v = (inp[x].float().requires_grad_() for x in ("q", "k", "v"))
    qq, kk = q, k
    if c.rot:
        qq = _ref_rope(q, inp["cos"], inp["sin"], inp["pos"], c.rot)
        kk = _ref_rope(k, inp["cos"], inp["sin"], inp["pos"], c.rot)
    o = ref_attention(qq, kk, v, c.scale, c.causal, c.causal_off, c.window, inp["kv_start"], inp["kv_end"], inp["segs"])
    gq, gk, gv = torch.autograd.grad(o, [q, k, v], inp["do"].float())
    for name, got in (("o", o), ("dq", gq), ("dk", gk), ("dv", gv)):
        ref = r[name]
        tol = 64 * R.EPS32 * ref.abs().max().item() * math.sqrt(c.Tk)
        err = (got.detach().to(F64) - ref).abs().max().item()
        assert err <= tol, f"{c.name}/{name}: fp32 autograd vs fp64 closed form {err:.3e} > {tol:.3e}"


def _has_empty_row(c):
    return c.mask == "rpad" or (c.mask == "lpad" and c.Tk == 1)


MUTANTS = {
    "causal_lt": lambda c: c.causal and c.window == 0,
    "causal_plus1": lambda c: c.causal and c.window == 0,
    "window_lo_plus1": lambda c: c.window == 48,
    "window_lo_minus1": lambda c: c.window == 48,
    "kv_end_plus1": lambda c: c.mask == "rpad",
    "kv_end_minus1": lambda c: c.mask == "rpad",
    "kv_start_plus1": lambda c: c.mask == "lpad" and c.Tk > 1,
    "kv_start_minus1": lambda c: c.mask == "lpad" and c.Tk > 1,
    "seg_start_plus1": lambda c: c.mask == "segs",
    "seg_start_minus1": lambda c: c.mask == "segs",
    "drop_tail_tile": lambda c: c.Tk % 64 != 0 and c.mask in ("causal", "full"),
    "gqa_mod": lambda c: c.Hkv > 1 and c.Hq > c.Hkv,
    "no_scale_dk": lambda c: True,
    "no_scale_dq": lambda c: True,
    "delta_unnorm": lambda c: True,
    "skip_slab": lambda c: c.Tk > 256 and c.Tq == c.Tk,
    "skip_part": lambda c: c.numerics()["hs"] > 1,
    "rope_pos_t": lambda c: c.pos == "leftpad",
    "unrotate_sign": lambda c: c.rot > 0,
    "nokey_mean_v": _has_empty_row,
}
SURVIVORS = []


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_mutant_rejected(mut):
    """At least one sentinel case fails the check under the mutant, with error / bound >= 4."""
    cands = sorted((c for c in GRID if c.fam == "peaked" and MUTANTS[mut](c)), key=lambda c: (c.Tk < 31, c.Tk * c.Tq * c.Hq))[:3]
    assert cands, f"no sentinel case exercises {mut}"
    best = 0.0
    for c in cands:
        inp, num, r, bnd = prepared(c)
        res = R.ratios(emulate(inp, c, num, mut), r, bnd)
        print(f"FIG mutant {mut} on {c.name}: {R.fmt(res)}")
        best = max(best, max(res.values()))
        if best >= 4.0:
            break
    if best < 4.0:
        SURVIVORS.append(mut)
    assert best >= 4.0, f"mutant {mut} survives: worst error / bound {best:.2f} on {[c.name for c in cands]}"
