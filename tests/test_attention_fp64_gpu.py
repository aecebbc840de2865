"""Training attention forward and backward (csrc/attention.hip) against the fp64 reference and the
derived elementwise bound of _attn_ref64.py, over the covering grid `_attn_ref64.grid()`.

Every case
  * runs forward and backward twice and requires bitwise equal O, lse2, dQ, dK, dV;
  * checks EVERY element of O, lse2 * ln 2, dQ, dK, dV as |kernel - ref64| <= bound (no sampling,
    no excluded rows: the share left out is zero) and reports max error / bound per output;
  * pins the no-visible-key contract: a query row that sees no key has O == 0, lse2 == +inf and
    dQ == 0 exactly; a key that no query sees (outside [kv_start, kv_end), above the causal
    diagonal of a short Tq, in a 256-key block without keys) has dK == 0 and dV == 0 exactly.
    (From the code: the forward's `inv = lsum > 0 ? 1 / lsum : 0` and `lsum > 0 ? m + log2 : +inf`;
    the backward recomputes p = exp2(. - inf) = 0 for such rows -- the 8-wave kernel substitutes
    -1e30 for the non-finite row constant -- so their dS is 0 and the slab rows it writes are 0,
    while attn_dq_reduce_kernel sums an empty block range to 0 for rows no block swept; dK / dV
    accumulators start at 0 and are stored for every key < Tk, also when block_has_keys is
    false.)

Before each backward the scratch the launcher takes with at::empty (dQ slabs, dK / dV head-split
partials, delta, and the gradient outputs) is made visibly stale: tensors of those sizes are
filled with NaN and freed, so that the caching allocator hands the same blocks out again. This is
best effort (the allocator may choose other blocks; on the MI355X a torch.empty of the same shape
right after such a free came back all NaN); where it takes, a reduce pass that reads a row no
workgroup wrote yields NaN instead of a plausible earlier gradient.

Measured on an MI355X, worst error / bound over the grid (the CPU emulation of
test_attention_ref_cpu.py: o 0.50, lse 0.92, dq 0.43, dk 0.09, dv 0.78):
    4 waves                     o 0.50  lse 0.92  dq 0.39  dk 0.09  dv 0.78
    8 waves, fp32 slab / part   o 0.46  lse 0.92  dq 0.43  dk 0.05  dv 0.78
    8 waves, bf16 partials      o 0.46  lse 0.92  dq 0.36  dk 0.07  dv 0.65
    8 waves, bf16 slabs         o 0.45  lse 0.92  dq 0.29  dk 0.09  dv 0.61
    8 waves, both (default)     o 0.46  lse 0.92  dq 0.34  dk 0.07  dv 0.69
(the variants run different cases of the grid, so the rows differ by case, not only by variant).
No kernel exceeded the bound and no contract was violated: no bug found.
"""
import pytest
import torch

import _attn_ref64 as R
from _attn_ref64 import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = R.grid()


def _poison(c, num):
    """NaN-filled tensors of the backward's scratch sizes, freed at once (see the module docstring)."""
    slab_rows = (c.Tq + 31) // 32 * 32
    sdt = torch.bfloat16 if num["slab16"] else torch.float32
    pdt = torch.bfloat16 if num["part16"] else torch.float32
    junk = [torch.full((max(num["nkb"], 1), c.B, slab_rows, c.Hq, c.D), float("nan"), dtype=sdt, device=DEV),
            torch.full((c.B, c.Hq, c.Tq), float("nan"), dtype=torch.float32, device=DEV),
            torch.full((c.B, c.Tq, c.Hq, c.D), float("nan"), dtype=torch.bfloat16, device=DEV)]
    if num["hs"] > 1:
        junk += [torch.full((num["hs"], c.B, c.Tk, c.Hkv, c.D), float("nan"), dtype=pdt, device=DEV) for _ in range(2)]
    junk += [torch.full((c.B, c.Tk, c.Hkv, c.D), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    if c.entry == "qkv":
        junk.append(torch.full((c.B, c.Tk, (c.Hq + 2 * c.Hkv) * c.D), float("nan"), dtype=torch.bfloat16, device=DEV))
    del junk


def _run(c, inp, num):
    """One forward + backward through the case's entry point -> o, lse2, dq, dk, dv."""
    from distributed_llm_alignment_amd import ops
    from distributed_llm_alignment_amd.ops.attention import RotaryCache

    B, Tq, Tk, Hq, Hkv, D = c.B, c.Tq, c.Tk, c.Hq, c.Hkv, c.D
    do = inp["do"]
    if c.layout == "do_nc":
        do = inp["do"].transpose(1, 2).contiguous().transpose(1, 2)
        assert not do.is_contiguous()
    if c.entry == "qkv":
        qkv = torch.cat([inp["q"].reshape(B, Tq, Hq * D), inp["k"].reshape(B, Tk, Hkv * D),
                         inp["v"].reshape(B, Tk, Hkv * D)], -1).requires_grad_()
        rope = None
        if c.rot:
            rope = RotaryCache(c.rot, max_pos=1024)
            cos, sin = rope.tables(qkv.device)
            assert torch.equal(cos, inp["cos"]) and torch.equal(sin, inp["sin"]), "reference rope tables differ"
        positions = inp["pos"] if c.pos == "leftpad" else None
        o = ops.qkv_attention(qkv, Hq, Hkv, D, rope, c.causal, c.window, inp["kv_start"], inp["kv_end"], positions,
                              segs=inp["segs"])
        lse2 = o.grad_fn.saved_tensors[4]
        _poison(c, num)
        (dqkv,) = torch.autograd.grad(o, [qkv], do.reshape(B, Tq, Hq * D))
        dq, dk, dv = dqkv.split([Hq * D, Hkv * D, Hkv * D], -1)
        return {"o": o.detach().view(B, Tq, Hq, D), "lse2": lse2, "dq": dq.reshape(B, Tq, Hq, D),
                "dk": dk.reshape(B, Tk, Hkv, D), "dv": dv.reshape(B, Tk, Hkv, D)}
    if c.layout == "qkvview":  # q / k / v as column views of one fused buffer (strided rows)
        buf = torch.cat([inp["q"].reshape(B, Tq, Hq * D), inp["k"].reshape(B, Tk, Hkv * D),
                         inp["v"].reshape(B, Tk, Hkv * D)], -1)
        q, k, v = (t.reshape(B, Tk, -1, D).detach().requires_grad_() for t in buf.split([Hq * D, Hkv * D, Hkv * D], -1))
        assert not q.is_contiguous() and q.stride(-1) == 1
    else:
        q, k, v = (inp[x].detach().clone().requires_grad_() for x in ("q", "k", "v"))
    o = ops.attention_core(q, k, v, causal=c.causal, causal_off=None if c.mask != "cross0" else 0, window=c.window,
                           kv_start=inp["kv_start"], kv_end=inp["kv_end"], segs=inp["segs"])
    lse2 = o.grad_fn.saved_tensors[4]
    _poison(c, num)
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], do)
    return {"o": o.detach(), "lse2": lse2, "dq": dq, "dk": dk, "dv": dv}


WORST = {}


@pytest.mark.parametrize("c", GRID, ids=lambda c: c.name)
def test_attention_fp64(c, monkeypatch):
    from distributed_llm_alignment_amd.ops import _ext
    from distributed_llm_alignment_amd.ops import attention as attn_mod

    C = _ext.require()
    persist, msub, ostage = c.fwd
    if persist is None:
        monkeypatch.delenv("DLA_ATTN_FWD_PERSIST", raising=False)
    else:
        monkeypatch.setenv("DLA_ATTN_FWD_PERSIST", str(persist))
    monkeypatch.setenv("DLA_ATTN_BWD_WAVES", str(c.bwd[0]))
    monkeypatch.setenv("DLA_ATTN_DQ_BF16", str(c.bwd[1]))
    monkeypatch.setenv("DLA_ATTN_DKV_BF16", str(c.bwd[2]))
    monkeypatch.setattr(attn_mod, "ROPE_Q_ON_LOAD", bool(c.ropesw[0]))
    monkeypatch.setattr(attn_mod, "FUSED_ROPE_BWD", bool(c.ropesw[1]))
    monkeypatch.setattr(attn_mod, "FUSED_ROPE_FWD", bool(c.ropesw[2]))
    num = c.numerics(torch.cuda.get_device_properties(0).multi_processor_count)
    inp = R.to_device(R.build(c), DEV)
    prev_m = C.attn_fwd_switch("msub", int(msub))
    prev_o = C.attn_fwd_switch("ostage", int(ostage))
    try:
        a = _run(c, inp, num)
        b = _run(c, inp, num)
        torch.cuda.synchronize()
    finally:
        C.attn_fwd_switch("msub", prev_m)
        C.attn_fwd_switch("ostage", prev_o)
    for k in a:  # bitwise (NaN-safe: compare the bit patterns)
        x, y = a[k].contiguous(), b[k].contiguous()
        it = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(x.view(it), y.view(it)), f"{c.name}: {k} differs between two runs"
    r = R.reference(inp, c)
    bnd = R.bounds(inp, c, r, num)
    got = {"o": a["o"], "lse": a["lse2"].to(F64) * R.LN2, "dq": a["dq"], "dk": a["dk"], "dv": a["dv"]}
    res = R.ratios(got, r, bnd)
    print(f"FIG attn {c.name} bwd{c.bwd} hs{num['hs']} emax {inp['emax']:.4f}: {R.fmt(res)}")
    key = "waves%d dq16=%d dkv16=%d" % c.bwd if c.bwd[0] == 8 else "waves4"
    for k, x in res.items():
        w = WORST.setdefault(key, {})
        w[k] = max(w.get(k, 0.0), x)
    # the no-visible-key contract, stated on its own (the bound is 0 there, so it is also part of
    # the elementwise check below)
    nokey = r["nokey"]  # [B, Hq, Tq]
    unseen = ~r["ok"].any(-2).squeeze(1)  # [B, Tk]: keys no query sees
    rows = nokey.transpose(1, 2)  # [B, Tq, Hq]
    assert (a["o"][rows] == 0).all(), f"{c.name}: O of a row without a visible key is not 0"
    assert (a["lse2"][nokey] == float("inf")).all(), f"{c.name}: lse2 of a row without a visible key is not +inf"
    assert (a["dq"][rows] == 0).all(), f"{c.name}: dQ of a row without a visible key is not 0"
    assert (a["dk"][unseen] == 0).all() and (a["dv"][unseen] == 0).all(), f"{c.name}: dK / dV of an unseen key not 0"
    assert max(res.values()) <= 1.0, f"{c.name}: max error / bound {R.fmt(res)}"


def test_attention_fp64_report():
    """Prints the worst error / bound per backward variant over the cases that ran before it."""
    for key in sorted(WORST):
        print(f"FIG attn worst {key}: {R.fmt(WORST[key])}")
