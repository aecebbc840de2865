"""Prefix-shared attention on the GPU (the PFX instantiation of attn_fwd_kernel; attn_bwd_kernel /
attn_bwd8_kernel with a seg_end that drops at the prefix end) against the fp64 reference and the
elementwise bound of _attn_ref64.py, on the cases of _attn_prefix_ref64.py.

Per case and backward variant (DLA_ATTN_BWD_WAVES 4 and 8): forward and backward run twice and
must agree bitwise; EVERY element of O, lse2 * ln 2, dQ, dK, dV lies within the bound (nothing
excluded, no term added); a row without a visible key (the left-padding slots) has O == 0,
lse2 == +inf, dQ == 0 and a key no query sees dK == dV == 0. One case runs with
DLA_ATTN_FWD_PERSIST=1: a prefix call must not reach the persistent forward, which knows no
second key range."""
import pytest
import torch

import _attn_prefix_ref64 as PR
import _attn_ref64 as R
from _attn_ref64 import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = PR.cases()


def _run(c, inp):
    from distributed_llm_alignment_amd import ops
    from distributed_llm_alignment_amd.ops.attention import RotaryCache

    B, T, Hq, Hkv, D = c.B, c.Tk, c.Hq, c.Hkv, c.D
    if c.entry == "qkv":
        qkv = torch.cat([inp["q"].reshape(B, T, Hq * D), inp["k"].reshape(B, T, Hkv * D),
                         inp["v"].reshape(B, T, Hkv * D)], -1).requires_grad_()
        rope = RotaryCache(c.rot, max_pos=1024)
        cos, sin = rope.tables(qkv.device)
        assert torch.equal(cos, inp["cos"]) and torch.equal(sin, inp["sin"]), "reference rope tables differ"
        o = ops.qkv_attention(qkv, Hq, Hkv, D, rope, True, 0, None, None, inp["pos"], segs=inp["segs"],
                              prefix=inp["prefix"])
        lse2 = o.grad_fn.saved_tensors[4]
        (dqkv,) = torch.autograd.grad(o, [qkv], inp["do"].reshape(B, T, Hq * D))
        dq, dk, dv = dqkv.split([Hq * D, Hkv * D, Hkv * D], -1)
        return {"o": o.detach().view(B, T, Hq, D), "lse2": lse2, "dq": dq.reshape(B, T, Hq, D),
                "dk": dk.reshape(B, T, Hkv, D), "dv": dv.reshape(B, T, Hkv, D)}
    q, k, v = (inp[x].detach().clone().requires_grad_() for x in ("q", "k", "v"))
    o = ops.attention_core(q, k, v, causal=True, segs=inp["segs"], prefix=inp["prefix"])
    lse2 = o.grad_fn.saved_tensors[4]
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], inp["do"])
    return {"o": o.detach(), "lse2": lse2, "dq": dq, "dk": dk, "dv": dv}


def _check(c, monkeypatch, persist=None):
    from distributed_llm_alignment_amd.ops import _ext
    from distributed_llm_alignment_amd.ops import attention as attn_mod

    _ext.require()
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
    inp_c, r, bnd, num = PR.built(c, torch.cuda.get_device_properties(0).multi_processor_count)
    inp = R.to_device(inp_c, DEV)
    a = _run(c, inp)
    b = _run(c, inp)
    torch.cuda.synchronize()
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        it = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(x.view(it), y.view(it)), f"{c.name}: {k} differs between two runs"
    a = {k: x.cpu() for k, x in a.items()}
    got = {"o": a["o"], "lse": a["lse2"].to(F64) * R.LN2, "dq": a["dq"], "dk": a["dk"], "dv": a["dv"]}
    res = R.ratios(got, r, bnd)
    print(f"FIG attn prefix {c.name} waves{c.bwd[0]} persist={persist} hs{num['hs']} emax {inp_c['emax']:.4f}: {R.fmt(res)}")
    nokey = r["nokey"]
    unseen = ~r["ok"].any(-2).squeeze(1)
    rows = nokey.transpose(1, 2)
    assert (a["o"][rows] == 0).all(), f"{c.name}: O of a row without a visible key is not 0"
    assert (a["lse2"][nokey] == float("inf")).all(), f"{c.name}: lse2 of a row without a visible key is not +inf"
    assert (a["dq"][rows] == 0).all(), f"{c.name}: dQ of a row without a visible key is not 0"
    assert (a["dk"][unseen] == 0).all() and (a["dv"][unseen] == 0).all(), f"{c.name}: dK / dV of an unseen key not 0"
    assert max(res.values()) <= 1.0, f"{c.name}: max error / bound {R.fmt(res)}"


@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_attention_prefix_fp64(c, waves, monkeypatch):
    _check(PR.with_bwd(c, waves), monkeypatch)


def test_attention_prefix_never_persistent(monkeypatch):
    """DLA_ATTN_FWD_PERSIST=1 forces the persistent forward for plain calls; a prefix call must
    still take attn_fwd_kernel (the persistent kernel would drop the prefix keys: the mutation
    `prefix_hidden` of the CPU tests, hundreds of times the bound)."""
    _check(PR.with_bwd(CASES[2], 8), monkeypatch, persist=1)


def test_attention_prefix_argument_checks():
    from distributed_llm_alignment_amd import ops

    c = CASES[0]
    inp = R.to_device(PR.built(c)[0], DEV)
    q, k, v = inp["q"], inp["k"], inp["v"]
    new_check = "prefix needs segs and causal self-attention without a window"
    with pytest.raises(RuntimeError, match=new_check):  # window
        ops.attention_core(q, k, v, causal=True, window=16, segs=inp["segs"], prefix=inp["prefix"])
    with pytest.raises(RuntimeError, match=new_check):  # no segs
        ops.attention_core(q, k, v, causal=True, prefix=inp["prefix"])
    with pytest.raises(RuntimeError, match="prefix must be contiguous int32"):  # [B, 2]
        ops.attention_core(q, k, v, causal=True, segs=inp["segs"], prefix=inp["prefix"][:, :2].contiguous())
    # Tq != Tk (and a non-causal call) cannot carry segs at all: the segs check, which the prefix
    # needs to have passed, refuses them first
    with pytest.raises(RuntimeError, match="packed sequences need causal self-attention"):
        ops.attention_core(q[:, :5].contiguous(), k, v, causal=True, segs=inp["segs"][:, :, :5].contiguous(),
                           prefix=inp["prefix"])
    with pytest.raises(RuntimeError, match="packed sequences need causal self-attention"):
        ops.attention_core(q, k, v, causal=False, segs=inp["segs"], prefix=inp["prefix"])
