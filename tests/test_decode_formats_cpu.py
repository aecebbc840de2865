"""The quantised decode weight formats of ops/decode.py (fp8, mxfp4) as one table, on CPU: the scope
state, the cached copy builder and its attribute names, and the derived-weight bookkeeping built
on the table (DERIVED_ATTRS, refresh_folded_weights, drop_derived_weights)."""
import pytest
import torch

from distributed_llm_alignment_amd.models import build_model, get_config
from distributed_llm_alignment_amd.ops import decode as D

FORMATS = ["fp8", "mxfp4"]
SCOPE = {"fp8": D.fp8_weights, "mxfp4": D.mxfp4_weights}
ENABLED = {"fp8": D.fp8_enabled, "mxfp4": D.mxfp4_enabled}
BUILD = {"fp8": D.fp8_tiled_weight, "mxfp4": D.mxfp4_tiled_weight}
ATTRS = {"fp8": ("_dla_f8", "_dla_f8_n", "_dla_f8_g"), "mxfp4": ("_dla_f4", "_dla_f4_n", "_dla_f4_g")}


def _formula(name, src):
    if name == "fp8":
        q, sc = D.quantize_rows_f8(src)
        return D.tile_f8(q), sc
    return D.tile_mxfp4(*D.quantize_mxfp4(src))


def _state():
    return D.fp8_enabled(), D.mxfp4_enabled()


@pytest.mark.parametrize("name", FORMATS)
def test_scope_truth_table(name):
    other = FORMATS[1 - FORMATS.index(name)]
    assert _state() == (False, False)
    with SCOPE[name](True):
        assert ENABLED[name]() and not ENABLED[other]()
        with SCOPE[name](False):
            assert _state() == (False, False)
            with SCOPE[other](True):  # the other format may enter once this one is off
                assert ENABLED[other]() and not ENABLED[name]()
            assert _state() == (False, False)
        with SCOPE[other](False):  # turns off the other format only
            assert ENABLED[name]() and not ENABLED[other]()
        with SCOPE[name](True):
            assert ENABLED[name]()
        assert ENABLED[name]() and not ENABLED[other]()
        with pytest.raises(RuntimeError):
            SCOPE[other](True).__enter__()
        assert ENABLED[name]() and not ENABLED[other]()  # the refused scope moved nothing
    assert _state() == (False, False)
    with SCOPE[other](True), pytest.raises(RuntimeError):
        SCOPE[name](True).__enter__()
    assert _state() == (False, False)
    with pytest.raises(KeyError):
        with SCOPE[name](True):
            with SCOPE[name](False):
                raise KeyError("inside the block")
    assert _state() == (False, False)
    # the scope generate() enters: the named format whatever is active outside, None = the bf16 weights
    with SCOPE[other](True):
        with D.weight_format(name):
            assert ENABLED[name]() and not ENABLED[other]()
            with D.weight_format(None):
                assert _state() == (False, False)
        assert ENABLED[other]() and not ENABLED[name]()
    assert _state() == (False, False)


def test_mxfp4_scope_marks_the_model_for_the_block():
    m = build_model(get_config("tiny-llama-d128", num_layers=2), device="cpu", dtype=torch.float32, seed=0)
    marked = [m.lm_head] + [w for l in m.layers for w in (l.attn.qkv_proj, l.attn.o_proj, l.mlp.up_proj,
                                                          l.mlp.down_proj)]
    for scope in (lambda: D.mxfp4_weights(True, m), lambda: D.weight_format("mxfp4", m)):
        with scope():
            assert all(getattr(w, "_dla_mx", False) for w in marked)
            assert not hasattr(m.layers[0].ln1_w, "_dla_mx")
        assert not any(hasattr(p, "_dla_mx") for p in m.parameters())
    for scope in (lambda: D.mxfp4_weights(False, m), lambda: D.weight_format("fp8", m), lambda: D.weight_format(None, m)):
        with scope():
            assert not any(hasattr(p, "_dla_mx") for p in m.parameters())


@pytest.mark.parametrize("name", FORMATS)
def test_builder_attributes_and_in_place_refresh(name):
    g = torch.Generator().manual_seed(0)
    w = torch.randn(32, 128, generator=g).to(torch.bfloat16)
    nw = (1 + 0.2 * torch.randn(128, generator=g)).to(torch.bfloat16)
    forms = [(dict(), lambda: w), (dict(norm_w=nw), lambda: w * nw.view(1, -1)),
             (dict(norm_w=nw, glu_il=True), lambda: D._glu_interleave(w * nw.view(1, -1)))]
    held = []
    for (kw, src), attr in zip(forms, ATTRS[name]):
        pair = BUILD[name](w, **kw)
        assert getattr(w, attr)[1] is pair and BUILD[name](w, **kw) is pair  # cached under its attribute
        ref = _formula(name, src())
        assert all(torch.equal(t, r) and t.dtype == r.dtype for t, r in zip(pair, ref))
        held.append((pair, [t.data_ptr() for t in pair]))
    assert sorted(k for k in w.__dict__ if k.startswith("_dla")) == sorted(ATTRS[name])
    with torch.no_grad():
        w.add_(1)
    for (kw, src), (pair, ptrs) in zip(forms, held):
        before = [t.clone() for t in pair]
        again = BUILD[name](w, **kw)
        assert again is pair and [t.data_ptr() for t in again] == ptrs  # refreshed in place
        ref = _formula(name, src())
        assert all(torch.equal(t, r) for t, r in zip(again, ref))
        assert not torch.equal(again[0], before[0])


def test_derived_attrs_are_the_names_in_use():
    assert set(D.DERIVED_ATTRS) == {"_dla_fold", "_dla_fold_t", "_dla_fold_g", "_dla_tile", "_dla_f8", "_dla_f8_n",
                                    "_dla_f8_g", "_dla_f4", "_dla_f4_n", "_dla_f4_g", "_dla_f4_ref", "_dla_fp8"}
    assert len(D.DERIVED_ATTRS) == 12


@pytest.mark.parametrize("name", FORMATS)
def test_refresh_touches_the_copies_that_exist_and_drop_frees_them(name):
    cfg = get_config("tiny-llama-d128", num_layers=2)
    m = build_model(cfg, device="cpu", dtype=torch.bfloat16, seed=0).eval()
    l0, l1 = m.layers
    plain, folded, il = ATTRS[name]
    made = {(l0.attn.o_proj, plain): BUILD[name](l0.attn.o_proj),
            (l1.attn.qkv_proj, folded): BUILD[name](l1.attn.qkv_proj, l1.ln1_w),
            (l1.mlp.up_proj, il): BUILD[name](l1.mlp.up_proj, l1.ln2_w, glu_il=True),
            (m.lm_head, plain): BUILD[name](m.lm_head)}
    ptrs = {k: [t.data_ptr() for t in v] for k, v in made.items()}

    def held():
        return {(p, k) for p in m.parameters() for k in D.DERIVED_ATTRS if k in p.__dict__}

    assert held() == set(made)
    before = {k: [t.clone() for t in v] for k, v in made.items()}
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
        l1.ln1_w.add_(0.25)
    D.refresh_folded_weights(m)
    assert held() == set(made)  # nothing new was built
    for (w, attr), pair in made.items():
        assert getattr(w, attr)[1] is pair and [t.data_ptr() for t in pair] == ptrs[(w, attr)]
        assert not torch.equal(pair[0], before[(w, attr)][0]) or not torch.equal(pair[1], before[(w, attr)][1])
    ref = _formula(name, l1.attn.qkv_proj.detach() * l1.ln1_w.detach().view(1, -1))
    assert all(torch.equal(t, r) for t, r in zip(made[(l1.attn.qkv_proj, folded)], ref))
    nbytes = sum(t.numel() * t.element_size() for pair in made.values() for t in pair)
    assert D.drop_derived_weights(m) == nbytes
    assert held() == set() and D.drop_derived_weights(m) == 0
