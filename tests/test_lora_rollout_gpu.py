"""LoRA-merged decode weights on the GPU: the one-pass merge kernels (csrc/skinny64.hip
lora_tile_weight_kernel / lora_quant_tile_f8_kernel) and `generate(..., adapters="merged")`.

Ops. Every launch runs twice and the bits must be equal. References:
  * exact integers (`_refs64_lora_rollout.exact_case`): m built on the CPU from fp64; the new ops
    must equal the existing `tile_weight(m, nw, glu_il)` / `quant_tile_f8(m, nw, glu_il)` bit for bit.
  * random: the un-tiled `nw = None` output against fp64 w + s b a with `_refs64.check(bf16=True)`,
    extra = |s| gamma_r max sum_j |b||a| (r terms summed in another order), derived, not measured;
    then that m through the existing ops against the new ops with nw / glu_il, bit for bit.
The existing ops take `glu_il` at N % 32 == 0 only; at N = 16, 48 with `glu_il` the reference is the
package's torch tiling of record (`ops.decode._tile_into`'s CPU branch: interleave, reshape, permute).
The existing `quant_tile_f8` op takes N % 32 == 0 only. At N = 16, 48 its reference is built from
it all the same where the layout allows: without `glu_il` a tile depends on its own 16 rows only, so
the op runs on m padded with 16 zero rows and the first N / 16 tiles and N scales are compared; with
`glu_il` (the padding would move the gate / up split) the reference is the package's torch
formula of record, `quantize_rows_f8` + `tile_f8` on the interleaved rows.

End to end on the tiny d128 model (3 layers, hidden 1024), r = 16, 5 and 24 decode rows (the
<= 16-row and the 17..64-row kernels), 8 new tokens. `g_on` of
`test_merged_decode_computes_the_adapted_function` is a measurement (printed, recorded in
profiles/lora_rollout.md); the gate is relative: g_on < g_off / 10.
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd.ops import _ext
from distributed_llm_alignment_amd.ops import decode as D

import _refs64 as R
import _refs64_lora as RL
import _refs64_lora_rollout as RR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
RANKS = [8, 16, 32, 64]
NS = [16, 48, 160]
KS_F8 = [64, 192, 1088]
KS_BF16 = [32, 64, 96, 192, 1088]
SCALES = [2.0, 0.5]
WORST = {"ratio": 0.0}


def _dev(t):
    return None if t is None else t.to(DEV)


def _glu_ok(N):
    return (N // 2) % 8 == 0


# ------------------------------------------------------------------------------ op drivers
def _tile2(w, a, b, scale, nw, glu_il):
    N, K = w.shape
    outs = []
    for _ in range(2):
        out = torch.full((N // 16, K // 32, 4, 16, 8), float("nan"), dtype=BF16, device=DEV)
        torch.ops.dla.lora_tile_weight(w, a, b, float(scale), nw, out, glu_il)
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two launches differ"
    return outs[0]


def _quant2(w, a, b, scale, nw, glu_il):
    N, K = w.shape
    outs = []
    for _ in range(2):
        o8 = torch.full((N // 16, K // 64, 64, 16), 0x7F, dtype=torch.uint8, device=DEV)
        sc = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
        torch.ops.dla.lora_quant_tile_f8(w, a, b, float(scale), nw, o8, sc, glu_il)
        outs.append((o8, sc))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(torch.int32),
                                                               outs[1][1].view(torch.int32)), "two launches differ"
    return outs[0]


def _ref_tile(m, nw, glu_il):
    N, K = m.shape
    if glu_il and N % 32:  # the existing op refuses it: the package's torch tiling of record
        src = D._glu_interleave(m if nw is None else m * nw.view(1, -1))
        return src.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
    out = torch.empty((N // 16, K // 32, 4, 16, 8), dtype=BF16, device=DEV)
    torch.ops.dla.tile_weight(m, nw, out, glu_il)
    return out


def _ref_quant(m, nw, glu_il):
    """The existing op's (bytes, scales) of m (see the module docstring for N % 32 != 0)."""
    N, K = m.shape
    if N % 32 == 0:
        o8 = torch.empty((N // 16, K // 64, 64, 16), dtype=torch.uint8, device=DEV)
        sc = torch.empty(N, dtype=torch.float32, device=DEV)
        torch.ops.dla.quant_tile_f8(m, nw, o8, sc, glu_il)
        return o8, sc
    if not glu_il:
        mp = torch.cat([m, torch.zeros((16, K), dtype=m.dtype, device=DEV)])
        o8 = torch.empty(((N + 16) // 16, K // 64, 64, 16), dtype=torch.uint8, device=DEV)
        sc = torch.empty(N + 16, dtype=torch.float32, device=DEV)
        torch.ops.dla.quant_tile_f8(mp, nw, o8, sc, False)
        return o8[: N // 16].contiguous(), sc[:N].contiguous()
    # on the CPU: true fp32 divisions, as in the kernels (the GPU's div-by-scalar multiplies by 1 / 448)
    mc, nc = m.cpu(), (None if nw is None else nw.cpu())
    src = mc if nc is None else mc * nc.view(1, -1)
    q, sc = D.quantize_rows_f8(D._glu_interleave(src))
    return D.tile_f8(q).to(DEV), sc.to(DEV)


def _same_tile(got, ref, what):
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), what


def _same_quant(got, ref, what):
    assert torch.equal(got[0], ref[0]), what + ": e4m3 bytes"
    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), what + ": scales"


# ------------------------------------------------------------------------------ exact integers
@pytest.mark.parametrize("R_", RANKS)
def test_tile_exact_integers(R_):
    _ext.require()
    for N in NS:
        for K in KS_BF16:
            for with_nw in (False, True):
                w, a, b, nw = RR.exact_case(N, K, R_, seed=N + K, with_nw=with_nw)
                wd, ad, bd, nwd = _dev(w), _dev(a), _dev(b), _dev(nw)
                for scale in SCALES:
                    m = RR.merged64(w, a, b, scale).to(BF16).to(DEV)
                    for glu_il in (False, True):
                        if glu_il and not _glu_ok(N):
                            continue
                        got = _tile2(wd, ad, bd, scale, nwd, glu_il)
                        _same_tile(got, _ref_tile(m, nwd, glu_il),
                                   f"lora_tile_weight N={N} K={K} R={R_} s={scale} nw={with_nw} glu_il={glu_il}")


@pytest.mark.parametrize("R_", RANKS)
def test_quant_exact_integers(R_):
    _ext.require()
    for N in NS:
        for K in KS_F8:
            for with_nw in (False, True):
                w, a, b, nw = RR.exact_case(N, K, R_, seed=N + K + 1, with_nw=with_nw)
                wd, ad, bd, nwd = _dev(w), _dev(a), _dev(b), _dev(nw)
                for scale in SCALES:
                    m = RR.merged64(w, a, b, scale).to(BF16).to(DEV)
                    for glu_il in (False, True):
                        if glu_il and not _glu_ok(N):
                            continue
                        got = _quant2(wd, ad, bd, scale, nwd, glu_il)
                        _same_quant(got, _ref_quant(m, nwd, glu_il),
                                    f"lora_quant_tile_f8 N={N} K={K} R={R_} s={scale} nw={with_nw} glu_il={glu_il}")


def test_strided_w_exact():
    """w a strided view (ldw = K + 8) inside a NaN buffer."""
    N, K, R_ = 48, 192, 16
    w, a, b, nw = RR.exact_case(N, K, R_, seed=3, with_nw=True)
    buf = torch.full((N, K + 8), float("nan"), dtype=BF16, device=DEV)
    buf[:, :K] = w.to(DEV)
    wv = buf[:, :K]
    assert wv.stride(0) == K + 8
    m = RR.merged64(w, a, b, 2.0).to(BF16).to(DEV)
    for glu_il in (False, True):
        _same_tile(_tile2(wv, _dev(a), _dev(b), 2.0, _dev(nw), glu_il), _ref_tile(m, _dev(nw), glu_il), "strided w")
        _same_quant(_quant2(wv, _dev(a), _dev(b), 2.0, _dev(nw), glu_il), _ref_quant(m, _dev(nw), glu_il), "strided w")


# ------------------------------------------------------------------------------ random vs fp64
@pytest.mark.parametrize("R_", RANKS)
def test_random_against_fp64(R_):
    for N in NS:
        for K in KS_BF16:
            for scale in SCALES:
                w, a, b, nw = RR.random_case(N, K, R_, seed=N * 7 + K, with_nw=True)
                wd, ad, bd, nwd = _dev(w), _dev(a), _dev(b), _dev(nw)
                m = RR.untile(_tile2(wd, ad, bd, scale, None, False)).contiguous()
                ref = RR.merged64(w, a, b, scale)
                e32 = R.e32_of(w.float() + float(scale) * (b.float() @ a.float()), ref)
                extra = abs(scale) * RL.dot_extra(R_, RL.abs_dot_max(b, a.t()))
                err, bound = R.check("lora_tile_weight", f"N{N} K{K} R{R_} s{scale}", m, ref, e32, extra, bf16=True)
                WORST["ratio"] = max(WORST["ratio"], err / bound)
                for with_nw in (False, True):
                    nwx = nwd if with_nw else None
                    for glu_il in (False, True):
                        if glu_il and not _glu_ok(N):
                            continue
                        what = f"random N={N} K={K} R={R_} s={scale} nw={with_nw} glu_il={glu_il}"
                        _same_tile(_tile2(wd, ad, bd, scale, nwx, glu_il), _ref_tile(m, nwx, glu_il), what)
                        if K % 64 == 0:
                            _same_quant(_quant2(wd, ad, bd, scale, nwx, glu_il), _ref_quant(m, nwx, glu_il), what)
    print(f"FIG lora_tile_weight worst err/bound so far: {WORST['ratio']:.3f}")


def test_zero_adapter_equals_the_existing_ops():
    for N, K in ((48, 192), (160, 1088)):
        w, a, _, nw = RR.random_case(N, K, 16, seed=N, with_nw=True)
        assert not bool(((w == 0) & (w.view(torch.int16) < 0)).any()), "input holds a signed zero"
        wd, ad, nwd = _dev(w), _dev(a), _dev(nw)
        bd = torch.zeros((N, 16), dtype=BF16, device=DEV)
        for nwx in (None, nwd):
            for glu_il in (False, True):
                _same_tile(_tile2(wd, ad, bd, 2.0, nwx, glu_il), _ref_tile(wd, nwx, glu_il), "b = 0")
                _same_quant(_quant2(wd, ad, bd, 2.0, nwx, glu_il), _ref_quant(wd, nwx, glu_il), "b = 0")


def test_bad_arguments_raise():
    N, K = 48, 192
    w, a, b, _ = RR.random_case(N, K, 16, seed=1)
    wd, ad, bd = _dev(w), _dev(a), _dev(b)
    out = torch.empty((N // 16, K // 32, 4, 16, 8), dtype=BF16, device=DEV)
    o8 = torch.empty((N // 16, K // 64, 64, 16), dtype=torch.uint8, device=DEV)
    sc = torch.empty(N, dtype=torch.float32, device=DEV)

    def both(w_, a_, b_, out_=out, o8_=o8, sc_=sc):
        with pytest.raises(RuntimeError):
            torch.ops.dla.lora_tile_weight(w_, a_, b_, 1.0, None, out_, False)
        with pytest.raises(RuntimeError):
            torch.ops.dla.lora_quant_tile_f8(w_, a_, b_, 1.0, None, o8_, sc_, False)

    a12, b12 = RL.rand_bf16((12, K), 2).to(DEV), RL.rand_bf16((N, 12), 3).to(DEV)
    both(wd, a12[:12], b12.contiguous())  # rank 12
    both(wd[:, :K - 16].contiguous(), ad[:, :K - 16].contiguous(), bd)  # K % 32 != 0
    both(wd, ad, bd, out_=out.view(N // 16, K // 32, 4, 8, 16), o8_=o8.view(N // 16, K // 64, 16, 64))  # out shape
    both(w, a, b)  # CPU tensors
    both(wd, ad, _dev(RL.rand_bf16((N, 32), 4)))  # b's r != a's r
    with pytest.raises(RuntimeError):  # fp8: K % 64 != 0
        torch.ops.dla.lora_quant_tile_f8(wd[:, :160].contiguous(), ad[:, :160].contiguous(), bd, 1.0, None,
                                         torch.empty(N * 160, dtype=torch.uint8, device=DEV), sc, False)


def test_wrapper_dispatch_and_fallback():
    """ops.decode with `lora=`: the kernels at the native ranks, the composition (merged() + the
    existing op) at rank 24, same storage and attribute on refresh, the key follows B."""
    N, K = 160, 1088
    w, a, b, nw = RR.random_case(N, K, 16, seed=9, with_nw=True)
    wd, ad, bd, nwd = _dev(w), _dev(a), _dev(b), _dev(nw)
    n0 = dict(D.MERGE_CALLS)
    t = D.folded_weight(wd, nwd, tiled=True, lora=(ad, bd, 2.0))
    assert D.MERGE_CALLS["kernel"] == n0["kernel"] + 1
    _same_tile(t, _tile2(wd, ad, bd, 2.0, nwd, False), "folded_weight(lora=)")
    ptr = t.data_ptr()
    bd.mul_(2)
    t2 = D.folded_weight(wd, nwd, tiled=True, lora=(ad, bd, 2.0))
    assert t2.data_ptr() == ptr and D.MERGE_CALLS["kernel"] == n0["kernel"] + 2
    _same_tile(t2, _tile2(wd, ad, bd, 2.0, nwd, False), "refresh after B moved")
    t3 = D.folded_weight(wd, nwd, tiled=True)
    assert t3.data_ptr() == ptr
    _same_tile(t3, _ref_tile(wd, nwd, False), "adapter off: the existing op on W")
    a24, b24 = RL.rand_bf16((24, K), 5, amp=K ** -0.5).to(DEV), RL.rand_bf16((N, 24), 6, amp=24 ** -0.5).to(DEV)
    w2 = wd.clone()
    tt = D.tiled_weight(w2, lora=(a24, b24, 0.5))
    assert D.MERGE_CALLS["composition"] == n0["composition"] + 1
    _same_tile(tt, _ref_tile(D.merged(w2, (a24, b24, 0.5)), None, False), "rank 24: composition")
    q8, sc = D.fp8_tiled_weight(w2, nwd, lora=(a24, b24, 0.5))
    _same_quant((q8, sc), _ref_quant(D.merged(w2, (a24, b24, 0.5)), nwd, False), "rank 24 fp8: composition")


# ------------------------------------------------------------------------------ end to end
AMP = 0.1  # B amplitude: live-versus-disabled gap of this model >= 0.5 nat / token (asserted below)
NEW = 8


def _tiny(device=DEV, dtype=BF16):
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.models.lora import apply_lora

    cfg = get_config("tiny-llama-d128", hidden_size=1024, num_heads=8, num_kv_heads=2, head_dim=128,
                     intermediate_size=2048, num_layers=3, vocab_size=4096)
    m = build_model(cfg, device=device, dtype=dtype, seed=0)
    apply_lora(m, r=16)
    return cfg, m


def _set_b(m, amp=AMP, seed=100):
    from distributed_llm_alignment_amd.models.lora import lora_adapters

    for i, ad in enumerate(lora_adapters(m)):
        g = torch.Generator().manual_seed(seed + i)
        with torch.no_grad():
            ad.B.copy_((torch.randn(ad.B.shape, generator=g) * amp).to(device=ad.B.device, dtype=ad.B.dtype))


def _prompts(cfg, rows, T=12, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, cfg.vocab_size, (rows, T), generator=g).to(DEV)


@pytest.mark.parametrize("rows", [5, 24])
def test_fresh_adapters_equal_the_disabled_model(rows):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen
    from distributed_llm_alignment_amd.models.lora import lora_disabled

    cfg, m = _tiny()
    ids = _prompts(cfg, rows)
    kw = dict(max_new_tokens=NEW, do_sample=False, eos_token_id=-1, return_logprobs=True)
    for wd in ("bf16", "fp8"):
        for use_graph in (True, False):
            s1, l1 = generate(m, ids, None, adapters="merged", weight_dtype=wd, use_graph=use_graph, **kw)
            with lora_disabled(m):
                s0, l0 = generate(m, ids, None, weight_dtype=wd, use_graph=use_graph, **kw)
            assert torch.equal(s1, s0), (wd, use_graph)
            assert torch.equal(l1.view(torch.int32), l0.view(torch.int32)), (wd, use_graph)
    gen.clear_graph_cache()


def _derived(m):
    """[(weight, attr, norm weight, adapter, glu_il)] of every derived buffer present."""
    out = []
    for layer in m.layers:
        at, mlp = layer.attn, layer.mlp
        for w, nw, ad in ((at.qkv_proj, layer.ln1_w, at.lora_qkv), (mlp.up_proj, layer.ln2_w, mlp.lora_up),
                          (at.o_proj, None, at.lora_o), (mlp.down_proj, None, mlp.lora_down)):
            for attr in D.DERIVED_ATTRS:
                if getattr(w, attr, None) is not None:
                    out.append((w, attr, nw, ad, attr in ("_dla_fold_g", "_dla_f8_g")))
    return out


def _check_buffers(m, merged, what):
    items = _derived(m)
    for w, attr, nw, ad, glu_il in items:
        got = getattr(w, attr)[1]
        A, B, s = ad.A.detach(), ad.B.detach(), ad.scale
        if attr.startswith("_dla_f8"):
            ref = _quant2(w.detach(), A, B, s, nw, glu_il) if merged else _ref_quant(w.detach(), nw, glu_il)
            _same_quant(got, ref, f"{what}: {attr}")
        else:
            ref = _tile2(w.detach(), A, B, s, nw, glu_il) if merged else _ref_tile(w.detach(), nw, glu_il)
            _same_tile(got, ref, f"{what}: {attr}")
    return items


def _ptrs(items):
    out = []
    for w, attr, *_ in items:
        c = getattr(w, attr)[1]
        out.append(tuple(t.data_ptr() for t in (c if isinstance(c, tuple) else (c,))))
    return out


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
def test_derived_buffers_follow_the_adapters(wd):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen
    from distributed_llm_alignment_amd.models.lora import lora_adapters, lora_disabled

    cfg, m = _tiny()
    _set_b(m)
    ids = _prompts(cfg, 5)
    kw = dict(max_new_tokens=NEW, do_sample=False, eos_token_id=-1, weight_dtype=wd)
    generate(m, ids, None, adapters="merged", **kw)
    items = _check_buffers(m, True, "first merged generate")
    attrs = {(i, a) for i, (w, a, *_r) in enumerate(items)}
    names = sorted({a for _, a in attrs})
    # layers 1 and 2 run all four projections fused; layer 0's qkv is the un-fused one
    want = ["_dla_f8", "_dla_f8_g", "_dla_f8_n"] if wd == "fp8" else ["_dla_fold_t", "_dla_tile"]
    assert names == want, names
    assert len(items) == (2 + 3 + 3 + 3), [(a) for _, a, *_r in items]
    ptrs = _ptrs(items)
    slot = gen._GRAPH_SLOT.get(id(m))
    with torch.no_grad():
        for i, ad in enumerate(lora_adapters(m)):
            ad.B.add_(0.01 * (1 + i % 3))
    generate(m, ids, None, adapters="merged", **kw)
    if slot is not None:  # (a captured graph exists in this mode): reused, same cache object
        again = gen._GRAPH_SLOT.get(id(m))
        assert again is not None and again[2] is slot[2] and again[3] is slot[3]
    items2 = _check_buffers(m, True, "after B.add_")
    assert _ptrs(items2) == ptrs
    with lora_disabled(m):
        generate(m, ids, None, **kw)
    items3 = _check_buffers(m, False, "under lora_disabled")
    assert _ptrs(items3) == ptrs
    gen.clear_graph_cache()


def test_graph_is_captured_on_merged_weights():
    """bf16, 5 rows: the merged rollout runs through a captured decode graph, reused after B moves."""
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen
    from distributed_llm_alignment_amd.models.lora import lora_adapters

    cfg, m = _tiny()
    _set_b(m)
    ids = _prompts(cfg, 5)
    kw = dict(max_new_tokens=NEW, do_sample=False, eos_token_id=-1, adapters="merged")
    a = generate(m, ids, None, **kw)
    slot = gen._GRAPH_SLOT[id(m)]
    assert slot[3].graph is not None
    with torch.no_grad():
        lora_adapters(m)[0].B.add_(0.01)
    b = generate(m, ids, None, **kw)
    assert gen._GRAPH_SLOT[id(m)][3] is slot[3] and gen._GRAPH_SLOT[id(m)][2] is slot[2]
    c = generate(m, ids, None, use_graph=False, **kw)
    assert torch.equal(b, c), "graph and eager merged decoding differ"
    assert a.shape == b.shape
    gen.clear_graph_cache()


@pytest.mark.parametrize("rows", [5, 24])
def test_merged_decode_computes_the_adapted_function(rows):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen
    from distributed_llm_alignment_amd.models.lora import lora_disabled

    cfg, m = _tiny()
    _set_b(m)
    ids = _prompts(cfg, rows)
    Tp = ids.shape[1]
    seqs, lp_eng = generate(m, ids, None, max_new_tokens=NEW, do_sample=False, eos_token_id=-1,
                            return_logprobs=True, adapters="merged")
    sl = slice(Tp - 1, Tp - 1 + NEW)
    with torch.no_grad():
        lp_live = m.token_logprobs(seqs)[:, sl].float()
        with lora_disabled(m):
            lp_off = m.token_logprobs(seqs)[:, sl].float()
    # precondition, on the CPU in fp32: the adapters move this model by >= 0.5 nat per token
    _, mc = _tiny(device="cpu", dtype=torch.float32)
    _set_b(mc)
    with torch.no_grad():
        c_live = mc.token_logprobs(seqs.cpu())[:, sl]
        with lora_disabled(mc):
            c_off = mc.token_logprobs(seqs.cpu())[:, sl]
    gap = (c_live - c_off).abs().mean().item()
    g_on = (lp_eng - lp_live).abs().mean().item()
    g_off = (lp_eng - lp_off).abs().mean().item()
    print(f"FIG lora rollout rows {rows}: fp32 live-vs-off gap {gap:.4f} g_on {g_on:.5f} g_off {g_off:.4f}")
    assert gap >= 0.5, gap
    assert g_on < g_off / 10, (g_on, g_off)
    # the same engine-vs-trainer gap of the adapter-free model, for the record
    with lora_disabled(m):
        s0, l0 = generate(m, ids, None, max_new_tokens=NEW, do_sample=False, eos_token_id=-1, return_logprobs=True)
        with torch.no_grad():
            t0 = m.token_logprobs(s0)[:, sl].float()
    print(f"FIG lora rollout rows {rows}: adapter-free engine-vs-trainer gap {(l0 - t0).abs().mean().item():.5f}")
    gen.clear_graph_cache()


def test_default_call_still_refuses_live_adapters():
    from distributed_llm_alignment_amd.models import generate

    cfg, m = _tiny()
    with pytest.raises(ValueError):
        generate(m, _prompts(cfg, 2), None, max_new_tokens=4)
    with pytest.raises(ValueError):
        generate(m, _prompts(cfg, 2), None, max_new_tokens=4, adapters="bogus")


def test_shipped_grpo_lora_config_runs_scaled_down(tmp_path):
    """config/rlhf_grpo_lora_llama3_8b.yaml with the architecture overridden to the tiny d128 preset:
    24 decode rows (the 17..64-row fused layer), rollouts through the captured graph on merged
    copies that the one-pass kernels rebuild after every optimizer step, adapters only updated."""
    import json
    from pathlib import Path

    from safetensors.torch import load_file

    from distributed_llm_alignment_amd.models import generation as gen
    from distributed_llm_alignment_amd.training import train_rlhf

    root = Path(__file__).resolve().parents[1]
    args = ["--config", str(root / "config" / "rlhf_grpo_lora_llama3_8b.yaml")]
    for o in ["model.policy_model_name_or_path=tiny-llama-d128", "reward_model.base_model_name_or_path=tiny-llama-d128",
              "model.max_seq_length=48", "sampling.num_samples=8", "ppo.batch_size=24", "ppo.steps=3",
              "ppo.learning_rate=1e-3", "ppo.generation_params.max_new_tokens=6",
              f"logging.output_dir={tmp_path / 'ck'}", f"logging.log_dir={tmp_path / 'logs'}",
              "logging.log_every_steps=1"]:
        args += ["--override", o]
    gen.clear_graph_cache()
    n0 = D.MERGE_CALLS["kernel"]
    seen = {}
    real = train_rlhf.save_state

    def save(out_dir, models, *a, **k):
        seen["models"] = list(models)
        seen["graph"] = [e[3].graph is not None for e in gen._GRAPH_SLOT.values() if e[0]() is models[0]]
        return real(out_dir, models, *a, **k)

    train_rlhf.save_state = save
    try:
        assert train_rlhf.main(args) == 0
    finally:
        train_rlhf.save_state = real
        gen.clear_graph_cache()
    assert seen["graph"] == [True], "the rollouts did not run through a captured decode graph"
    # 2 layers: qkv of layer 1 + gate|up, o, down of both = 7 merged copies, rebuilt for each of 3 rollouts
    assert D.MERGE_CALLS["kernel"] - n0 == 7 * 3, D.MERGE_CALLS["kernel"] - n0
    assert len(seen["models"]) == 2
    ad = load_file(str(tmp_path / "ck" / "adapter.safetensors"))
    assert any(k.endswith(".B") and float(v.float().abs().sum()) > 0 for k, v in ad.items())
    rows = [json.loads(l) for l in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines()]
    kl = [r["train/rollout_kl"] for r in rows if "train/rollout_kl" in r]
    print(f"FIG lora rollout trainer: train/rollout_kl per step {kl}")
    assert len(kl) == 3
