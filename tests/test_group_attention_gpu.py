"""Group-shared decode attention on the MI355X (csrc/decode.hip decode_prefix_kernel + the loop
kernel's grouped form): `decode_attn_group` / `decode_attn_rope_group` against the fp32 reference
that reads the prefix of row p*G, the rows they read, their bitwise properties, graph capture with
device-side lengths, and the `group_attention` switch through KVCache, `generate` and one GRPO step.

Tolerance of the reference comparison: atol = rtol = 2e-2, the one tests/test_decode_gpu.py uses
for this kernel family (bf16 output of an fp32 softmax over bf16 P.V MFMAs)."""
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = Path(__file__).resolve().parents[1]
P, TMAX = 3, 640
BIG = 1.0e4  # the "large finite constant" written over the prefix of rows g >= 1

A, S64, C8 = (128, 32, 8), (64, 8, 8), (128, 16, 2)  # (D, Hq, Hkv): 4, 1 and 8 q heads per kv head
# (shape, G, Tp, kv_len - Tp, window, split geometry, cache layout)
#   G: 2; 5 (padded columns); 8; 20 (two 16-row tiles at 4 heads, 8 + 8 + 4 rows at 8 heads)
#   Tp: 1, 7, 130, 257, 384 (chunk-aligned and not); window 300 cuts into the prefix, window 20 with
#   kv_len = Tp + 37 leaves the whole prefix outside
#   geometry: None = default, "16" / "60" = DLA_DECODE_BLOCKS, "one-chunk" = DLA_DECODE_LOOP=0
CASES = [
    (A, 8, 384, 37, 0, None, "token"),
    (A, 8, 257, 200, 0, "16", "token"),
    (A, 8, 130, 1, 0, "60", "head"),
    (A, 8, 384, 200, 300, "one-chunk", "token"),
    (A, 5, 257, 37, 0, None, "head"),
    (A, 5, 7, 1, 0, None, "token"),
    (A, 20, 384, 37, 0, None, "token"),
    (A, 20, 130, 200, 300, "60", "head"),
    (A, 2, 1, 1, 0, None, "token"),
    (A, 2, 1, 200, 0, "one-chunk", "token"),
    (A, 8, 384, 37, 20, None, "token"),
    (A, 8, 257, 37, 20, "16", "head"),
    (A, 8, 257, 37, 0, None, "layer"),
    (S64, 2, 130, 37, 0, None, "token"),
    (S64, 5, 384, 200, 300, "16", "head"),
    (S64, 8, 257, 1, 0, "one-chunk", "token"),
    (S64, 8, 7, 37, 20, "60", "token"),
    (S64, 20, 257, 200, 0, None, "head"),
    (S64, 8, 384, 200, 0, None, "layer"),
    (C8, 2, 384, 200, 0, None, "token"),
    (C8, 5, 130, 37, 300, "60", "head"),
    (C8, 8, 257, 1, 0, "16", "token"),
    (C8, 8, 1, 37, 0, "one-chunk", "head"),
    (C8, 20, 384, 37, 20, None, "token"),
    (C8, 20, 7, 200, 0, "60", "head"),
]
POISONED = [CASES[i] for i in (0, 3, 4, 7, 9, 12, 14, 17, 20, 22, 24)]


def _id(c):
    (D, Hq, Hkv), G, Tp, dl, w, blocks, layout = c
    return f"D{D}h{Hq}kv{Hkv}-G{G}-Tp{Tp}+{dl}-w{w}-{blocks}-{layout}"


@pytest.fixture(scope="module", autouse=True)
def _native():
    from distributed_llm_alignment_amd.ops import _ext

    _ext.require()


def _geometry(blocks, monkeypatch):
    if blocks == "one-chunk":
        monkeypatch.setenv("DLA_DECODE_LOOP", "0")
    elif blocks is not None:
        monkeypatch.setenv("DLA_DECODE_BLOCKS", blocks)


def _cache(B, Hkv, D, layout, g):
    """randn -> bf16 behind the [B, TMAX, Hkv, D] view the ops take."""
    if layout == "head":  # head-major storage, as KVCache keeps it
        return torch.randn(B, Hkv, TMAX, D, device=DEV, generator=g).to(torch.bfloat16).transpose(1, 2)
    if layout == "layer":  # one layer of an [L, B, ...] cache
        return torch.randn(3, B, TMAX, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)[1]
    return torch.randn(B, TMAX, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)


def _first(B, G):
    return (torch.arange(B, device=DEV) // G) * G


def _inputs(case, seed=0):
    (D, Hq, Hkv), G, Tp, dl, window, _, layout = case
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = P * G
    kc, vc = _cache(B, Hkv, D, layout, g), _cache(B, Hkv, D, layout, g)
    first = _first(B, G)
    kc[:, :Tp] = kc[first, :Tp]  # the rows of a group share the prefix
    vc[:, :Tp] = vc[first, :Tp]
    q = torch.randn(B, Hq, D, device=DEV, generator=g).to(torch.bfloat16)
    ks = torch.tensor([0, min(3, Tp - 1), Tp - 1], dtype=torch.int32, device=DEV).repeat_interleave(G)
    L = Tp + dl
    return q, kc, vc, ks, L, torch.tensor([L], dtype=torch.int32, device=DEV)


def _poison(kc, vc, G, Tp):
    rest = torch.arange(kc.shape[0], device=DEV) % G != 0
    kc[rest, :Tp] = BIG
    vc[rest, :Tp] = BIG


# ------------------------------------------------------------------ 1. the fp32 reference
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_group_decode_attention_matches_reference(case, monkeypatch):
    from distributed_llm_alignment_amd.ops import decode

    (D, Hq, Hkv), G, Tp, dl, window, blocks, layout = case
    _geometry(blocks, monkeypatch)
    q, kc, vc, ks, L, kv_len = _inputs(case)
    o = decode.decode_attention(q, kc, vc, kv_len, ks, window, group_size=G, prefix_len=Tp)
    r = decode.ref_decode_attention_grouped(q, kc, vc, L, G, Tp, ks, window)
    row = decode.decode_attention(q, kc, vc, kv_len, ks, window)  # the per-row op, for the record
    err = (o.float() - r.float()).abs().max().item()
    print(f"{_id(case)}: max |grouped - ref| {err:.3e}, max |grouped - per-row| "
          f"{(o.float() - row.float()).abs().max().item():.3e}")
    assert o.shape == (P * G, Hq, D) and torch.isfinite(o.float()).all()
    assert torch.allclose(o.float(), r.float(), atol=2e-2, rtol=2e-2), err
    # no float atomics, a fixed merge order: a second call is bitwise equal
    assert torch.equal(decode.decode_attention(q, kc, vc, kv_len, ks, window, group_size=G, prefix_len=Tp), o)


# ------------------------------------------------------- 2. only the first row's prefix is read
@pytest.mark.parametrize("case", POISONED, ids=_id)
def test_group_decode_attention_reads_only_the_first_rows_prefix(case, monkeypatch):
    from distributed_llm_alignment_amd.ops import decode

    (D, Hq, Hkv), G, Tp, dl, window, blocks, layout = case
    _geometry(blocks, monkeypatch)
    q, kc, vc, ks, L, kv_len = _inputs(case)
    r = decode.ref_decode_attention_grouped(q, kc, vc, L, G, Tp, ks, window)  # before the overwrite
    clean = decode.decode_attention(q, kc, vc, kv_len, ks, window, group_size=G, prefix_len=Tp)
    _poison(kc, vc, G, Tp)
    o = decode.decode_attention(q, kc, vc, kv_len, ks, window, group_size=G, prefix_len=Tp)
    err = (o.float() - r.float()).abs().max().item()
    print(f"{_id(case)}: max |grouped(poisoned) - ref| {err:.3e}")
    assert torch.allclose(o.float(), r.float(), atol=2e-2, rtol=2e-2), err
    assert torch.equal(o, clean)  # bytes that are never read cannot move the result
    # the reference built from row p*G sees the same thing on the overwritten cache
    r2 = decode.ref_decode_attention_grouped(q, kc, vc, L, G, Tp, ks, window)
    assert torch.equal(r2, r)


# ------------------------------------------------------------------------ 3. bitwise properties
@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[6], CASES[17], CASES[23]], ids=_id)
def test_group_rows_with_equal_query_and_suffix_are_bitwise_equal(case, monkeypatch):
    from distributed_llm_alignment_amd.ops import decode

    (D, Hq, Hkv), G, Tp, dl, window, blocks, layout = case
    _geometry(blocks, monkeypatch)
    q, kc, vc, ks, L, kv_len = _inputs(case)
    first = _first(P * G, G)
    q = q[first].contiguous()
    kc[:, Tp:] = kc[first, Tp:]
    vc[:, Tp:] = vc[first, Tp:]
    o = decode.decode_attention(q, kc, vc, kv_len, ks, window, group_size=G, prefix_len=Tp)
    grouped = o.view(P, G, Hq, D)
    assert torch.equal(grouped, grouped[:, :1].expand_as(grouped))


@pytest.mark.parametrize("D,Hq,Hkv,rot,G", [(128, 32, 8, 128, 5), (64, 8, 8, 32, 8), (128, 8, 1, 64, 8),
                                            (128, 32, 8, 128, 20)])
@pytest.mark.parametrize("blocks", [None, "4", "one-chunk"])
def test_fused_rope_group_decode_attention_matches_unfused(D, Hq, Hkv, rot, G, blocks, monkeypatch):
    """decode_attn_rope_group == rope_cache_write + decode_attn_group, bitwise: the output and the
    written cache row (mirrors test_fused_rope_decode_attention_matches_unfused; the newest token
    sits at slot 256, the first key of a fresh 128-key chunk, the prefix ends inside chunk 1)."""
    from distributed_llm_alignment_amd.ops import RotaryCache, _ext

    _geometry(blocks, monkeypatch)
    C = _ext.require()
    g = torch.Generator(device=DEV).manual_seed(7)
    B, Tmax, L, Tp = P * G, 300, 257, 200
    rope = RotaryCache(rot, 10000.0, 4096, None)
    cos, sin = rope.tables(DEV)
    kc = torch.randn(B, Tmax, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Tmax, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    first = _first(B, G)
    kc[:, :Tp] = kc[first, :Tp]
    vc[:, :Tp] = vc[first, :Tp]
    qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    kv_start = torch.tensor([0, 5, 40], device=DEV, dtype=torch.int32).repeat_interleave(G)
    pos = (L - 1 - kv_start).to(torch.int32)
    slot = torch.tensor([L - 1], device=DEV, dtype=torch.long)
    kv_len = torch.tensor([L], device=DEV, dtype=torch.int32)
    k1, v1 = kc.clone(), vc.clone()
    q = C.rope_cache_write(qkv, cos, sin, pos, k1, v1, slot, Hq, Hkv, D, rot)
    ref = C.decode_attn_group(q, k1, v1, kv_len, kv_start, 0, D ** -0.5, G, Tp)
    k2, v2 = kc.clone(), vc.clone()
    out = C.decode_attn_rope_group(qkv, cos, sin, pos, k2, v2, slot, kv_len, kv_start, 0, D ** -0.5, Hq, Hkv,
                                   D, rot, G, Tp)
    torch.cuda.synchronize()
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert torch.equal(out, ref)
    # and the pair stays inside the reference tolerance of the per-row op's result
    row = C.decode_attn(q, k1, v1, kv_len, kv_start, 0, D ** -0.5)
    assert torch.allclose(out.float(), row.float(), atol=2e-2, rtol=2e-2)


def test_group_op_argument_checks():
    from distributed_llm_alignment_amd.ops import decode

    q, kc, vc, ks, L, kv_len = _inputs(CASES[0])
    for kw in (dict(group_size=7, prefix_len=384), dict(group_size=8, prefix_len=0),
               dict(group_size=8, prefix_len=TMAX + 1)):
        with pytest.raises(ValueError):
            decode.decode_attention(q, kc, vc, kv_len, ks, **kw)
    C = decode._ext.require()
    with pytest.raises(RuntimeError, match="group_size"):
        C.decode_attn_group(q, kc, vc, kv_len, ks, 0, 128 ** -0.5, 7, 384)
    with pytest.raises(RuntimeError, match="prefix_len"):
        C.decode_attn_group(q, kc, vc, kv_len, ks, 0, 128 ** -0.5, 8, TMAX + 1)


# ----------------------------------------------------------------------------- 4. graph capture
@pytest.mark.parametrize("fused", [True, False])
def test_group_decode_step_graph_replay_matches_eager(fused):
    """One grouped step captured in a hipGraph; the newest token, kv_len / slot / pos then move on
    the device and the replay equals the same step run eagerly, bitwise (output and cache)."""
    from distributed_llm_alignment_amd.ops import RotaryCache, _ext

    C = _ext.require()
    (D, Hq, Hkv), G, Tp, L0, Tmax = A, 5, 130, 255, 300
    B = P * G
    g = torch.Generator(device=DEV).manual_seed(11)
    rope = RotaryCache(D, 10000.0, 4096, None)
    cos, sin = rope.tables(DEV)
    kc = torch.randn(B, Tmax, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Tmax, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    first = _first(B, G)
    kc[:, :Tp] = kc[first, :Tp]
    vc[:, :Tp] = vc[first, :Tp]
    qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    qkv_next = [torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16) for _ in range(2)]
    kv_start = torch.tensor([0, 5, 40], device=DEV, dtype=torch.int32).repeat_interleave(G)
    pos = (L0 - 1 - kv_start).to(torch.int32)
    slot = torch.tensor([L0 - 1], device=DEV, dtype=torch.long)
    kv_len = torch.tensor([L0], device=DEV, dtype=torch.int32)

    def step(x, k, v, s, n, p):
        if fused:
            return C.decode_attn_rope_group(x, cos, sin, p, k, v, s, n, kv_start, 0, D ** -0.5, Hq, Hkv, D, D, G, Tp)
        q = C.rope_cache_write(x, cos, sin, p, k, v, s, Hq, Hkv, D, D)
        return C.decode_attn_group(q, k, v, n, kv_start, 0, D ** -0.5, G, Tp)

    ke, ve = kc.clone(), vc.clone()  # the eager arm's cache
    step(qkv, ke, ve, slot, kv_len, pos)  # warm (arrival counters are never created in a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(qkv, kc, vc, slot, kv_len, pos)
    graph.replay()  # step at L0 (the eager arm ran it as the warm-up call)
    for nxt in qkv_next:  # 255 -> 256 -> 257: the newest token crosses into a fresh chunk
        qkv.copy_(nxt)
        slot.add_(1)
        kv_len.add_(1)
        pos.add_(1)
        graph.replay()
        torch.cuda.synchronize()
        want = step(nxt, ke, ve, slot.clone(), kv_len.clone(), pos.clone())
        assert torch.equal(out, want)
        assert torch.equal(kc, ke) and torch.equal(vc, ve)


# ------------------------------------------------------------------------------ 5. model level
def rel_l2(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-12)).item()


@pytest.fixture(scope="module")
def rollout_model():
    from distributed_llm_alignment_amd.models import build_model, get_config

    cfg = get_config("tiny-llama-d128")
    m = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    g = torch.Generator(device=DEV).manual_seed(3)
    ids = torch.randint(3, cfg.vocab_size, (3, 20), device=DEV, generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0  # left padding
    ids[1, :5] = 0
    return m, ids, am


def test_kvcache_group_decode_tracks_per_row_decode(rollout_model):
    """Teacher-forced: 6 decode steps with the same tokens through a cache with and without
    `group`; the bound is the one tests/test_grpo_gpu.py uses between prefill arms. A third cache
    has the prompt K/V of rows g >= 1 overwritten: the grouped steps never read them."""
    from distributed_llm_alignment_amd.models import prefill_shared

    m, ids, am = rollout_model
    (Pn, Tp), G, n = ids.shape, 4, 6
    m.eval()
    g = torch.Generator(device=DEV).manual_seed(5)
    toks = torch.randint(3, m.cfg.vocab_size, (n, Pn * G, 1), device=DEV, generator=g)
    with torch.no_grad():
        row, _ = prefill_shared(m, ids, am, G, Tp + n + 1)
        grp, _ = prefill_shared(m, ids, am, G, Tp + n + 1, group_attention=True)
        bad, _ = prefill_shared(m, ids, am, G, Tp + n + 1, group_attention=True)
        assert row.group is None and grp.group == (G, Tp) and grp.fast_decode
        rest = torch.arange(Pn * G, device=DEV) % G != 0
        bad.k[:, rest, :Tp] = BIG
        bad.v[:, rest, :Tp] = BIG
        for t in range(n):
            h_row = m(toks[t], cache=row)
            h_grp = m(toks[t], cache=grp)
            h_bad = m(toks[t], cache=bad)
            assert rel_l2(h_grp, h_row) < 1e-2, (t, rel_l2(h_grp, h_row))
            assert torch.equal(h_bad, h_grp), t
    assert row.len == grp.len == Tp + n


def test_generate_group_attention_greedy(rollout_model):
    from distributed_llm_alignment_amd.models import generate

    m, ids, am = rollout_model
    (Pn, Tp), G, n = ids.shape, 4, 24
    kw = dict(max_new_tokens=n, do_sample=False, eos_token_id=-1, return_mask=True, num_return_sequences=G)
    seqs, mask = generate(m, ids, am, group_attention=True, **kw)
    assert seqs.shape == (Pn * G, Tp + n) and mask.shape == (Pn * G, Tp + n)
    assert torch.equal(seqs[:, :Tp], ids.repeat_interleave(G, 0))
    assert torch.equal(mask[:, :Tp], am.repeat_interleave(G, 0)) and (mask[:, Tp:] == 1).all()
    grouped = seqs.view(Pn, G, Tp + n)
    assert torch.equal(grouped, grouped[:, :1].expand_as(grouped))  # the rows of a group are identical


def test_generate_group_attention_sampled_graph_matches_eager(rollout_model):
    from distributed_llm_alignment_amd.models import generate

    m, ids, am = rollout_model
    (Pn, Tp), G, n = ids.shape, 4, 24
    kw = dict(max_new_tokens=n, do_sample=True, temperature=0.8, eos_token_id=-1, seed=11,
              num_return_sequences=G, group_attention=True)
    a = generate(m, ids, am, use_graph=True, **kw)
    b = generate(m, ids, am, use_graph=False, **kw)
    assert a.shape == (Pn * G, Tp + n)
    assert torch.equal(a, b)  # graph replay and the eager loop draw the same tokens
    new = a[:, Tp:].view(Pn, G, n)
    for p in range(Pn):  # the G rows of a group sample independently
        assert any(not torch.equal(new[p, 0], new[p, gg]) for gg in range(1, G)), p
    assert torch.equal(generate(m, ids, am, use_graph=True, **kw), a)  # same seed: same rollouts


def test_generate_group_attention_toggle_never_replays_the_other_arms_graph(rollout_model):
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation

    m, ids, am = rollout_model
    kw = dict(max_new_tokens=24, do_sample=True, temperature=0.8, eos_token_id=-1, seed=13,
              num_return_sequences=4, use_graph=True)
    generation.release_graph_cache(m)
    off0 = generate(m, ids, am, group_attention=False, **kw)
    key_off = generation._GRAPH_SLOT[id(m)][1]
    on1 = generate(m, ids, am, group_attention=True, **kw)
    key_on = generation._GRAPH_SLOT[id(m)][1]
    assert key_on != key_off and generation._GRAPH_SLOT[id(m)][2].group is not None
    off2 = generate(m, ids, am, group_attention=False, **kw)
    assert generation._GRAPH_SLOT[id(m)][2].group is None
    on3 = generate(m, ids, am, group_attention=True, **kw)
    assert torch.equal(off2, off0) and torch.equal(on3, on1)
    # the eager loop of each arm agrees with its graph
    assert torch.equal(generate(m, ids, am, group_attention=False, **{**kw, "use_graph": False}), off0)
    assert torch.equal(generate(m, ids, am, group_attention=True, **{**kw, "use_graph": False}), on1)


def test_generate_group_attention_graph_is_keyed_by_group_size():
    """G is a host constant of the captured grouped step: 2 prompts x 4 samples and 4 prompts x 2
    samples have the same number of decode rows, prompt bucket and sampling arguments, and must not
    share a graph (rows 2 and 3 of the second call belong to prompt 1, not to prompt 0)."""
    from distributed_llm_alignment_amd.models import build_model, generate, generation, get_config

    cfg = get_config("tiny-llama-d128")
    m = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    g = torch.Generator(device=DEV).manual_seed(9)
    ids = torch.randint(3, cfg.vocab_size, (4, 20), device=DEV, generator=g)
    am = torch.ones_like(ids)
    kw = dict(max_new_tokens=24, do_sample=True, temperature=0.8, eos_token_id=-1, seed=17,
              group_attention=True)
    generation.release_graph_cache(m)
    a4 = generate(m, ids[:2], am[:2], num_return_sequences=4, use_graph=True, **kw)
    key4 = generation._GRAPH_SLOT[id(m)][1]
    a2 = generate(m, ids, am, num_return_sequences=2, use_graph=True, **kw)  # straight after G = 4
    assert generation._GRAPH_SLOT[id(m)][1] != key4
    assert generation._GRAPH_SLOT[id(m)][2].group[0] == 2
    assert a4.shape == a2.shape
    # each against the eager loop, and against a graph captured from scratch
    assert torch.equal(a2, generate(m, ids, am, num_return_sequences=2, use_graph=False, **kw))
    assert torch.equal(a4, generate(m, ids[:2], am[:2], num_return_sequences=4, use_graph=False, **kw))
    generation.release_graph_cache(m)
    assert torch.equal(a2, generate(m, ids, am, num_return_sequences=2, use_graph=True, **kw))
    # greedy, again straight after a G = 4 call: the rows of each of the 4 groups are identical
    gk = dict(max_new_tokens=24, do_sample=False, eos_token_id=-1, group_attention=True)
    generate(m, ids[:2], am[:2], num_return_sequences=4, **gk)
    s2 = generate(m, ids, am, num_return_sequences=2, **gk).view(4, 2, -1)
    assert torch.equal(s2, s2[:, :1].expand_as(s2))


def test_kvcache_group_refuses_a_cache_shorter_than_the_prefix(rollout_model):
    from distributed_llm_alignment_amd.models import prefill_shared

    m, ids, am = rollout_model
    (Pn, Tp), G = ids.shape, 4
    m.eval()
    with torch.no_grad():
        cache, _ = prefill_shared(m, ids, am, G, Tp + 4, group_attention=True)
        cache.group = (G, Tp + 2)  # a prefix boundary beyond the keys the cache holds
        tok = torch.full((Pn * G, 1), 5, dtype=torch.long, device=DEV)
        with pytest.raises(RuntimeError, match="prefix"):
            m(tok, cache=cache)


# ------------------------------------------------------------------------------- 6. one GRPO step
def test_grpo_trainer_step_with_group_attention(tmp_path):
    import math

    import yaml

    from distributed_llm_alignment_amd.data import write_jsonl
    from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
    from distributed_llm_alignment_amd.training import train_rlhf

    write_jsonl(tmp_path / "prompts.jsonl", synthetic_prompt_records(8, seed=4))
    model = "tiny-llama-d128"
    rl = {"seed": 21,
          "model": {"policy_model_name_or_path": model, "reference_model_name_or_path": model, "max_seq_length": 64},
          "reward_model": {"path": None, "base_model_name_or_path": model},
          "ppo": {"algorithm": "grpo", "batch_size": 8, "group_size": 4, "learning_rate": 1e-4, "kl_coef": 0.04,
                  "steps": 1, "group_attention": True,
                  "generation_params": {"max_new_tokens": 8, "temperature": 0.7, "top_p": 0.9}},
          "sampling": {"source": "local", "prompt_path": str(tmp_path / "prompts.jsonl")},
          "logging": {"output_dir": str(tmp_path / "ck"), "log_dir": str(tmp_path / "logs"), "log_every_steps": 1}}
    cfg = tmp_path / "rl.yaml"
    cfg.write_text(yaml.safe_dump(rl))
    assert train_rlhf.main(["--config", str(cfg)]) == 0
    rows = [json.loads(l) for l in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines()]
    last = [r for r in rows if "train/loss" in r][-1]
    assert math.isfinite(last["train/loss"]) and math.isfinite(last["train/grad_norm"]), last
    assert last["train/grad_norm"] > 0
