"""MXFP4 weight-only decode, the CPU formulas of record (ops/decode.py quantize_mxfp4 /
dequantize_mxfp4 / tile_mxfp4) and `generate(weight_dtype="mxfp4")` off the GPU (placed quantiser
cases with hand-written codes: _mxfp4_cases.py)."""
import copy

import pytest
import torch

from distributed_llm_alignment_amd.models import build_model, generate, get_config
from distributed_llm_alignment_amd.ops import decode as D

from _mxfp4_cases import placed_row

def test_quantize_placed_values():
    x, codes, scales = placed_row()
    for src in (x, x.to(torch.bfloat16)):
        c, s = D.quantize_mxfp4(src.view(1, -1))
        assert torch.equal(s[0], scales)
        assert torch.equal(c[0], codes)


def test_roundtrip_on_grid():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 256, (16, 64), generator=g, dtype=torch.uint8)
    scales = torch.randint(40, 200, (16, 4), generator=g, dtype=torch.uint8)
    x = D.dequantize_mxfp4(codes, scales)
    assert x.dtype == torch.float32 and x.shape == (16, 128)
    assert torch.equal(x.to(torch.bfloat16).float(), x)  # exact in bf16
    assert torch.equal(D.dequantize_mxfp4(*D.quantize_mxfp4(x)), x)


def test_tile_layout_index_formula():
    N, K = 32, 256
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(0, 256, (N, K // 32), generator=g, dtype=torch.uint8)
    t, sc = D.tile_mxfp4(codes, scales)
    assert t.shape == (N // 16, K // 128, 64, 16) and sc.shape == (N // 16, K // 128, 16, 4)
    ti, kt, lane, by = torch.meshgrid(*(torch.arange(n) for n in t.shape), indexing="ij")
    r, q, sl, j = lane & 15, lane >> 4, by >> 2, by & 3  # byte 4s + j of lane r + 16q
    assert torch.equal(t, codes[16 * ti + r, (128 * kt + 32 * sl + 8 * q) // 2 + j])
    ti, kt, r, sl = torch.meshgrid(*(torch.arange(n) for n in sc.shape), indexing="ij")
    assert torch.equal(sc, scales[16 * ti + r, 4 * kt + sl])


def test_unknown_values_raise():
    from distributed_llm_alignment_amd.training.train_rlhf import rollout_weight_dtype

    cfg = get_config("tiny-llama-d128")
    m = build_model(cfg, device="cpu", dtype=torch.float32, seed=0).eval()
    with pytest.raises(ValueError, match="weight_dtype"):
        generate(m, torch.randint(3, cfg.vocab_size, (2, 6)), max_new_tokens=2, weight_dtype="nope")
    with pytest.raises(ValueError, match="rollout_weight_dtype"):
        rollout_weight_dtype({"rollout_weight_dtype": "nope"})
    assert rollout_weight_dtype({}) == "bf16" and rollout_weight_dtype({"rollout_weight_dtype": "mxfp4"}) == "mxfp4"
    with D.fp8_weights(True), pytest.raises(RuntimeError):
        D.mxfp4_weights(True).__enter__()


def test_generate_equals_model_with_dequantised_weights():
    cfg = get_config("tiny-llama-d128", hidden_size=1024, num_heads=8, num_kv_heads=2, head_dim=128,
                     intermediate_size=2048, num_layers=3, vocab_size=4096)
    m = build_model(cfg, device="cpu", dtype=torch.float32, seed=4).eval()
    ref = copy.deepcopy(m)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n == "lm_head" or n.endswith(("qkv_proj", "o_proj", "up_proj", "down_proj")):
                p.copy_(D.dequantize_mxfp4(*D.quantize_mxfp4(p)))
    ids = torch.randint(3, cfg.vocab_size, (2, 8), generator=torch.Generator().manual_seed(2))
    kw = dict(max_new_tokens=6, do_sample=False, eos_token_id=-1)
    a = generate(m, ids, weight_dtype="mxfp4", **kw)
    assert torch.equal(a, generate(ref, ids, **kw))
    assert not torch.equal(a, generate(m, ids, **kw))  # the quantised weights were in use
    assert not D.mxfp4_enabled() and not hasattr(m.lm_head, "_dla_mx")
