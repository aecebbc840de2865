"""Group-shared decode attention on the CPU tier: the `group_size` / `prefix_len` arguments of
`ops.decode.decode_attention`, the grouped torch reference (which rows it reads), the argument
checks, and the `group_attention` switch through `generate` and the GRPO trainer (a no-op on the
fallback paths: same tokens)."""
from pathlib import Path

import pytest
import torch

from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.models import KVCache, build_model, generate, get_config, prefill_shared
from distributed_llm_alignment_amd.ops.decode import (decode_attention, ref_decode_attention,
                                                      ref_decode_attention_grouped)

ROOT = Path(__file__).resolve().parents[1]
P, G, TP, L, TMAX, HQ, HKV, D = 3, 4, 9, 14, 16, 4, 2, 16


@pytest.fixture(scope="module")
def shared():
    """A group-structured batch: rows p*G .. p*G+G-1 share keys / values [0, TP)."""
    g = torch.Generator().manual_seed(0)
    B = P * G
    q = torch.randn(B, HQ, D, generator=g)
    k = torch.randn(B, TMAX, HKV, D, generator=g)
    v = torch.randn(B, TMAX, HKV, D, generator=g)
    first = (torch.arange(B) // G) * G
    k[:, :TP] = k[first, :TP]
    v[:, :TP] = v[first, :TP]
    kv_start = torch.tensor([0, 3, TP - 1], dtype=torch.int32).repeat_interleave(G)
    return q, k, v, kv_start


@pytest.mark.parametrize("window", [0, 8, 3])
def test_decode_attention_group_arguments_on_cpu_equal_the_reference(shared, window):
    q, k, v, kv_start = shared
    kv_len = torch.tensor([L], dtype=torch.int32)
    want = ref_decode_attention(q, k, v, L, kv_start, window)
    got = decode_attention(q, k, v, kv_len, kv_start, window, group_size=G, prefix_len=TP)
    assert torch.equal(got, want)
    assert torch.equal(decode_attention(q, k, v, kv_len, kv_start, window), want)  # the defaults: today's call


@pytest.mark.parametrize("window", [0, 8, 3])
def test_grouped_reference_reads_the_first_rows_prefix(shared, window):
    q, k, v, kv_start = shared
    want = ref_decode_attention(q, k, v, L, kv_start, window)
    assert torch.allclose(ref_decode_attention_grouped(q, k, v, L, G, TP, kv_start, window), want, atol=1e-6)
    # the prefix of rows g >= 1 overwritten: the grouped reference never reads it
    k2, v2 = k.clone(), v.clone()
    rest = torch.arange(P * G) % G != 0
    k2[rest, :TP] = 50.0
    v2[rest, :TP] = 50.0
    assert torch.allclose(ref_decode_attention_grouped(q, k2, v2, L, G, TP, kv_start, window), want, atol=1e-6)
    if window != 3:  # (window 3: no prefix key is visible, nothing to tell the two apart)
        assert not torch.allclose(ref_decode_attention(q, k2, v2, L, kv_start, window), want, atol=1e-2)


def test_decode_attention_group_argument_checks(shared):
    q, k, v, kv_start = shared
    kv_len = torch.tensor([L], dtype=torch.int32)
    for kw in (dict(group_size=5, prefix_len=TP),      # does not divide the 12 rows
               dict(group_size=0, prefix_len=TP),
               dict(group_size=G, prefix_len=0),
               dict(group_size=G, prefix_len=TMAX + 1)):
        with pytest.raises(ValueError):
            decode_attention(q, k, v, kv_len, kv_start, **kw)
        with pytest.raises(ValueError):
            ref_decode_attention_grouped(q, k, v, L, kw["group_size"], kw["prefix_len"], kv_start)
    decode_attention(q, k, v, kv_len, kv_start, group_size=G, prefix_len=TMAX)  # the upper bound is allowed


@pytest.fixture(scope="module")
def tiny():
    cfg = get_config("tiny-llama")
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=0).eval()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, cfg.vocab_size, (3, 11), generator=g)
    am = torch.ones(3, 11, dtype=torch.long)
    am[1, :4] = 0  # one left-padded prompt
    ids[1, :4] = 0
    return model, ids, am


def test_generate_group_attention_same_tokens_on_cpu(tiny):
    model, ids, am = tiny
    kw = dict(max_new_tokens=6, do_sample=True, temperature=0.9, eos_token_id=-1, pad_token_id=0,
              return_mask=True, num_return_sequences=3)
    a, ma = generate(model, ids, am, generator=torch.Generator().manual_seed(5), group_attention=False, **kw)
    b, mb = generate(model, ids, am, generator=torch.Generator().manual_seed(5), group_attention=True, **kw)
    assert torch.equal(a, b) and torch.equal(ma, mb)
    # no effect without groups / without the shared prefill
    kw["num_return_sequences"] = 1
    c = generate(model, ids, am, generator=torch.Generator().manual_seed(5), group_attention=True, **kw)[0]
    d = generate(model, ids, am, generator=torch.Generator().manual_seed(5), **kw)[0]
    assert torch.equal(c, d)


def test_kvcache_group_attribute(tiny):
    model, ids, am = tiny
    Tp = ids.shape[1]
    with torch.no_grad():
        cache, _ = prefill_shared(model, ids, am, 3, Tp + 4)
        assert cache.group is None
        cache, _ = prefill_shared(model, ids, am, 3, Tp + 4, group_attention=True)
        assert cache.group == (3, Tp)
        cache.reset(None)
        assert cache.group is None
        assert KVCache(model, 3, Tp, None).group is None
        cache, _ = prefill_shared(model, ids, am, 1, Tp + 4, group_attention=True)
        assert cache.group is None  # groups of one: nothing to share


def test_grpo_trainer_runs_with_group_attention(tmp_path):
    from distributed_llm_alignment_amd.training import train_rlhf

    prompts = tmp_path / "prompts.jsonl"
    write_jsonl(prompts, synthetic_prompt_records(6, seed=4))
    ov = ["optimization.max_train_steps=1", f"logging.output_dir={tmp_path / 'ck'}",
          f"logging.log_dir={tmp_path / 'logs'}", "logging.save_every_steps=0", "logging.use_wandb=false",
          "logging.log_every_steps=1", "data.num_workers=0", "hardware.gradient_accumulation_steps=1",
          "model.policy_model_name_or_path=tiny-llama", "model.reference_model_name_or_path=tiny-llama",
          "model.max_seq_length=48", "reward_model.path=null", "reward_model.base_model_name_or_path=tiny-llama",
          "ppo.algorithm=grpo", "ppo.group_size=2", "ppo.batch_size=4", "ppo.steps=1",
          "ppo.generation_params.max_new_tokens=4", "ppo.group_attention=true",
          "sampling.source=local", f"sampling.prompt_path={prompts}"]
    args = ["--config", str(ROOT / "config" / "rlhf_config.yaml")]
    for o in ov:
        args += ["--override", o]
    assert train_rlhf.main(args) == 0
