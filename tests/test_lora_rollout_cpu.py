"""CPU tier: LoRA-merged decode weights (ops.decode `lora=`), `generate(..., adapters="merged")`
and `model.lora` in the RLHF trainer (grpo / ppo)."""
import json
from pathlib import Path

import pytest
import torch
import yaml

from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.models import build_model, generate, get_config
from distributed_llm_alignment_amd.models import lora as ML
from distributed_llm_alignment_amd.ops import decode as D

import _refs64_lora_rollout as RR

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------ ops.decode fallbacks
def _torch_tile(src):
    N, K = src.shape
    return src.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


@pytest.mark.parametrize("R_", [8, 12, 64])
def test_decode_fallbacks_equal_merged_weight_then_the_torch_path(R_):
    N, K = 64, 128
    w, a, b, nw = RR.random_case(N, K, R_, seed=R_, with_nw=True)
    ad = ML.LoRAAdapter(K, N, R_, 2 * R_, 0.0, seed=0, name="x", dtype=BF16)
    with torch.no_grad():
        ad.A.copy_(a)
        ad.B.copy_(b)
    m = ML.merged_weight(w, ad)
    assert torch.equal(D.merged(w, ad), m) and torch.equal(D.merged(w, (a, b, ad.scale)), m)
    w1 = w.clone()
    assert torch.equal(D.tiled_weight(w1, lora=ad), _torch_tile(m))
    assert torch.equal(D.folded_weight(w1, nw, tiled=True, lora=ad), _torch_tile(m * nw.view(1, -1)))
    assert torch.equal(D.folded_weight(w1, nw, tiled=True, glu_il=True, lora=(a, b, ad.scale)),
                       _torch_tile(D._glu_interleave(m * nw.view(1, -1))))
    for nwx, glu_il in ((None, False), (nw, False), (nw, True)):
        src = m if nwx is None else m * nwx.view(1, -1)
        q, sc = D.quantize_rows_f8(D._glu_interleave(src) if glu_il else src)
        t8, s8 = D.fp8_tiled_weight(w1, nwx, glu_il=glu_il, lora=ad)
        assert torch.equal(t8, D.tile_f8(q)) and torch.equal(s8, sc)
    with pytest.raises(ValueError):
        D.folded_weight(w1, nw, lora=ad)  # the row-major copy has no merged form


def test_cache_key_follows_the_adapter_and_storage_stays():
    N, K = 32, 64
    w, a, b, nw = RR.random_case(N, K, 8, seed=1, with_nw=True)
    t0 = D.folded_weight(w, nw, tiled=True)
    base = t0.clone()
    ptr = t0.data_ptr()
    t1 = D.folded_weight(w, nw, tiled=True, lora=(a, b, 2.0))
    assert t1.data_ptr() == ptr and not torch.equal(t1, base)
    merged1 = t1.clone()
    b.mul_(2)  # an in-place update of B is noticed (version counter)
    t2 = D.folded_weight(w, nw, tiled=True, lora=(a, b, 2.0))
    assert t2.data_ptr() == ptr and not torch.equal(t2, merged1)
    t3 = D.folded_weight(w, nw, tiled=True, lora=(a, b, 1.0))  # so is another scale
    assert not torch.equal(t3.clone(), D.folded_weight(w, nw, tiled=True, lora=(a, b, 2.0)))
    assert torch.equal(D.folded_weight(w, nw, tiled=True), base) and D.folded_weight(w, nw, tiled=True).data_ptr() == ptr
    assert list(w.__dict__) == ["_dla_fold_t"]  # no second set of copies

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(w)

    h = Holder()
    h.p._dla_fold_t = w._dla_fold_t
    assert D.drop_derived_weights(h) == N * K * 2


def test_merged_scope():
    assert not D.lora_merged_enabled()
    with D.lora_merged(True):
        assert D.lora_merged_enabled()
        with D.lora_merged(False):
            assert not D.lora_merged_enabled()
        assert D.lora_merged_enabled()
    assert not D.lora_merged_enabled()


# ------------------------------------------------------------------------------ generate
def _tiny(seed=0):
    m = build_model(get_config("tiny-llama"), device="cpu", dtype=torch.float32, seed=seed)
    ML.apply_lora(m, r=8, alpha=16, seed=3)
    for i, ad in enumerate(ML.lora_adapters(m)):
        g = torch.Generator().manual_seed(50 + i)
        with torch.no_grad():
            ad.B.copy_(torch.randn(ad.B.shape, generator=g) * 0.1)
    return m


def test_generate_merged_on_cpu_is_the_live_adapter_forward():
    m = _tiny().eval()
    cfg = m.cfg
    ids = torch.randint(3, cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(2))
    out = generate(m, ids, None, max_new_tokens=6, do_sample=False, eos_token_id=-1, adapters="merged")
    x = ids
    with torch.no_grad():
        for _ in range(6):  # the full live-adapter forward's greedy continuation, no cache
            x = torch.cat([x, m.logits(m(x)[:, -1]).argmax(-1, keepdim=True)], 1)
    assert torch.equal(out, x)
    with ML.lora_disabled(m):
        off = generate(m, ids, None, max_new_tokens=6, do_sample=False, eos_token_id=-1)
        assert torch.equal(off, generate(m, ids, None, max_new_tokens=6, do_sample=False, eos_token_id=-1,
                                         adapters="merged"))  # nothing active: today's call
    assert not torch.equal(off, out), "the adapters do not move this model: the test shows nothing"


def test_generate_adapter_argument():
    m = _tiny()
    ids = torch.randint(3, m.cfg.vocab_size, (2, 5), generator=torch.Generator().manual_seed(3))
    with pytest.raises(ValueError, match="LoRA"):
        generate(m, ids, None, max_new_tokens=2)
    with pytest.raises(ValueError, match="adapters"):
        generate(m, ids, None, max_new_tokens=2, adapters="bogus")
    plain = build_model(get_config("tiny-llama"), device="cpu", dtype=torch.float32, seed=0)
    with pytest.raises(ValueError, match="adapters"):
        generate(plain, ids, None, max_new_tokens=2, adapters="live")
    a = generate(plain, ids, None, max_new_tokens=3, do_sample=False, eos_token_id=-1)
    assert torch.equal(a, generate(plain, ids, None, max_new_tokens=3, do_sample=False, eos_token_id=-1,
                                   adapters="merged"))


# ------------------------------------------------------------------------------ train_rlhf
LORA = {"enabled": True, "r": 8, "alpha": 16, "target_modules": ["qkv", "o", "up", "down"]}


def _cfg(tmp, name, body):
    p = Path(tmp) / f"{name}.yaml"
    p.write_text(yaml.safe_dump(body))
    return str(p)


def _body(d, tag, algo, lora=True, ref=None, **ppo):
    write_jsonl(d / "prompts.jsonl", synthetic_prompt_records(8, seed=4))
    model = {"policy_model_name_or_path": "tiny-llama", "max_seq_length": 64}
    if lora:
        model["lora"] = dict(LORA)
    if ref:
        model["reference_model_name_or_path"] = ref
    return {"seed": 5, "model": model, "reward_model": {"base_model_name_or_path": "tiny-llama"},
            "ppo": {"algorithm": algo, "batch_size": 4, "group_size": 2, "learning_rate": 1e-2, "kl_coef": 0.05,
                    "steps": 2, "rollout_logprobs": "monitor",
                    "generation_params": {"max_new_tokens": 5, "temperature": 0.8}, **ppo},
            "sampling": {"source": "local", "prompt_path": str(d / "prompts.jsonl")},
            "logging": {"output_dir": str(d / "ck" / tag), "log_dir": str(d / "logs" / tag), "log_every_steps": 1}}


def _spy(monkeypatch, train_rlhf):
    """Record what main() builds: the policy after apply_lora (with a snapshot of its tensors), the
    reference handed to the rollout statistics, the models handed to save_state, the generate kwargs."""
    seen = {"refs": [], "adapters": []}
    real_apply, real_save, real_gen = train_rlhf.maybe_apply_lora, train_rlhf.save_state, train_rlhf.generate

    def apply(ctx, model, base=None):
        out = real_apply(ctx, model, base)
        seen["policy"] = model
        seen["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
        return out

    def save(out_dir, models, *a, **k):
        seen["saved"] = list(models)
        return real_save(out_dir, models, *a, **k)

    def gen(model, *a, **k):
        seen["adapters"].append(k.get("adapters"))
        return real_gen(model, *a, **k)

    for name in ("grpo_rollout_stats", "ppo_rollout_stats"):
        real = getattr(train_rlhf, name)

        def stats(policy, ref, *a, _real=real, **k):
            seen["refs"].append(ref)
            return _real(policy, ref, *a, **k)

        monkeypatch.setattr(train_rlhf, name, stats)
    monkeypatch.setattr(train_rlhf, "maybe_apply_lora", apply)
    monkeypatch.setattr(train_rlhf, "save_state", save)
    monkeypatch.setattr(train_rlhf, "generate", gen)
    return seen


@pytest.mark.parametrize("algo", ["grpo", "ppo"])
def test_rlhf_with_lora_and_the_shared_reference(tmp_path, monkeypatch, algo):
    from safetensors.torch import load_file

    from distributed_llm_alignment_amd.training import train_rlhf

    seen = _spy(monkeypatch, train_rlhf)
    d = tmp_path
    assert train_rlhf.main(["--config", _cfg(d, algo, _body(d, algo, algo))]) == 0
    policy = seen["policy"]
    assert ML.has_lora(policy)
    moved = 0
    for n, p in policy.named_parameters():
        if ".lora_" in n:
            moved += int(not torch.equal(p.detach(), seen["before"][n]))
        else:
            assert torch.equal(p.detach(), seen["before"][n]), f"base tensor {n} changed"
    assert moved >= len(ML.lora_adapters(policy)), "A / B did not move"  # every B leaves zero
    # no second policy: the reference is the policy with its adapters off
    assert seen["refs"] and all(isinstance(r, ML.LoRAReference) for r in seen["refs"])
    assert all(r._model is policy for r in seen["refs"])
    assert len(seen["saved"]) == (3 if algo == "ppo" else 2) and seen["saved"][0] is policy
    assert seen["adapters"] and all(a == "merged" for a in seen["adapters"])
    ck = d / "ck" / algo
    assert (ck / "adapter.safetensors").exists() and (ck / "model.safetensors").exists()
    assert (ck / "model_1.safetensors").exists()  # the reward model
    assert (ck / "model_2.safetensors").exists() == (algo == "ppo")  # the critic; never a reference
    assert not (ck / f"model_{3 if algo == 'ppo' else 2}.safetensors").exists()
    ad = load_file(str(ck / "adapter.safetensors"))
    assert any(k.endswith(".B") and v.abs().sum() > 0 for k, v in ad.items())
    rows = [json.loads(l) for l in (d / "logs" / algo / "metrics.jsonl").read_text().splitlines()]
    assert any("train/rollout_kl" in r for r in rows)


def test_rlhf_with_lora_and_a_separate_reference(tmp_path, monkeypatch):
    from distributed_llm_alignment_amd.training import train_rlhf

    seen = _spy(monkeypatch, train_rlhf)
    d = tmp_path
    body = _body(d, "sep", "grpo", ref="tiny-llama-d128")
    assert train_rlhf.main(["--config", _cfg(d, "sep", body)]) == 0
    assert seen["refs"] and not any(isinstance(r, ML.LoRAReference) for r in seen["refs"])
    assert len(seen["saved"]) == 3 and (d / "ck" / "sep" / "model_2.safetensors").exists()


def test_rlhf_without_lora_is_the_run_it_was(tmp_path, monkeypatch):
    from distributed_llm_alignment_amd.training import train_rlhf

    seen = _spy(monkeypatch, train_rlhf)
    d = tmp_path
    body = _body(d, "off", "grpo", lora=False, ref="tiny-llama")
    assert train_rlhf.main(["--config", _cfg(d, "off", body)]) == 0
    assert not ML.has_lora(seen["policy"]) and all(a is None for a in seen["adapters"])
    assert len(seen["saved"]) == 3 and not (d / "ck" / "off" / "adapter.safetensors").exists()
    assert not any(isinstance(r, ML.LoRAReference) for r in seen["refs"])


def test_rlhf_lora_refusals(tmp_path):
    from distributed_llm_alignment_amd.training import train_rlhf

    d = tmp_path
    with pytest.raises(ValueError, match="RLHF.*grpo and ppo"):
        train_rlhf.main(["--config", _cfg(d, "r", _body(d, "r", "reinforce", rollout_logprobs="off"))])
    with pytest.raises(ValueError, match="frozen_fp8"):
        train_rlhf.main(["--config", _cfg(d, "f", _body(d, "f", "grpo", frozen_fp8=True))])
    with pytest.raises(ValueError, match="frozen_fp8"):  # the policy's own path is the shared reference too
        train_rlhf.main(["--config", _cfg(d, "g", _body(d, "g", "ppo", ref="tiny-llama", frozen_fp8=True))])


def test_shipped_grpo_lora_config():
    root = Path(__file__).resolve().parents[1] / "config"
    cfg = yaml.safe_load((root / "rlhf_grpo_lora_llama3_8b.yaml").read_text())
    assert ML.lora_config(cfg["model"])["enabled"] is True and "reference_model_name_or_path" not in cfg["model"]
    assert cfg["ppo"]["algorithm"] == "grpo" and cfg["ppo"]["rollout_logprobs"] == "monitor"
    base = yaml.safe_load((root / "rlhf_grpo_llama3_8b.yaml").read_text())
    assert {k: v for k, v in cfg["ppo"].items() if k != "rollout_logprobs"} == \
        {k: v for k, v in base["ppo"].items() if k != "rollout_logprobs"}


def test_engine_epoch_on_the_adapter_parameters_moves_the_key():
    """An engine-owned parameter is updated by a fused kernel that moves no version counter; the
    engine bumps `_dla_epoch` instead. The merged copy must follow it (the key is read off the
    parameter objects, not off detached views)."""
    N, K = 32, 64
    w, a, b, nw = RR.random_case(N, K, 8, seed=2, with_nw=True)
    ad = ML.LoRAAdapter(K, N, 8, 16, 0.0, seed=0, name="x", dtype=BF16)
    with torch.no_grad():
        ad.A.copy_(a)
        ad.B.copy_(b)
    ad.A._dla_epoch = ad.B._dla_epoch = [0]
    t = D.tiled_weight(w, lora=ad)
    before, ver = t.clone(), ad.B._version
    ad.B.data.mul_(2)  # what the optimizer kernel does: new values, same version
    assert ad.B._version == ver
    assert torch.equal(D.tiled_weight(w, lora=ad), before)  # nothing told the cache yet
    ad.B._dla_epoch[0] += 1
    after = D.tiled_weight(w, lora=ad)
    assert after.data_ptr() == t.data_ptr() and not torch.equal(after, before)
    assert torch.equal(after, _torch_tile(ML.merged_weight(w, ad)))
