"""CPU tier: LoRA adapters (ops/lora.py, models/lora.py, the trainers and the checkpoint files).

Bounds. The formula of record against fp64: `_refs64.check` with E32 = the error of the
un-rounded fp32 composition and one bf16 ulp for the bf16 output. Merging: W' = W + s B A is
formed in fp32 and rounded once, so W' is within half an ulp (of W's dtype) of the fp64 sum, and
the merged model's logits / loss equal the adapter model's within one bf16 ulp of the reference
value (the CPU models are fp32, whose merge error is 2^-16 of that allowance).
"""
import json
import math
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
import yaml

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import (synthetic_instruction_records,
                                                          synthetic_preference_records)
from distributed_llm_alignment_amd.models import build_model, get_config, load_causal_lm
from distributed_llm_alignment_amd.models import lora as ML
from distributed_llm_alignment_amd.models.loader import count_trainable_params
from distributed_llm_alignment_amd.ops import lora as L

import _refs64 as R
import _refs64_lora as RL

BF16 = torch.bfloat16


def _tiny(seed=0, name="tiny-llama"):
    return build_model(get_config(name), seed=seed)


# ------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("mode", ["plain", "bias", "resid"])
def test_formula_of_record_against_fp64(mode):
    c = RL.full_case(33, 40, 24, 8, seed=1, with_bias=mode == "bias", with_resid=mode == "resid")
    scale = 2.0
    y = L.lora_linear(c["x"], c["w"], c["a"], c["b"], scale, bias=c["bias"], resid=c["resid"])
    assert y.dtype == BF16
    # the two pieces, each against fp64 with its own input as given
    t = L.lora_shrink(c["x"], c["a"], scale)
    ref_t = RL.shrink64(c["x"], c["a"], scale)
    R.check("lora_cpu", f"{mode} t", t, ref_t, R.e32_of(scale * (c["x"].float() @ c["a"].float().t()), ref_t),
            bf16=True)
    y0 = F.linear(c["x"], c["w"], c["bias"]) if c["resid"] is None else torch.addmm(c["resid"], c["x"], c["w"].t())
    ref_y = RL.expand64(y0, t, c["b"])
    R.check("lora_cpu", f"{mode} y", y, ref_y, R.e32_of(y0.float() + t.float() @ c["b"].float().t(), ref_y),
            bf16=True)
    want = (y0.float() + t.float() @ c["b"].float().t()).to(BF16)
    assert torch.equal(y, want), "the CPU branch is not the formula of record"


def test_gradients_against_fp64():
    """fp32 tensors: no rounding of t / dts, so the gradients are the plain derivatives."""
    c = {k: (v.float() if v is not None else None) for k, v in RL.full_case(17, 40, 24, 8, seed=2, with_resid=True).items()}
    x, r = c["x"].clone().requires_grad_(True), c["resid"].clone().requires_grad_(True)
    A, B = torch.nn.Parameter(c["a"]), torch.nn.Parameter(c["b"])
    y = L.lora_linear(x, c["w"], A, B, 2.0, resid=r)
    ref = RL.full64(c["x"], c["w"], c["a"], c["b"], 2.0, resid=c["resid"])
    y.backward(c["dy"])
    g = RL.full_grads64(c["x"], c["w"], c["a"], c["b"], 2.0, c["dy"])
    # every output is a sum of products: the same formulas on the absolute values give, per
    # element, the sum of |terms| that the fp32 error of a (nested) dot product is relative to.
    # The longest chain sums K + R terms (y, dx) or M + N terms (dA); gamma_n with n = their total.
    ab = {k: v.abs() for k, v in c.items() if v is not None}
    sums = RL.full_grads64(ab["x"], ab["w"], ab["a"], ab["b"], 2.0, ab["dy"])
    sums["y"] = RL.full64(ab["x"], ab["w"], ab["a"], ab["b"], 2.0, resid=ab["resid"])
    n_terms = 40 + 24 + 17 + 8
    for name, got, want in (("y", y, ref), ("dx", x.grad, g["dx"]), ("dA", A.grad, g["dA"]), ("dB", B.grad, g["dB"]),
                            ("dresid", r.grad, g["dresid"])):
        err = (got.double() - want).abs().max().item()
        bound = RL.dot_extra(n_terms, sums[name].max().item())
        print(f"FIG lora_cpu grads {name}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, name


def test_b_zero_is_the_base_projection_bitwise():
    c = RL.full_case(33, 40, 24, 16, seed=3, with_resid=True)
    zb = torch.zeros_like(c["b"])
    y = L.lora_linear(c["x"], c["w"], c["a"], zb, 2.0)
    assert torch.equal(y, ops.linear(c["x"], c["w"]))
    y = L.lora_linear(c["x"], c["w"], c["a"], zb, 2.0, resid=c["resid"])
    assert torch.equal(y, ops.linear_add(c["x"], c["w"], c["resid"]))


def test_dropout_feeds_the_adapter_branch_only():
    c = {k: (v.float() if v is not None else None) for k, v in RL.full_case(9, 16, 8, 4, seed=4).items()}
    torch.manual_seed(0)
    y = L.lora_linear(c["x"], c["w"], c["a"], c["b"], 2.0, dropout=0.5, training=True)
    torch.manual_seed(0)
    xd = F.dropout(c["x"], 0.5, training=True)
    want = F.linear(c["x"], c["w"]) + F.linear(2.0 * F.linear(xd, c["a"]), c["b"])
    assert torch.allclose(y, want, atol=1e-6)
    # eval mode: no dropout, the kernel-served function
    y_eval = L.lora_linear(c["x"], c["w"], c["a"], c["b"], 2.0, dropout=0.5, training=False)
    assert torch.equal(y_eval, L.lora_linear(c["x"], c["w"], c["a"], c["b"], 2.0))


# ------------------------------------------------------------------------------ the model
def test_apply_lora_keeps_and_freezes_the_base():
    plain, m = _tiny(), _tiny()
    stats = ML.apply_lora(m, r=16, alpha=32, seed=5)
    base = [(n, p) for n, p in m.named_parameters() if ".lora_" not in n]
    assert [n for n, _ in base] == [n for n, _ in plain.named_parameters()]
    for (n, p), (_, q) in zip(base, plain.named_parameters()):
        assert torch.equal(p, q), f"{n} changed by apply_lora"
        assert not p.requires_grad, f"{n} not frozen"
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable and all(".lora_" in n and n.endswith((".A", ".B")) for n in trainable)
    cfg = m.cfg
    H, Fd, qkv = cfg.hidden_size, cfg.intermediate_size, cfg.q_size + 2 * cfg.kv_size
    per_layer = 16 * ((H + qkv) + (cfg.q_size + H) + (H + 2 * Fd) + (Fd + H))
    print(f"tiny-llama LoRA r=16: {stats}")
    assert stats["trainable_params"] == cfg.num_layers * per_layer == count_trainable_params(m)["trainable_params"]
    assert stats["total_params"] == sum(p.numel() for p in plain.parameters()) + stats["trainable_params"]
    assert 0.0 < stats["trainable_ratio"] < 0.2


def test_adapter_init_is_seeded_by_name_not_order():
    m1, m2 = _tiny(), _tiny()
    ML.apply_lora(m1, r=8, seed=7, target_modules=["qkv", "o", "up", "down"])
    ML.apply_lora(m2, r=8, seed=7, target_modules=["down", "qkv"])
    sd1, sd2 = ML.adapter_state_dict(m1), ML.adapter_state_dict(m2)
    assert set(sd2) < set(sd1)
    for k, v in sd2.items():
        assert torch.equal(v, sd1[k]), k
    a = sd1["layers.0.attn.lora_qkv.A"]
    assert a.abs().max() <= 1.0 / math.sqrt(m1.cfg.hidden_size) and a.abs().max() > 0
    assert all(torch.count_nonzero(v) == 0 for k, v in sd1.items() if k.endswith(".B"))
    m3 = _tiny()
    ML.apply_lora(m3, r=8, seed=8)
    assert not torch.equal(ML.adapter_state_dict(m3)["layers.0.attn.lora_qkv.A"], a)


def _randomize_b(m, seed=0, std=0.05):
    g = torch.Generator().manual_seed(seed)
    for ad in ML.lora_adapters(m):
        ad.B.data.copy_(torch.randn(ad.B.shape, generator=g) * std)


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-gpt2", "tiny-phi"])
def test_lora_disabled_and_reference(name):
    plain, m = _tiny(name=name), _tiny(name=name)
    ML.apply_lora(m, r=8, seed=1)
    ids = torch.randint(0, m.cfg.vocab_size, (2, 19), generator=torch.Generator().manual_seed(0))
    h0 = plain(ids)
    assert torch.equal(m(ids), h0), "B == 0: the adapter model is the base model"
    _randomize_b(m)
    h1 = m(ids)
    assert (h1 - h0).abs().max() > 1e-3
    with ML.lora_disabled(m):
        assert torch.equal(m(ids), h0)
    assert torch.equal(m(ids), h1), "lora_disabled did not restore the adapters"
    ref = ML.LoRAReference(m)
    out = ref(ids)
    assert torch.equal(out, h0) and not out.requires_grad
    assert torch.equal(ref.sequence_logprob(ids, None, "mean"), plain.sequence_logprob(ids, None, "mean"))
    assert torch.equal(ref.token_logprobs(ids), plain.token_logprobs(ids))
    assert ref.cfg is m.cfg and next(ref.parameters()) is next(m.parameters())
    # every target receives a gradient; the base receives none
    m.causal_lm_loss(ids, ids).backward()
    for n, p in m.named_parameters():
        assert (p.grad is not None and p.grad.abs().sum() > 0) == (".lora_" in n), n


def test_merge_lora():
    m = _tiny()
    ML.apply_lora(m, r=8, alpha=16, seed=2)
    _randomize_b(m)
    ids = torch.randint(0, m.cfg.vocab_size, (2, 19), generator=torch.Generator().manual_seed(1))
    import copy

    # the fp64 merged reference: the same model in fp64 with W + s B A folded in fp64
    ref64 = copy.deepcopy(m).double()
    for _, owner, wname, aname in list(ML.lora_sites(ref64)):
        ad64 = getattr(owner, aname)
        getattr(owner, wname).data += ad64.scale * (ad64.B.data @ ad64.A.data)
        setattr(owner, aname, None)
    with torch.no_grad():
        lg_ref = ref64.logits(ref64(ids))
        lg_adapter = m.logits(m(ids)).double()
    assert lg_ref.dtype == torch.float64
    w = m.layers[0].attn.qkv_proj.detach().clone()
    ad = m.layers[0].attn.lora_qkv
    ref_w = w.double() + ad.scale * (ad.B.detach().double() @ ad.A.detach().double())
    ML.merge_lora(m)
    assert not ML.has_lora(m) and all(p.requires_grad for p in m.parameters())
    # fp32 weights: one rounding of the fp64 sum (half an fp32 ulp, plus the fp32 product's own error)
    err = (m.layers[0].attn.qkv_proj.double() - ref_w).abs().max().item()
    assert err <= 4 * RL.EPS32 * ref_w.abs().max().item(), err
    with torch.no_grad():
        lg_merged = m.logits(m(ids)).double()
    # one bf16 ulp of the fp64 merged reference, plus the fp32 arithmetic of the forward itself
    # (E32 = the un-merged fp32 model's own distance from that reference: near-zero logits have a
    # bf16 ulp below it)
    R.check("lora_cpu", "merged logits", lg_merged, lg_ref, R.e32_of(lg_adapter, lg_ref), bf16=True)
    # bf16 weights: W' is the fp64 sum rounded once
    wb = RL.rand_bf16((24, 40), 5)
    adb = ML.LoRAAdapter(40, 24, 8, 16, 0.0, seed=0, name="x", dtype=BF16)
    adb.B.data.copy_(RL.rand_bf16((24, 8), 6, amp=0.1))
    ref = wb.double() + adb.scale * (adb.B.detach().double() @ adb.A.detach().double())
    got = ML.merged_weight(wb, adb)
    assert got.dtype == BF16
    assert ((got.double() - ref).abs() <= 0.5 * R.bf16_ulp(ref) + 8 * RL.EPS32 * ref.abs()).all()


# ------------------------------------------------------------------------------ refusals
def test_refusals():
    with pytest.raises(ValueError, match="MoE"):
        ML.apply_lora(_tiny(name="tiny-mixtral"))
    for attr, val, word in (("tp", object(), "tensor"), ("sp", object(), "sequence"), ("ep_size", 2, "expert"),
                            ("layer_devices", ["cpu", "cpu"], "layer_split"), ("_dla_fsdp", object(), "ZeRO-3")):
        m = _tiny()
        setattr(m, attr, val)
        with pytest.raises(ValueError, match=word):
            ML.apply_lora(m)
    m = _tiny()
    m.layers[1].attn.tp = object()
    with pytest.raises(ValueError, match="parallelism"):
        ML.apply_lora(m)
    m = _tiny()
    ML.apply_lora(m, r=4)
    with pytest.raises(ValueError, match="already"):
        ML.apply_lora(m, r=4)
    from distributed_llm_alignment_amd.models.generation import generate

    ids = torch.randint(0, m.cfg.vocab_size, (1, 5))
    with pytest.raises(ValueError, match="generate"):
        generate(m, ids, max_new_tokens=2)
    ML.merge_lora(m)
    assert generate(m, ids, max_new_tokens=2, do_sample=False).shape[1] > 5
    with pytest.raises(ValueError, match="adapters"):
        ML.LoRAReference(_tiny())
    c = RL.full_case(3, 8, 8, 4)
    with pytest.raises(ValueError, match="frozen"):
        L.lora_linear(c["x"], c["w"].clone().requires_grad_(True), c["a"], c["b"], 1.0)
    with pytest.raises(ValueError, match="shapes"):
        L.lora_linear(c["x"], c["w"], c["a"][:, :4], c["b"], 1.0)


@pytest.mark.parametrize("block", [{"rank": 8}, {"r": 0}, {"r": 300}, {"r": 8.5}, {"alpha": 0}, {"dropout": 1.0},
                                   {"target_modules": ["q"]}, {"target_modules": []}, {"target_modules": "qkv"},
                                   {"enabled": "yes"}, {"save_merged": 1}, {"target_modules": ["o", "o"]}])
def test_config_refusals(block):
    with pytest.raises(ValueError):
        ML.lora_config({"lora": block})


def test_config_defaults():
    assert ML.lora_config(None) == ML.lora_config({}) == {"enabled": False, "r": 16, "alpha": 32, "dropout": 0.0,
                                                          "target_modules": ["qkv", "o", "up", "down"],
                                                          "save_merged": True}
    assert ML.lora_config({"lora": {"enabled": True, "r": 12}})["r"] == 12
    root = Path(__file__).resolve().parent.parent / "config"
    for name in ("sft_config.yaml", "dpo_config.yaml", "reward_config.yaml", "distill_config.yaml"):
        assert ML.lora_config(yaml.safe_load((root / name).read_text())["model"])["enabled"] is False, name
    cfg = yaml.safe_load((root / "dpo_lora_llama3_8b.yaml").read_text())["model"]
    assert ML.lora_config(cfg)["enabled"] is True and "reference_model_name_or_path" not in cfg


# ------------------------------------------------------------------------------ trainers
def _cfg(tmp, name, body):
    p = Path(tmp) / f"{name}.yaml"
    p.write_text(yaml.safe_dump(body))
    return str(p)


def _metrics(log_dir):
    return [json.loads(l) for l in (Path(log_dir) / "metrics.jsonl").read_text().splitlines()]


def _dirs(tmp, tag, **logging):
    return {"logging": {"output_dir": str(Path(tmp) / "ck" / tag), "log_dir": str(Path(tmp) / "logs" / tag),
                        "log_every_steps": 1, **logging},
            "hardware": {"gradient_accumulation_steps": 1}}


LORA = {"enabled": True, "r": 8, "alpha": 16, "target_modules": ["qkv", "o", "up", "down"]}


def test_sft_trainer_with_lora(tmp_path):
    from safetensors.torch import load_file

    from distributed_llm_alignment_amd.training import train_sft

    d = tmp_path
    write_jsonl(d / "sft.jsonl", synthetic_instruction_records(16, seed=1))
    body = {"seed": 11, "model": {"model_name_or_path": "tiny-llama", "max_seq_length": 96,
                                  "gradient_checkpointing": True, "lora": dict(LORA)},
            "data": {"source": "local", "train_path": str(d / "sft.jsonl"), "num_workers": 0},
            "optimization": {"micro_batch_size": 2, "learning_rate": 5e-3, "warmup_steps": 0, "max_train_steps": 3,
                             "lr_scheduler": "constant"}}
    assert train_sft.main(["--config", _cfg(d, "a", {**body, **_dirs(d, "a", save_every_steps=2)})]) == 0
    losses = {r["step"]: r["train/loss"] for r in _metrics(d / "logs" / "a") if "train/loss" in r}
    assert set(losses) >= {1, 2, 3} and all(math.isfinite(v) for v in losses.values())
    ck = d / "ck" / "a" / "step_2"
    for f in ("adapter.safetensors", "adapter_config.json", "model.safetensors", "hf/model.safetensors",
              "hf/config.json", "optimizer_shard_0.safetensors", "random_states_0.pkl"):
        assert (ck / f).exists(), f
    acfg = json.loads((ck / "adapter_config.json").read_text())
    assert acfg["r"] == 8 and acfg["alpha"] == 16 and acfg["target_modules"] == LORA["target_modules"]
    assert acfg["base_model_name_or_path"] == "tiny-llama"

    # a fresh base + freshly initialised adapters: what the run started from
    fresh = load_causal_lm("tiny-llama", device="cpu", seed=11).model
    base0 = {n: p.detach().clone() for n, p in fresh.named_parameters()}
    ML.apply_lora(fresh, r=8, alpha=16, seed=11)
    init = {k: v.clone() for k, v in ML.adapter_state_dict(fresh).items()}
    saved = load_file(str(ck / "adapter.safetensors"))
    assert set(saved) == set(init)
    for k in saved:  # adapters changed: B left zero, A left its init
        assert not torch.equal(saved[k], init[k]), f"{k} did not train"
    # the files hold MERGED weights: base (bitwise the seeded one) + scale * B A, rounded once
    ML.load_adapter_state_dict(fresh, saved)
    for n, p in fresh.named_parameters():
        if ".lora_" not in n:
            assert torch.equal(p, base0[n]), f"base weight {n} changed"
    merged = load_causal_lm(str(ck / "hf"), device="cpu", seed=0).model
    assert not ML.has_lora(merged)
    mp = dict(merged.named_parameters())
    adapted = set()
    for name, owner, wname, aname in ML.lora_sites(fresh):
        wn = name.rsplit(".", 1)[0] + "." + wname
        adapted.add(wn)
        assert torch.equal(mp[wn], ML.merged_weight(getattr(owner, wname), getattr(owner, aname))), wn
    for n, p in base0.items():
        if n not in adapted:
            assert torch.equal(mp[n], p), f"untargeted weight {n} differs in the export"
    # the export as a plain model: same loss as the adapter model within the merge bound
    ids = torch.randint(0, fresh.cfg.vocab_size, (2, 24), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        la, lm_ = fresh.causal_lm_loss(ids, ids).double(), merged.causal_lm_loss(ids, ids).double()
    print(f"FIG lora_cpu sft export: adapter loss {la.item():.7f} merged loss {lm_.item():.7f}")
    assert (la - lm_).abs() <= R.bf16_ulp(la)

    # resume from step 2: step 3's loss is reproduced exactly
    assert train_sft.main(["--config", _cfg(d, "b", {**body, **_dirs(d, "b")}), "--resume", str(ck)]) == 0
    resumed = {r["step"]: r["train/loss"] for r in _metrics(d / "logs" / "b") if "train/loss" in r}
    assert set(resumed) == {3}
    assert resumed[3] == losses[3], (resumed[3], losses[3])


def test_sft_trainer_adapters_only_checkpoint(tmp_path):
    from distributed_llm_alignment_amd.training import train_sft

    d = tmp_path
    write_jsonl(d / "sft.jsonl", synthetic_instruction_records(8, seed=1))
    body = {"seed": 11, "model": {"model_name_or_path": "tiny-llama", "max_seq_length": 96,
                                  "lora": dict(LORA, save_merged=False)},
            "data": {"source": "local", "train_path": str(d / "sft.jsonl"), "num_workers": 0},
            "optimization": {"micro_batch_size": 2, "learning_rate": 5e-3, "max_train_steps": 2}}
    assert train_sft.main(["--config", _cfg(d, "a", {**body, **_dirs(d, "a")})]) == 0
    ck = d / "ck" / "a" / "final"
    assert (ck / "adapter.safetensors").exists() and (ck / "optimizer_shard_0.safetensors").exists()
    assert (ck / "random_states_0.pkl").exists()
    assert not (ck / "model.safetensors").exists() and not (ck / "hf").exists()


def test_dpo_trainer_with_shared_reference(tmp_path):
    from distributed_llm_alignment_amd.training import train_dpo

    d = tmp_path
    write_jsonl(d / "pref.jsonl", synthetic_preference_records(16, seed=3))
    body = {"seed": 5, "model": {"policy_model_name_or_path": "tiny-llama", "beta": 0.1, "max_seq_length": 96,
                                 "gradient_checkpointing": False, "lora": dict(LORA)},
            "data": {"preference_path": str(d / "pref.jsonl"), "num_workers": 0},
            "optimization": {"micro_batch_size": 2, "learning_rate": 1e-2, "max_train_steps": 3}}
    assert train_dpo.main(["--config", _cfg(d, "a", {**body, **_dirs(d, "a", eval_every_steps=1)})]) == 0
    recs = [r for r in _metrics(d / "logs" / "a") if "train/loss" in r]
    # step 0: B == 0, the policy IS the reference, so the loss is -logsigmoid(0) = log 2 exactly
    log2 = float(-F.logsigmoid(torch.zeros((), dtype=torch.float32)))
    assert abs(log2 - math.log(2.0)) < 1e-7
    assert recs[0]["step"] == 1 and recs[0]["train/loss"] == log2, recs[0]["train/loss"]
    assert all(math.isfinite(r["train/reward_accuracy"]) and 0.0 <= r["train/reward_accuracy"] <= 1.0 for r in recs)
    assert recs[-1]["train/loss"] != log2, "the adapters did not move the policy"
    ck = d / "ck" / "a" / "final"
    assert (ck / "model.safetensors").exists() and (ck / "adapter.safetensors").exists()
    assert not (ck / "model_1.safetensors").exists() and not (ck / "adapter_1.safetensors").exists()
    assert json.loads((ck / "dla_state.json").read_text())["num_models"] == 1
    # the same path given as reference is still the shared one; fp8 with it is refused
    both = {**body, "model": dict(body["model"], reference_model_name_or_path="tiny-llama", reference_fp8=True)}
    with pytest.raises(ValueError, match="reference_fp8"):
        train_dpo.main(["--config", _cfg(d, "b", {**both, **_dirs(d, "b")})])


def test_reward_trainer_with_lora_keeps_the_head_trainable(tmp_path):
    from safetensors.torch import load_file

    from distributed_llm_alignment_amd.training import train_reward

    d = tmp_path
    write_jsonl(d / "pref.jsonl", synthetic_preference_records(8, seed=3))
    body = {"model": {"base_model_name_or_path": "tiny-llama", "pooling": "last_token", "dropout": 0.0,
                      "max_seq_length": 96, "lora": dict(LORA, target_modules=["qkv", "down"])},
            "data": {"source": "local", "train_path": str(d / "pref.jsonl"), "num_workers": 0},
            "optimization": {"micro_batch_size": 2, "learning_rate": 1e-2, "max_train_steps": 2}}
    assert train_reward.main(["--config", _cfg(d, "a", {**body, **_dirs(d, "a")})]) == 0
    ck = d / "ck" / "a" / "final"
    sd = load_file(str(ck / "adapter.safetensors"))
    head = {"scorer.1.weight", "scorer.1.bias"}
    assert head < set(sd), "the trained score head is not in the adapter file"
    assert all(k.startswith("backbone.layers.") and (".lora_qkv." in k or ".lora_down." in k)
               for k in set(sd) - head)
    assert any(torch.count_nonzero(v) > 0 for k, v in sd.items() if k.endswith(".B"))
    assert (ck / "model.safetensors").exists()


def test_reward_trainer_resume_restores_head_and_is_exact(tmp_path):
    """The score head trains next to the adapters; resume must bring both back: the next step's loss
    is reproduced exactly, with merged weights and with `save_merged: false` (adapter files only)."""
    from safetensors.torch import load_file

    from distributed_llm_alignment_amd.models.loader import build_reward_model
    from distributed_llm_alignment_amd.training import train_reward
    from distributed_llm_alignment_amd.utils.checkpoint import load_state

    d = tmp_path
    write_jsonl(d / "pref.jsonl", synthetic_preference_records(16, seed=3))
    for tag, merged in (("m", True), ("a", False)):
        body = {"seed": 9, "model": {"base_model_name_or_path": "tiny-llama", "pooling": "last_token",
                                     "dropout": 0.0, "max_seq_length": 96,
                                     "lora": dict(LORA, save_merged=merged)},
                "data": {"source": "local", "train_path": str(d / "pref.jsonl"), "num_workers": 0},
                "optimization": {"micro_batch_size": 2, "learning_rate": 1e-2, "max_train_steps": 3}}
        assert train_reward.main(["--config", _cfg(d, tag, {**body, **_dirs(d, tag, save_every_steps=2)})]) == 0
        losses = {r["step"]: r["train/loss"] for r in _metrics(d / "logs" / tag) if "train/loss" in r}
        ck = d / "ck" / tag / "step_2"
        assert (ck / "model.safetensors").exists() == merged
        sd = load_file(str(ck / "adapter.safetensors"))
        # a fresh model as the trainer builds it, then the checkpoint: the trained head comes back
        rm, _ = build_reward_model("tiny-llama", pooling="last_token", dropout=0.0, device="cpu", seed=9)
        ML.apply_lora(rm, r=8, alpha=16, seed=9)
        w0 = rm.scorer[1].weight.detach().clone()
        assert rm.scorer[1].weight.requires_grad
        load_state(ck, [rm])
        assert torch.equal(rm.scorer[1].weight, sd["scorer.1.weight"]) and torch.equal(rm.scorer[1].bias, sd["scorer.1.bias"])
        assert not torch.equal(rm.scorer[1].weight, w0), "the head did not train"
        assert train_reward.main(["--config", _cfg(d, tag + "r", {**body, **_dirs(d, tag + "r")}),
                                  "--resume", str(ck)]) == 0
        resumed = {r["step"]: r["train/loss"] for r in _metrics(d / "logs" / (tag + "r")) if "train/loss" in r}
        assert set(resumed) == {3} and resumed[3] == losses[3], (tag, resumed, losses)


def test_dpo_without_lora_needs_a_reference_path(tmp_path):
    from distributed_llm_alignment_amd.training import train_dpo

    body = {"model": {"policy_model_name_or_path": "tiny-llama"}, "data": {}, "optimization": {},
            **_dirs(tmp_path, "x")}
    with pytest.raises(ValueError, match="reference_model_name_or_path"):
        train_dpo.main(["--config", _cfg(tmp_path, "x", body)])


def test_trainer_refusals(tmp_path):
    from distributed_llm_alignment_amd.training import train_distill, train_rlhf, train_sft

    d = tmp_path
    lora_on = {"lora": {"enabled": True}}
    with pytest.raises(ValueError, match="RLHF"):
        train_rlhf.main(["--config", _cfg(d, "rl", {"model": {"policy_model_name_or_path": "tiny-llama", **lora_on},
                                                    "ppo": {}, **_dirs(d, "rl")})])
    gk = {"model": {"student_model_name_or_path": "tiny-llama", **lora_on},
          "distill": {"teacher_model_name_or_path": "tiny-llama", "gkd": {"enabled": True, "lmbda": 0.5}},
          **_dirs(d, "gk")}
    with pytest.raises(ValueError, match="lmbda"):
        train_distill.main(["--config", _cfg(d, "gk", gk)])
    bad = {"model": {"model_name_or_path": "tiny-llama", "lora": {"enabled": True, "rank": 8}}, **_dirs(d, "bad")}
    with pytest.raises(ValueError, match="unknown"):
        train_sft.main(["--config", _cfg(d, "bad", bad)])
