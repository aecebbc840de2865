"""CPU tier of the temperature-aware log-probs: `ops.linear_logprob(_entropy)(temperature=)`,
`CausalLM.token_logprobs(temperature=)`, `generate(logprob_temperature=)`, the vocabulary-parallel
composition on gloo, and `ppo.logprob_temperature` through the trainer CLI. The formula of record is
log_softmax(F.linear(h, W).float() * i), i = fp32(1 / tau); fp64 references from _refs64_temp."""
import json
import math
from pathlib import Path

import pytest
import torch

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.models import build_model, generate, get_config
from distributed_llm_alignment_amd.objectives import action_mask, rollout_logp_grid

import _refs64_temp as RT
from test_distributed_cpu import run_ranks

ROOT = Path(__file__).resolve().parents[1]
CACHE_TOL = 2e-4  # tests/test_rollout_logprobs_cpu.py: KV-cache decode vs one full forward, fp32
NINF = float("-inf")


# ------------------------------------------------------------------------------------ ops
def _op_case():
    g = torch.Generator().manual_seed(5)
    N, H, V = 7, 12, 40
    h = torch.randn(N, H, generator=g)
    W = 0.5 * torch.randn(V, H, generator=g)
    tgt = torch.randint(0, V, (N,), generator=g)
    tgt[2] = -100  # one ignored row
    return h, W, tgt, torch.randn(N, generator=g), torch.randn(N, generator=g)


def _lin64(h, W, tgt, it, g=None, e=None):
    """fp64 on the fp32 logits (the CPU tier's logits are fp32: no bf16 rounding)."""
    hr = h.double().requires_grad_(True)
    Wr = W.double().requires_grad_(True)
    r = RT._rows((hr @ Wr.t()) * float(it), tgt)
    ent = torch.where(tgt >= 0, r["ent"], torch.zeros_like(r["ent"]))
    out = {"logp": r["logp"].detach(), "ent": ent.detach()}
    if g is not None:
        loss = (r["logp"] * g.double()).sum() + (0 if e is None else (ent * e.double()).sum())
        out["dh"], out["dW"] = torch.autograd.grad(loss, (hr, Wr))
    return out


@pytest.mark.parametrize("tau", RT.TEMPS)
def test_linear_logprob_temperature_matches_fp64(tau):
    h, W, tgt, g, e = _op_case()
    it = RT.inv32(tau)
    for entropy in (False, True):
        ref = _lin64(h, W, tgt, it, g, e if entropy else None)
        h1, W1 = h.clone().requires_grad_(), W.clone().requires_grad_()
        if entropy:
            lp, ent = ops.linear_logprob_entropy(h1, W1, tgt, temperature=tau)
            (lp * g + ent * e).sum().backward()
            torch.testing.assert_close(ent.detach().double(), ref["ent"], atol=1e-5, rtol=0)
            assert ent[2] == 0
        else:
            lp = ops.linear_logprob(h1, W1, tgt, temperature=tau)
            (lp * g).sum().backward()
        torch.testing.assert_close(lp.detach().double(), ref["logp"], atol=1e-5, rtol=0)
        assert lp[2] == 0
        torch.testing.assert_close(h1.grad.double(), ref["dh"], atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(W1.grad.double(), ref["dW"], atol=1e-5, rtol=1e-5)
        assert (h1.grad[2] == 0).all()  # the ignored row has no gradient


@pytest.mark.parametrize("tau", RT.TEMPS)
def test_linear_logprob_temperature_with_masked_vocabulary_entries(tau):
    """-inf logits (a -inf weight row under strictly positive hidden rows: every row of logits has
    -inf entries, one row's target sits on one) add exactly 0: values only, the gradient of a
    -inf product through the GEMM is not defined. The gradient on -inf logits is checked on the
    formula of record itself in the next test."""
    h, W, tgt, _, _ = _op_case()
    h = h.abs() + 0.1
    W[3] = NINF
    W[17] = NINF
    tgt[4] = 17
    it = RT.inv32(tau)
    z = h.double() @ W.double().t()
    assert (z[:, 3] == NINF).all() and torch.isfinite(z[:, 5]).all()
    ref = RT._rows(z * it, tgt)
    lp, ent = ops.linear_logprob_entropy(h, W, tgt, temperature=tau)
    lp2 = ops.linear_logprob(h, W, tgt, temperature=tau)
    assert torch.equal(lp, lp2)
    assert lp[4] == NINF and ref["logp"][4] == NINF
    fin = torch.isfinite(ref["logp"])
    torch.testing.assert_close(lp[fin].double(), ref["logp"][fin], atol=1e-5, rtol=0)
    want_ent = torch.where(tgt >= 0, ref["ent"], torch.zeros_like(ref["ent"]))
    assert torch.isfinite(ent).all()
    torch.testing.assert_close(ent.double(), want_ent, atol=1e-5, rtol=0)


@pytest.mark.parametrize("tau", RT.TEMPS)
def test_formula_of_record_gradient_with_masked_vocabulary_entries(tau):
    """The gradient half of the -inf case: -inf logits fed directly to the CPU formula of record
    (`_ref_logits_logprob_entropy`, what the wrappers apply to F.linear's output), differentiated
    with respect to the logits and compared with the fp64 dz formula. A -inf logit receives
    exactly 0; one row is ignored; the targets sit on finite logits (on a -inf logit logp is -inf
    and no gradient is defined)."""
    from distributed_llm_alignment_amd.ops.logprob import _ref_logits_logprob_entropy

    gen = torch.Generator().manual_seed(9)
    N, V = 6, 40
    z = 3.0 * torch.randn(N, V, generator=gen)
    dead = torch.zeros(N, V, dtype=torch.bool)
    dead[:, 3] = True
    dead[1, 10:30] = True
    dead[4, 1:] = True  # one finite logit: p = 1, H = 0
    z[dead] = NINF
    tgt = torch.tensor([5, 7, -100, 0, 0, 39])
    g, e = torch.randn(N, generator=gen), torch.randn(N, generator=gen)
    it = RT.inv32(tau)
    for ee in (None, e):
        z1 = z.clone().requires_grad_()
        lp, ent = _ref_logits_logprob_entropy(z1, tgt, tau)
        ((lp * g).sum() + (0 if ee is None else (ent * ee).sum())).backward()
        want = RT.bwd64(z, tgt, g, ee, it)
        ref = RT.rows64(z, tgt, it)
        torch.testing.assert_close(lp.detach().double(), ref["logp"], atol=1e-5, rtol=0)
        assert torch.isfinite(z1.grad).all()
        assert (z1.grad[dead] == 0).all() and (z1.grad[2] == 0).all()
        torch.testing.assert_close(z1.grad.double(), want, atol=1e-5, rtol=1e-5)


def test_unit_temperature_is_the_call_without_the_keyword():
    h, W, tgt, g, e = _op_case()
    outs = []
    for kw in ({}, {"temperature": 1.0}):
        h1, W1 = h.clone().requires_grad_(), W.clone().requires_grad_()
        lp = ops.linear_logprob(h1, W1, tgt, **kw)
        lp2, ent = ops.linear_logprob_entropy(h1, W1, tgt, **kw)
        (lp * g + lp2 * g + ent * e).sum().backward()
        outs.append((lp.detach(), lp2.detach(), ent.detach(), h1.grad, W1.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("bad", [0.0, -0.5, float("inf"), float("nan")])
def test_temperature_must_be_finite_and_positive(bad):
    h, W, tgt, _, _ = _op_case()
    with pytest.raises(ValueError, match="temperature"):
        ops.linear_logprob(h, W, tgt, temperature=bad)


# ---------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def tiny():
    cfg = get_config("tiny-llama")
    return cfg, build_model(cfg, device="cpu", dtype=torch.float32, seed=0).eval()


@pytest.mark.parametrize("tau", RT.TEMPS)
def test_token_logprobs_temperature_is_the_formula_on_model_logits(tiny, tau):
    cfg, model = tiny
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (3, 9), generator=g)
    am = torch.ones_like(ids)
    am[1, :2] = 0
    with torch.no_grad():
        lp, ent = model.token_logprobs(ids, am, with_entropy=True, temperature=tau)
        lp_only = model.token_logprobs(ids, am, temperature=tau)
        logits = model.logits(model(ids, am))
    assert torch.equal(lp, lp_only)
    tgt, _ = ops.shifted_targets(ids, am)
    r = RT._rows(logits.double().reshape(-1, cfg.vocab_size) * RT.inv32(tau), tgt.reshape(-1))
    want_ent = torch.where(tgt.reshape(-1) >= 0, r["ent"], torch.zeros_like(r["ent"]))
    torch.testing.assert_close(lp.double().reshape(-1), r["logp"], atol=2e-5, rtol=0)
    torch.testing.assert_close(ent.double().reshape(-1), want_ent, atol=2e-5, rtol=0)
    with torch.no_grad():
        assert torch.equal(model.token_logprobs(ids, am, temperature=1.0), model.token_logprobs(ids, am))


def test_lm_head_bias_branch_scales_its_logits():
    cfg = get_config("tiny-llama")
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=0).eval()
    model.lm_head_bias = torch.nn.Parameter(0.3 * torch.randn(cfg.vocab_size, generator=torch.Generator().manual_seed(1)))
    ids = torch.randint(3, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        lp, ent = model.token_logprobs(ids, with_entropy=True, temperature=0.7)
        logits = model.logits(model(ids))
    tgt, _ = ops.shifted_targets(ids, None)
    r = RT._rows(logits.double().reshape(-1, cfg.vocab_size) * RT.inv32(0.7), tgt.reshape(-1))
    torch.testing.assert_close(lp.double().reshape(-1), r["logp"], atol=2e-5, rtol=0)
    torch.testing.assert_close(ent.double().reshape(-1), torch.where(tgt.reshape(-1) >= 0, r["ent"], 0.0 * r["ent"]),
                               atol=2e-5, rtol=0)


# ------------------------------------------------------------------------------- generate
@pytest.mark.parametrize("G", [1, 3])
def test_generate_logprob_temperature(tiny, G):
    cfg, model = tiny
    g = torch.Generator().manual_seed(3)
    S, Tp, n, tau = 4, 7, 8, 0.7
    ids = torch.randint(3, cfg.vocab_size, (S, Tp), generator=g)
    am = torch.ones_like(ids)
    ids[1, :3] = 0
    am[1, :3] = 0
    kw = dict(max_new_tokens=n, do_sample=True, temperature=tau, top_p=0.95, return_mask=True, eos_token_id=-1,
              num_return_sequences=G)
    seqs0, mask0 = generate(model, ids, am, generator=torch.Generator().manual_seed(11), **kw)
    seqs, mask, logp = generate(model, ids, am, generator=torch.Generator().manual_seed(11), return_logprobs=True,
                                logprob_temperature=tau, **kw)
    assert torch.equal(seqs, seqs0) and torch.equal(mask, mask0)
    _, _, logp1 = generate(model, ids, am, generator=torch.Generator().manual_seed(11), return_logprobs=True, **kw)
    assert not torch.equal(logp, logp1)
    T = seqs.shape[1]
    act = action_mask(mask, Tp)
    with torch.no_grad():
        want = model.token_logprobs(seqs, mask, temperature=tau)
        want1 = model.token_logprobs(seqs, mask)
    err = ((rollout_logp_grid(logp, Tp, T) - want) * act).abs().max().item()
    err1 = ((rollout_logp_grid(logp1, Tp, T) - want1) * act).abs().max().item()
    print(f"LOGP_STAT cpu tempered grid-vs-token_logprobs max_err={err:.3e} (temperature 1: {err1:.3e})")
    assert err <= CACHE_TOL and err1 <= CACHE_TOL
    # None and 1.0 are today's behaviour
    _, _, logp2 = generate(model, ids, am, generator=torch.Generator().manual_seed(11), return_logprobs=True,
                           logprob_temperature=1.0, **kw)
    assert torch.equal(logp1, logp2)


def test_generate_rejects_a_logprob_temperature_the_sampler_does_not_have(tiny):
    cfg, model = tiny
    ids = torch.randint(3, cfg.vocab_size, (2, 5), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="logprob_temperature"):
        generate(model, ids, max_new_tokens=3, do_sample=True, temperature=0.7, return_logprobs=True,
                 logprob_temperature=0.9)
    with pytest.raises(ValueError, match="logprob_temperature"):  # greedy has no draw temperature
        generate(model, ids, max_new_tokens=3, do_sample=False, temperature=0.7, return_logprobs=True,
                 logprob_temperature=0.7)


def test_sample_tokens_logp_tempered_cpu_fallback():
    logits = torch.randn(5, 37, generator=torch.Generator().manual_seed(0)) * 3
    rng = torch.tensor([1, 0])
    tok, lp = ops.decode.sample_tokens_logp_tempered(logits, 0.7, 5, 0.9, False, rng,
                                                     generator=torch.Generator().manual_seed(1))
    again = ops.decode.sample_tokens(logits, 0.7, 5, 0.9, False, rng, generator=torch.Generator().manual_seed(1))
    assert torch.equal(tok, again)
    want = torch.log_softmax(logits.double() * RT.inv32(0.7), -1)[torch.arange(5), tok]
    torch.testing.assert_close(lp.double(), want, atol=1e-5, rtol=0)
    a = ops.decode.sample_tokens_logp_tempered(logits, 0.7, 5, 0.9, True, rng)
    b = ops.decode.sample_tokens_logp(logits, 0.7, 5, 0.9, True, rng)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------------------------------------- vocabulary parallel
VP_N, VP_V, VP_H, VP_TAU = 10, 64, 12, 0.7


def _vp_inputs():
    g = torch.Generator().manual_seed(21)
    hidden = torch.randn(VP_N, VP_H, generator=g)
    weight = 0.25 * torch.randn(VP_V, VP_H, generator=g)
    targets = torch.tensor([1, 17, 33, 49, 62, 15, -100, 40, 31, 5])
    a, b = torch.randn(VP_N, generator=g), torch.randn(VP_N, generator=g)
    return hidden, weight, targets, a, b


def _vp_rank(rank, world):
    import torch

    from distributed_llm_alignment_amd.parallel.tensor_parallel import (vocab_parallel_logprob,
                                                                        vocab_parallel_logprob_entropy)

    hidden, weight, targets, a, b = _vp_inputs()
    Vl = VP_V // world
    out = {}
    h = hidden.clone().requires_grad_(True)
    w = weight[rank * Vl:(rank + 1) * Vl].clone().requires_grad_(True)
    lp, ent = vocab_parallel_logprob_entropy(h, w, targets, rank * Vl, None, temperature=VP_TAU)
    (a * lp + b * ent).sum().backward()
    out.update(lp=lp, ent=ent, dh=h.grad, dw=w.grad)
    h = hidden.clone().requires_grad_(True)
    w = weight[rank * Vl:(rank + 1) * Vl].clone().requires_grad_(True)
    lp = vocab_parallel_logprob(h, w, targets, rank * Vl, None, temperature=VP_TAU)
    (a * lp).sum().backward()
    out.update(lp_plain=lp, dh_plain=h.grad, dw_plain=w.grad)
    return out


def test_vocab_parallel_temperature_matches_dense():
    hidden, weight, targets, a, b = _vp_inputs()
    h, w = hidden.clone().requires_grad_(True), weight.clone().requires_grad_(True)
    lp, ent = ops.linear_logprob_entropy(h, w, targets, temperature=VP_TAU)
    (a * lp + b * ent).sum().backward()
    h2, w2 = hidden.clone().requires_grad_(True), weight.clone().requires_grad_(True)
    lp2 = ops.linear_logprob(h2, w2, targets, temperature=VP_TAU)
    (a * lp2).sum().backward()
    with torch.no_grad():
        assert not torch.allclose(lp, ops.linear_logprob(hidden, weight, targets), atol=1e-3)
    out = run_ranks(_vp_rank, world=2)
    Vl = VP_V // 2
    for r in range(2):
        o = out[r]
        torch.testing.assert_close(o["lp"], lp.detach(), atol=1e-5, rtol=0)
        torch.testing.assert_close(o["ent"], ent.detach(), atol=1e-5, rtol=0)
        torch.testing.assert_close(o["dh"], h.grad, atol=1e-5, rtol=0)
        torch.testing.assert_close(o["dw"], w.grad[r * Vl:(r + 1) * Vl], atol=1e-5, rtol=0)
        torch.testing.assert_close(o["lp_plain"], lp2.detach(), atol=1e-5, rtol=0)
        torch.testing.assert_close(o["dh_plain"], h2.grad, atol=1e-5, rtol=0)
        torch.testing.assert_close(o["dw_plain"], w2.grad[r * Vl:(r + 1) * Vl], atol=1e-5, rtol=0)
        assert o["lp"][6] == 0 and o["ent"][6] == 0


# -------------------------------------------------------------------------------- trainer
@pytest.fixture(scope="module")
def prompts(tmp_path_factory):
    d = tmp_path_factory.mktemp("lptdata")
    write_jsonl(d / "prompts.jsonl", synthetic_prompt_records(6, seed=4))
    return d / "prompts.jsonl"


def _rlhf_args(tmp, prompts, extra, steps=1):
    ov = [f"optimization.max_train_steps={steps}", f"logging.output_dir={tmp / 'ck'}", f"logging.log_dir={tmp / 'logs'}",
          "logging.save_every_steps=0", "logging.use_wandb=false", "logging.log_every_steps=1",
          "data.num_workers=0", "hardware.gradient_accumulation_steps=1",
          "model.policy_model_name_or_path=tiny-llama", "model.reference_model_name_or_path=tiny-llama",
          "model.max_seq_length=48", "reward_model.path=null", "reward_model.base_model_name_or_path=tiny-llama",
          "critic.base_model_name_or_path=tiny-llama",
          "ppo.batch_size=4", "ppo.group_size=2", f"ppo.steps={steps}", "ppo.generation_params.max_new_tokens=4",
          "sampling.source=local", f"sampling.prompt_path={prompts}", *extra]
    args = ["--config", str(ROOT / "config" / "rlhf_config.yaml")]
    for o in ov:
        args += ["--override", o]
    return args


def _metrics(tmp):
    return [json.loads(l) for l in (tmp / "logs" / "metrics.jsonl").read_text().splitlines()]


KEY = "train/logprob_temperature"


@pytest.mark.parametrize("algo", ["grpo", "ppo"])
def test_trainer_rollout_temperature_with_correct(tmp_path, prompts, algo):
    """One step at `logprob_temperature: rollout` with `rollout_logprobs: correct`: the engine's and
    the trainer's log-probs are of the same tempered distribution, so the importance weights sit
    at 1 to the KV-cache tolerance (at temperature 1 against a 0.7 draw they would too, but of the
    wrong distribution; `rollout_kl` is the witness that the two sides agree)."""
    from distributed_llm_alignment_amd.training import train_rlhf

    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, [
        f"ppo.algorithm={algo}", "ppo.logprob_temperature=rollout", "ppo.rollout_logprobs=correct",
        "ppo.log_entropy=true"], steps=2)) == 0
    m = _metrics(tmp_path)
    assert len(m) == 2 and all(math.isfinite(r["train/loss"]) for r in m)
    assert m[0][KEY] == 0.7  # generation_params.temperature of config/rlhf_config.yaml
    assert KEY not in m[1]  # logged once
    for r in m:
        print(f"LOGP_STAT cpu trainer {algo} tempered is_mean={r['train/rollout_is_mean']:.6f} "
              f"rollout_kl={r['train/rollout_kl']:.3e}")
        assert abs(r["train/rollout_is_mean"] - 1.0) <= CACHE_TOL
        assert abs(r["train/rollout_kl"]) <= CACHE_TOL
        assert math.isfinite(r["train/entropy"])


def test_trainer_key_absent_equals_unit_temperature(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    a, b = tmp_path / "a", tmp_path / "b"
    assert train_rlhf.main(_rlhf_args(a, prompts, ["ppo.algorithm=grpo"])) == 0
    assert train_rlhf.main(_rlhf_args(b, prompts, ["ppo.algorithm=grpo", "ppo.logprob_temperature=1.0"])) == 0
    ma, mb = _metrics(a), _metrics(b)
    assert KEY not in ma[0] and mb[0][KEY] == 1.0
    assert ma[0]["train/loss"] == mb[0]["train/loss"]
    assert set(mb[0]) - set(ma[0]) == {KEY}


def test_trainer_temperature_changes_the_step(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    a, b = tmp_path / "a", tmp_path / "b"
    ex = ["ppo.algorithm=grpo", "ppo.log_entropy=true"]
    assert train_rlhf.main(_rlhf_args(a, prompts, ex)) == 0
    assert train_rlhf.main(_rlhf_args(b, prompts, ex + ["ppo.logprob_temperature=0.5"])) == 0
    # a sharper distribution: the same rollouts (same seed), a lower entropy
    assert _metrics(b)[0]["train/entropy"] < _metrics(a)[0]["train/entropy"]
    assert _metrics(b)[0][KEY] == 0.5


@pytest.mark.parametrize("extra", [
    ["ppo.algorithm=reinforce", "ppo.logprob_temperature=0.7"],
    ["ppo.algorithm=reinforce", "ppo.logprob_temperature=rollout"],
    ["ppo.algorithm=grpo", "ppo.logprob_temperature=warm"],
    ["ppo.algorithm=grpo", "ppo.logprob_temperature=0"],
    ["ppo.algorithm=ppo", "ppo.logprob_temperature=-1.0"],
    ["ppo.algorithm=grpo", "ppo.logprob_temperature=.inf"],
    ["ppo.algorithm=grpo", "ppo.logprob_temperature=.nan"],
    ["ppo.algorithm=grpo", "ppo.logprob_temperature=0.9", "ppo.rollout_logprobs=monitor"],
    ["ppo.algorithm=ppo", "ppo.logprob_temperature=0.9", "ppo.rollout_logprobs=correct"],
])
def test_trainer_start_up_errors(tmp_path, prompts, extra):
    from distributed_llm_alignment_amd.training import train_rlhf

    with pytest.raises(ValueError, match="logprob_temperature"):
        train_rlhf.main(_rlhf_args(tmp_path, prompts, extra))


def test_logprob_temperature_resolution():
    from distributed_llm_alignment_amd.training.train_rlhf import logprob_temperature

    gen = {"temperature": 0.7, "do_sample": True}
    assert logprob_temperature({}, "grpo") == 1.0
    assert logprob_temperature({"logprob_temperature": "rollout", "generation_params": gen}, "ppo") == 0.7
    assert logprob_temperature({"logprob_temperature": "rollout",
                                "generation_params": {"temperature": 0.7, "do_sample": False}}, "grpo") == 1.0
    assert logprob_temperature({"logprob_temperature": 1.0}, "reinforce") == 1.0
    assert logprob_temperature({"logprob_temperature": 0.7, "rollout_logprobs": "old", "generation_params": gen},
                               "grpo") == 0.7
    assert logprob_temperature({"logprob_temperature": 1.0, "rollout_logprobs": "old", "generation_params": gen},
                               "grpo") == 1.0
    for bad in (True, None, "hot", [0.7]):
        with pytest.raises(ValueError, match="logprob_temperature"):
            logprob_temperature({"logprob_temperature": bad}, "grpo")


@pytest.mark.parametrize("algo", ["grpo", "ppo"])
def test_default_run_never_enters_the_tempered_path(tmp_path, prompts, algo, monkeypatch):
    """With the key absent (and at 1.0) every wrapper takes the temperature == 1.0 branch, which
    calls the ops it called before: `inv_temperature` (the only way to a `*_temp` op or a scaled
    logit) and the tempered sampler wrapper are never reached."""
    from distributed_llm_alignment_amd.ops import decode as dec
    from distributed_llm_alignment_amd.ops import logprob as lpmod
    from distributed_llm_alignment_amd.training import train_rlhf

    def boom(*a, **k):
        raise AssertionError("tempered path entered in a default run")

    monkeypatch.setattr(lpmod, "inv_temperature", boom)
    monkeypatch.setattr(dec, "sample_tokens_logp_tempered", boom)
    for i, extra in enumerate(([], ["ppo.logprob_temperature=1.0"])):
        assert train_rlhf.main(_rlhf_args(tmp_path / str(i), prompts, [
            f"ppo.algorithm={algo}", "ppo.rollout_logprobs=monitor", "ppo.log_entropy=true", *extra])) == 0
