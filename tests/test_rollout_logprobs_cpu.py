"""Rollout log-probs on the CPU tier: `generate(return_logprobs=True)` aligned with the trainer's
action grid (`objectives.rollout_logp_grid`), the fallback of `ops.decode.sample_tokens_logp`, the
`old_logp=` argument of the PPO / GRPO stats functions, and `ppo.rollout_logprobs: off|monitor|old`
through the trainer CLI."""
import json
import math
from pathlib import Path

import pytest
import torch

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.models import build_model, build_value_model, generate, get_config
from distributed_llm_alignment_amd.objectives import (action_mask, grpo_rollout_stats, ppo_rollout_stats,
                                                      rollout_logp_grid)

ROOT = Path(__file__).resolve().parents[1]
CACHE_TOL = 2e-4  # KV-cache decode vs one full forward, fp32 (the bound test_models_cpu.py uses)


# ------------------------------------------------------------------------------ generate + grid
@pytest.fixture(scope="module")
def sampled():
    """A tiny fp32 model sampling 6 prompts (one left-padded) with an EOS id that occurs: some rows
    finish early."""
    cfg = get_config("tiny-llama")
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=0).eval()
    g = torch.Generator().manual_seed(3)
    S, Tp, n = 6, 7, 12
    ids = torch.randint(3, cfg.vocab_size, (S, Tp), generator=g)
    am = torch.ones_like(ids)
    ids[1, :3] = 0
    am[1, :3] = 0
    plain = generate(model, ids, am, max_new_tokens=n, do_sample=True, temperature=0.9, top_p=0.95,
                     generator=torch.Generator().manual_seed(11), return_mask=True, eos_token_id=-1)
    # an EOS id that the unconstrained draw emits early in at least one row but not in all
    first = plain[0][:, Tp:Tp + n // 2]
    vals, counts = first.reshape(-1).unique(return_counts=True)
    eos = int(vals[counts.argmax()])
    seqs, mask, logp = generate(model, ids, am, max_new_tokens=n, do_sample=True, temperature=0.9, top_p=0.95,
                                generator=torch.Generator().manual_seed(11), return_mask=True,
                                return_logprobs=True, eos_token_id=eos, pad_token_id=0)
    return model, ids, am, seqs, mask, logp, Tp, plain


def test_generate_return_order_and_default(sampled):
    model, ids, am, seqs, mask, logp, Tp, plain = sampled
    kw = dict(max_new_tokens=4, do_sample=True, generator=None, eos_token_id=-1)
    torch.manual_seed(0)
    only = generate(model, ids, am, **kw)
    assert isinstance(only, torch.Tensor)
    s2, lp2 = generate(model, ids, am, return_logprobs=True, **kw)
    assert s2.shape == (ids.shape[0], Tp + 4) and lp2.shape == (ids.shape[0], 4) and lp2.dtype == torch.float32
    assert len(plain) == 2  # seqs, mask: what the call returned before the flag existed
    assert logp.shape == (seqs.shape[0], seqs.shape[1] - Tp)


def test_rollout_logp_grid_matches_token_logprobs(sampled):
    model, ids, am, seqs, mask, logp, Tp, _ = sampled
    gm = mask[:, Tp:]
    assert 0 < int((gm == 0).sum()) and int(gm[:, -1].sum()) > 0, "want early-finished and running rows"
    assert torch.equal(logp[gm == 0], torch.zeros_like(logp[gm == 0]))  # exactly 0 past EOS
    assert (logp[gm == 1] < 0).all()
    T = seqs.shape[1]
    grid = rollout_logp_grid(logp, Tp, T)
    act = action_mask(mask, Tp)
    assert grid.shape == (seqs.shape[0], T) and grid.dtype == torch.float32
    assert torch.equal(grid[act == 0], torch.zeros_like(grid[act == 0]))  # exactly 0 outside the actions
    with torch.no_grad():
        want = model.token_logprobs(seqs, mask)
    err = ((grid - want) * act).abs().max().item()
    print(f"LOGP_STAT cpu grid-vs-token_logprobs max_err={err:.3e}")
    assert err <= CACHE_TOL
    # column j -> grid position Tp + j - 1, nothing else
    assert torch.equal(grid[:, Tp - 1:Tp - 1 + logp.shape[1]], logp)
    assert not grid[:, :Tp - 1].any() and not grid[:, Tp - 1 + logp.shape[1]:].any()


def test_rollout_logp_grid_rejects_a_grid_too_short():
    with pytest.raises(ValueError, match="rollout_logp_grid"):
        rollout_logp_grid(torch.zeros(2, 5), 4, 8)


def test_group_rollouts_return_logprobs(sampled):
    model, ids, am, *_ = sampled
    seqs, mask, logp = generate(model, ids[:2], am[:2], max_new_tokens=5, do_sample=True, return_mask=True,
                                return_logprobs=True, num_return_sequences=3, eos_token_id=-1,
                                generator=torch.Generator().manual_seed(5))
    Tp = ids.shape[1]
    assert seqs.shape == (6, Tp + 5) and logp.shape == (6, 5)
    with torch.no_grad():
        want = model.token_logprobs(seqs, mask)
    act = action_mask(mask, Tp)
    assert ((rollout_logp_grid(logp, Tp, Tp + 5) - want) * act).abs().max().item() <= CACHE_TOL


# ------------------------------------------------------------------------------------ fallback op
@pytest.mark.parametrize("greedy", [False, True])
def test_sample_tokens_logp_cpu_fallback(greedy):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(5, 37, generator=g) * 3
    rng = torch.tensor([1, 0])
    tok, lp = ops.decode.sample_tokens_logp(logits, 0.7, 5, 0.9, greedy, rng,
                                            generator=torch.Generator().manual_seed(1))
    assert tok.shape == (5,) and tok.dtype == torch.long and lp.shape == (5,) and lp.dtype == torch.float32
    want = torch.log_softmax(logits.float(), -1)[torch.arange(5), tok]
    assert torch.equal(lp, want)
    if greedy:
        assert torch.equal(tok, logits.argmax(-1))
    else:  # the tokens are the ones sample_tokens draws from the same generator state
        again = ops.decode.sample_tokens(logits, 0.7, 5, 0.9, greedy, rng, generator=torch.Generator().manual_seed(1))
        assert torch.equal(tok, again)


# ---------------------------------------------------------------------------------- stats functions
class _Counting:
    """Forwards everything to the wrapped policy and counts `token_logprobs` calls."""

    def __init__(self, model):
        self._m, self.calls = model, 0

    def token_logprobs(self, *a, **k):
        self.calls += 1
        return self._m.token_logprobs(*a, **k)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def __call__(self, *a, **k):
        return self._m(*a, **k)


@pytest.fixture(scope="module")
def rollouts():
    cfg = get_config("tiny-llama")
    policy = build_model(cfg, device="cpu", dtype=torch.float32, seed=0)
    ref = build_model(cfg, device="cpu", dtype=torch.float32, seed=1).requires_grad_(False)
    g = torch.Generator().manual_seed(7)
    S, Tp, T = 4, 5, 14
    seqs = torch.randint(3, cfg.vocab_size, (S, T), generator=g)
    mask = torch.ones(S, T, dtype=torch.long)
    mask[1, 11:] = 0
    mask[3, :2] = 0
    scores = torch.randn(S, generator=g)
    given = -torch.rand(S, T, generator=g)  # stands in for a rollout grid
    return policy, ref, seqs, mask, Tp, scores, given


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]), k


def test_grpo_rollout_stats_old_logp(rollouts):
    policy, ref, seqs, mask, Tp, scores, given = rollouts
    pol = _Counting(policy)
    for need_old in (False, True):
        pol.calls = 0
        st = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, 2, beta=0.04, need_old=need_old, old_logp=given)
        assert pol.calls == 0 and torch.equal(st["old_logp"], given)
    # without the argument: what the function returned before it existed
    pol.calls = 0
    st = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, 2, beta=0.04, need_old=True)
    assert pol.calls == 1
    with torch.no_grad():
        act = action_mask(mask, Tp)
        adv, gm = ops.group_advantages(scores, 2, True)
        want = {"act": act, "advantages": adv, "ref_logp": ref.token_logprobs(seqs, mask),
                "old_logp": policy.token_logprobs(seqs, mask), "scores": scores.float(),
                "reward_std": gm["reward_std"], "frac_zero_std": gm["frac_zero_std"]}
    _same(st, want)
    pol.calls = 0
    st = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, 2, beta=0.0)
    assert pol.calls == 0 and st["old_logp"] is None and st["ref_logp"] is None
    # everything but old_logp is the same with and without the argument
    a = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04, need_old=True)
    b = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04, old_logp=given)
    _same({k: v for k, v in a.items() if k != "old_logp"}, {k: v for k, v in b.items() if k != "old_logp"})


def test_ppo_rollout_stats_old_logp(rollouts):
    policy, ref, seqs, mask, Tp, scores, given = rollouts
    critic, _ = build_value_model("tiny-llama", device="cpu", seed=2)
    critic = critic.float()
    pol = _Counting(policy)
    st = ppo_rollout_stats(pol, ref, critic, seqs, mask, Tp, scores, old_logp=given)
    assert pol.calls == 0 and torch.equal(st["old_logp"], given)
    # the KL reward uses the given log-probs as well
    with torch.no_grad():
        act = action_mask(mask, Tp)
        kl = ((given - ref.token_logprobs(seqs, mask)) * act).sum(1) / act.sum(1).clamp(min=1)
    torch.testing.assert_close(st["kl"], kl, rtol=0, atol=0)
    # without the argument: one policy forward, and the result of passing that forward's output in
    base = ppo_rollout_stats(pol, ref, critic, seqs, mask, Tp, scores)
    assert pol.calls == 1
    with torch.no_grad():
        own = policy.token_logprobs(seqs, mask)
    assert torch.equal(base["old_logp"], own)
    _same(base, ppo_rollout_stats(pol, ref, critic, seqs, mask, Tp, scores, old_logp=own))
    assert pol.calls == 1


# --------------------------------------------------------------------------------------- trainer
@pytest.fixture(scope="module")
def prompts(tmp_path_factory):
    d = tmp_path_factory.mktemp("rlpdata")
    write_jsonl(d / "prompts.jsonl", synthetic_prompt_records(6, seed=4))
    return d / "prompts.jsonl"


def _rlhf_args(tmp, prompts, extra):
    ov = ["optimization.max_train_steps=2", f"logging.output_dir={tmp / 'ck'}", f"logging.log_dir={tmp / 'logs'}",
          "logging.save_every_steps=0", "logging.use_wandb=false", "logging.log_every_steps=1",
          "data.num_workers=0", "hardware.gradient_accumulation_steps=1",
          "model.policy_model_name_or_path=tiny-llama", "model.reference_model_name_or_path=tiny-llama",
          "model.max_seq_length=48", "reward_model.path=null", "reward_model.base_model_name_or_path=tiny-llama",
          "critic.base_model_name_or_path=tiny-llama",
          "ppo.batch_size=4", "ppo.group_size=2", "ppo.steps=2", "ppo.generation_params.max_new_tokens=4",
          "sampling.source=local", f"sampling.prompt_path={prompts}", *extra]
    args = ["--config", str(ROOT / "config" / "rlhf_config.yaml")]
    for o in ov:
        args += ["--override", o]
    return args


def _metrics(tmp):
    return [json.loads(l) for l in (tmp / "logs" / "metrics.jsonl").read_text().splitlines()]


NEW = ("train/rollout_kl", "train/rollout_logp_absdiff_max")


@pytest.mark.parametrize("algo", ["grpo", "ppo"])
@pytest.mark.parametrize("mode", ["off", "monitor", "old"])
def test_trainer_rollout_logprobs(tmp_path, prompts, algo, mode):
    from distributed_llm_alignment_amd.training import train_rlhf

    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, [f"ppo.algorithm={algo}",
                                                          f"ppo.rollout_logprobs={mode}"])) == 0
    m = _metrics(tmp_path)
    assert len(m) == 2 and all(math.isfinite(r["train/loss"]) for r in m)
    for r in m:
        if mode == "monitor":
            assert all(k in r for k in NEW), r.keys()
            print(f"LOGP_STAT cpu trainer {algo} rollout_kl={r[NEW[0]]:.3e} absdiff_max={r[NEW[1]]:.3e}")
            assert abs(r["train/rollout_kl"]) <= CACHE_TOL
            assert 0 <= r["train/rollout_logp_absdiff_max"] and math.isfinite(r["train/rollout_logp_absdiff_max"])
        else:
            assert not any(k in r for k in NEW), r.keys()


def test_trainer_default_is_off(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    assert train_rlhf.rollout_logprobs_mode({}, "grpo") == "off"
    assert train_rlhf.rollout_logprobs_mode({"rollout_logprobs": False}, "ppo") == "off"  # a bare YAML `off`
    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=grpo"])) == 0
    assert not any(k in r for r in _metrics(tmp_path) for k in NEW)


@pytest.mark.parametrize("mode", ["monitor", "old"])
def test_trainer_reinforce_rejects_rollout_logprobs(tmp_path, prompts, mode):
    from distributed_llm_alignment_amd.training import train_rlhf

    with pytest.raises(ValueError, match="rollout_logprobs"):
        train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=reinforce", f"ppo.rollout_logprobs={mode}"]))
    with pytest.raises(ValueError, match="rollout_logprobs"):
        train_rlhf.rollout_logprobs_mode({"rollout_logprobs": "sometimes"}, "ppo")


def test_reinforce_with_off_runs(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=reinforce", "ppo.rollout_logprobs=off"])) == 0
