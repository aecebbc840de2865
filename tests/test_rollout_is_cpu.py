"""Truncated importance weights on the CPU tier: the `ops` CPU branch of `rollout_is_weights` and of
the weighted `grpo_loss` / `ppo_policy_loss` against the fp64 references of tests/_refs64_is.py
(the agreement check of test_refs64_cpu.py), the properties of the weight argument, the argument
checks, and `ppo.rollout_logprobs: correct` through the trainer CLI."""
import json
import math
from pathlib import Path

import pytest
import torch

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.ops.losses import (GRPO_LOSS_TYPES, _ref_grpo_loss,
                                                      _ref_rollout_is_weights)

import _branch32 as B32
import _branch32_is as BI
import _refs64 as R
import _refs64_is as RI
from test_refs64_cpu import agree

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("mode", RI.IS_MODES)
@pytest.mark.parametrize("level", RI.IS_LEVELS)
@pytest.mark.parametrize("S,T", RI.IS_SHAPES)
def test_is_weights(S, T, level, mode):
    c = RI.is_case(S, T, level)
    cpu, ref = BI.is_weights(**c, level=level, mode=mode), RI.is_weights64(**c, level=level, mode=mode)
    agree("rollout_is_weights", cpu, ref)
    # decisions are the same in fp32 and fp64: both fractions and the count are exact
    assert torch.equal(cpu["metrics"][[1, 2, 4]].double(), ref["metrics"][[1, 2, 4]].float().double())
    assert not cpu["w"].requires_grad
    assert (cpu["w"][c["m"] == 0] == 0).all()
    if mode == "truncate":
        assert cpu["metrics"][2].item() == 0
    if S >= 5:  # the row above C, the row below F
        on0, on1 = c["m"][0] != 0, c["m"][1] != 0
        assert (cpu["w"][0][on0] == (RI.IS_CAP if mode == "truncate" else 0.0)).all()
        assert ((cpu["w"][1][on1] == 0) if mode == "mask" else (cpu["w"][1][on1] < RI.IS_FLOOR)).all()


@pytest.mark.parametrize("mode", RI.IS_MODES)
@pytest.mark.parametrize("level", RI.IS_LEVELS)
def test_is_weights_saturated(level, mode):
    c = RI.is_sat_case()
    cpu, ref = BI.is_weights(**c, level=level, mode=mode), RI.is_weights64(**c, level=level, mode=mode)
    agree("rollout_is_weights_sat", cpu, ref, inscale=100.0)
    RI.check_saturated(cpu, level, mode)


def test_is_weights_empty_mask():
    c = RI.is_case(5, 256, "token")
    c["m"] = torch.zeros_like(c["m"])
    for level in RI.IS_LEVELS:
        for mode in RI.IS_MODES:
            got = BI.is_weights(**c, level=level, mode=mode)
            assert (got["w"] == 0).all() and (got["metrics"] == 0).all()


@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
@pytest.mark.parametrize("S,T", R.GRPO_SHAPES)
def test_grpo_weighted(S, T, mode, beta):
    c = R.grpo_case(S, T)
    c["w"] = RI.weight_case((S, T))
    kw = dict(beta=beta, mode=mode, max_len=T)
    agree("grpo_loss_w", BI.grpo_w(**c, **kw), RI.grpo_w64(**c, **kw))


def test_grpo_weighted_denom():
    c = R.grpo_case(257, 5)
    c["w"] = RI.weight_case((257, 5))
    kw = dict(beta=0.04, mode="token", max_len=5, denom=R.GRPO_DENOM)
    agree("grpo_loss_w_denom", BI.grpo_w(**c, **kw), RI.grpo_w64(**c, **kw))


@pytest.mark.parametrize("n,masked", [(n, False) for n in R.PPO_N] + [(1025, True)])
def test_ppo_weighted(n, masked):
    c = R.ppo_policy_case(n, masked)
    c["w"] = RI.weight_case((n,))
    agree("ppo_policy_loss_w", BI.ppo_policy_w(**c), RI.ppo_policy_w64(**c))


# ------------------------------------------------------------------------- properties
def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_grpo_none_and_ones_are_the_unweighted_loss(mode):
    c = R.grpo_case(257, 5)
    kw = dict(beta=0.04, mode=mode, max_len=5)
    base = B32.grpo(**c, **kw)
    _same(base, BI.grpo_w(**c, w=None, **kw))
    _same(base, BI.grpo_w(**c, w=torch.ones_like(c["lp"]), **kw))


def test_ppo_none_and_ones_are_the_unweighted_loss():
    c = R.ppo_policy_case(1025)
    base = B32.ppo_policy(**c)
    _same(base, BI.ppo_policy_w(**c, w=None))
    _same(base, BI.ppo_policy_w(**c, w=torch.ones_like(c["lp"])))


@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_grpo_constant_weight_scales_the_advantages(mode):
    """beta = 0: the loss is linear in A, so a constant w equals advantages scaled by w."""
    c = R.grpo_case(300, 257)
    kw = dict(beta=0.0, mode=mode, max_len=257)
    a = BI.grpo_w(**c, w=torch.full_like(c["lp"], 0.75), **kw)
    b = B32.grpo(**{**c, "adv": 0.75 * c["adv"]}, **kw)
    for k in ("loss", "dlp"):
        torch.testing.assert_close(a[k], b[k], rtol=1e-5, atol=1e-7)
    assert torch.equal(a["metrics"], b["metrics"])


def test_ppo_constant_weight_scales_the_advantages():
    c = R.ppo_policy_case(1025)
    a = BI.ppo_policy_w(**c, w=torch.full_like(c["lp"], 0.75))
    b = B32.ppo_policy(**{**c, "adv": 0.75 * c["adv"]})
    for k in ("loss", "dlp"):
        torch.testing.assert_close(a[k], b[k], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("loss_type", GRPO_LOSS_TYPES)
def test_grpo_micro_batches_with_sliced_weights_sum_to_the_full_gradient(loss_type):
    from distributed_llm_alignment_amd.objectives import grpo_denominator

    S, T = 12, 37
    c = R.grpo_case(S, T)
    w = RI.weight_case((S, T))
    args = dict(clip_low=0.2, clip_high=0.28, beta=0.04, loss_type=loss_type, max_len=T)
    x = c["lp"].clone().requires_grad_(True)
    full, _ = ops.grpo_loss(x, c["old"], c["ref"], c["adv"], c["m"], is_weight=w, **args)
    (gfull,) = torch.autograd.grad(full, x)
    denom = grpo_denominator(c["m"], loss_type, T)
    tot, parts = 0.0, []
    for a, b in ((0, 5), (5, 8), (8, 12)):
        y = c["lp"][a:b].clone().requires_grad_(True)
        loss, _ = ops.grpo_loss(y, c["old"][a:b], c["ref"][a:b], c["adv"][a:b], c["m"][a:b], denom=denom,
                                is_weight=w[a:b], **args)
        parts.append(torch.autograd.grad(loss, y)[0])
        tot = tot + loss.detach()
    torch.testing.assert_close(torch.cat(parts), gfull, rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(tot, full.detach(), rtol=1e-5, atol=1e-7)


def test_a_masked_out_token_still_counts_in_the_divisor():
    c = R.ppo_policy_case(257)
    w = torch.ones_like(c["lp"])
    w[::2] = 0.0
    got = BI.ppo_policy_w(**c, w=w)
    want = BI.ppo_policy_w(**{**c, "m": c["m"] * w}, w=torch.ones_like(w))
    n, nw = c["m"].sum(), (c["m"] * w).sum()
    torch.testing.assert_close(got["loss"] * n, want["loss"] * nw, rtol=1e-5, atol=1e-7)
    assert got["count"].item() == n.item()


# --------------------------------------------------------------------- argument checks
def test_argument_checks():
    c = RI.is_case(3, 255, "token")
    t, r, m = c["trainer_lp"], c["rollout_lp"], c["m"]
    for kw in (dict(cap=0.0), dict(cap=-1.0), dict(cap=float("inf")), dict(cap=float("nan")),
               dict(floor=-0.1), dict(floor=2.5), dict(level="batch"), dict(mode="clip")):
        with pytest.raises(ValueError, match="rollout_is_weights"):
            ops.rollout_is_weights(t, r, m, **kw)
    with pytest.raises(ValueError, match="rollout_is_weights"):
        ops.rollout_is_weights(t, r[:, :-1], m)
    with pytest.raises(ValueError, match="rollout_is_weights"):
        ops.rollout_is_weights(t[0], r[0], m[0])
    # floor=None is 1 / cap
    a = ops.rollout_is_weights(t, r, m, cap=4.0, mode="mask")
    b = ops.rollout_is_weights(t, r, m, cap=4.0, floor=0.25, mode="mask")
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert set(a[1]) == {"is_mean", "is_frac_high", "is_frac_low", "is_ess", "tokens"}
    w2, met = _ref_rollout_is_weights(t, r, m, 4.0, None, "token", "mask")
    assert torch.equal(a[0], w2) and met.shape == (5,)
    g = R.grpo_case(3, 7)
    with pytest.raises(ValueError, match="is_weight"):
        ops.grpo_loss(g["lp"], g["old"], g["ref"], g["adv"], g["m"], is_weight=torch.ones(3, 6))
    p = R.ppo_policy_case(9)
    with pytest.raises(ValueError, match="is_weight"):
        ops.ppo_policy_loss(p["lp"], p["old"], p["adv"], p["m"], is_weight=torch.ones(8))
    # the weight is detached: no gradient reaches it
    w = torch.ones(3, 7, requires_grad=True)
    x = g["lp"].clone().requires_grad_(True)
    loss, _ = ops.grpo_loss(x, g["old"], g["ref"], g["adv"], g["m"], is_weight=w)
    loss.backward()
    assert w.grad is None and x.grad is not None
    loss2, _ = _ref_grpo_loss(g["lp"], g["old"], g["ref"], g["adv"], g["m"], is_weight=w.detach())
    assert torch.equal(loss.detach(), loss2)


def test_rollout_logprobs_mode_and_settings():
    from distributed_llm_alignment_amd.training import train_rlhf as tr

    assert "correct" in tr.ROLLOUT_LOGPROBS
    assert tr.rollout_logprobs_mode({"rollout_logprobs": "correct"}, "ppo") == "correct"
    assert tr.rollout_logprobs_mode({"rollout_logprobs": "Correct"}, "grpo") == "correct"
    with pytest.raises(ValueError, match="rollout_logprobs"):
        tr.rollout_logprobs_mode({"rollout_logprobs": "correct"}, "reinforce")
    assert tr.rollout_is_settings({}) == {"is_cap": 2.0, "is_floor": None, "is_level": "token", "is_mode": "truncate"}
    assert tr.rollout_is_settings({"rollout_is_cap": 3, "rollout_is_floor": 0.1, "rollout_is_level": "sequence",
                                   "rollout_is_mode": "mask"}) == {"is_cap": 3.0, "is_floor": 0.1,
                                                                   "is_level": "sequence", "is_mode": "mask"}
    for bad in ({"rollout_is_cap": 0}, {"rollout_is_cap": -2}, {"rollout_is_cap": "big"},
                {"rollout_is_cap": float("inf")}, {"rollout_is_floor": -1}, {"rollout_is_floor": 3.0},
                {"rollout_is_level": "batch"}, {"rollout_is_mode": "clip"}):
        with pytest.raises(ValueError, match="rollout_is_"):
            tr.rollout_is_settings(bad)


# ----------------------------------------------------------------------- stats functions
def test_rollout_stats_return_weights():
    from distributed_llm_alignment_amd.models import build_model, build_value_model, get_config
    from distributed_llm_alignment_amd.objectives import (action_mask, grpo_rollout_stats, ppo_rollout_stats)

    cfg = get_config("tiny-llama")
    policy = build_model(cfg, device="cpu", dtype=torch.float32, seed=0)
    ref = build_model(cfg, device="cpu", dtype=torch.float32, seed=1).requires_grad_(False)
    critic, _ = build_value_model("tiny-llama", device="cpu", seed=2)
    critic = critic.float()
    g = torch.Generator().manual_seed(7)
    S, Tp, T = 4, 5, 14
    seqs = torch.randint(3, cfg.vocab_size, (S, T), generator=g)
    mask = torch.ones(S, T, dtype=torch.long)
    mask[1, 11:] = 0
    scores = torch.randn(S, generator=g)
    act = action_mask(mask, Tp)
    with torch.no_grad():
        own = policy.token_logprobs(seqs, mask)
    given = (own + 0.5 * torch.randn(S, T, generator=g)) * act  # a rollout grid: zeros off the actions
    kw = dict(is_cap=1.5, is_floor=0.8, is_level="sequence", is_mode="mask")
    want_w, want_m = ops.rollout_is_weights(own, given, act, 1.5, 0.8, "sequence", "mask")
    base = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04, need_old=True)
    st = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04, rollout_logp=given, **kw)
    assert set(st) == set(base) | {"is_weight", "rollout_is"}
    assert torch.equal(st["old_logp"], own)  # the trainer's own, computed without need_old
    assert torch.equal(st["is_weight"], want_w)
    assert set(st["rollout_is"]) == {"rollout_is_mean", "rollout_is_frac_high", "rollout_is_frac_low", "rollout_is_ess"}
    assert torch.equal(st["rollout_is"]["rollout_is_ess"], want_m["is_ess"])
    pb = ppo_rollout_stats(policy, ref, critic, seqs, mask, Tp, scores)
    ps = ppo_rollout_stats(policy, ref, critic, seqs, mask, Tp, scores, rollout_logp=given, **kw)
    assert set(ps) == set(pb) | {"is_weight", "rollout_is"}
    for k in pb:  # old-policy log-probs, KL reward, advantages: the trainer's own, unchanged
        assert torch.equal(ps[k], pb[k]), k
    assert torch.equal(ps["is_weight"], want_w)


# -------------------------------------------------------------------------------- trainer
@pytest.fixture(scope="module")
def prompts(tmp_path_factory):
    d = tmp_path_factory.mktemp("risdata")
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


NEW = ("train/rollout_is_mean", "train/rollout_is_frac_high", "train/rollout_is_frac_low", "train/rollout_is_ess")
MONITOR = ("train/rollout_kl", "train/rollout_logp_absdiff_max")


@pytest.mark.parametrize("level,mode", [("token", "truncate"), ("sequence", "mask")])
@pytest.mark.parametrize("algo", ["grpo", "ppo"])
def test_trainer_correct(tmp_path, prompts, algo, level, mode):
    from distributed_llm_alignment_amd.training import train_rlhf

    cap = 2.0
    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, [
        f"ppo.algorithm={algo}", "ppo.rollout_logprobs=correct", f"ppo.rollout_is_cap={cap}",
        f"ppo.rollout_is_level={level}", f"ppo.rollout_is_mode={mode}", "ppo.update_micro_batch=2"])) == 0
    m = _metrics(tmp_path)
    assert len(m) == 2 and all(math.isfinite(r["train/loss"]) for r in m)
    for r in m:
        assert all(k in r for k in NEW + MONITOR), r.keys()
        assert all(math.isfinite(r[k]) for k in NEW + MONITOR)
        print(f"IS_STAT cpu trainer {algo} {level}/{mode} " + " ".join(f"{k[6:]}={r[k]:.4e}" for k in NEW))
        assert 0 < r["train/rollout_is_mean"] <= cap
        assert 0 < r["train/rollout_is_ess"] <= 1
        assert 0 <= r["train/rollout_is_frac_high"] <= 1 and 0 <= r["train/rollout_is_frac_low"] <= 1


def test_trainer_off_has_no_new_metrics(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=grpo", "ppo.rollout_logprobs=off"])) == 0
    assert not any(k in r for r in _metrics(tmp_path) for k in NEW + MONITOR)


def test_trainer_rejects_bad_settings(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    with pytest.raises(ValueError, match="rollout_logprobs"):
        train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=reinforce", "ppo.rollout_logprobs=correct"]))
    with pytest.raises(ValueError, match="rollout_is_mode"):
        train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=grpo", "ppo.rollout_logprobs=correct",
                                                       "ppo.rollout_is_mode=clip"]))
