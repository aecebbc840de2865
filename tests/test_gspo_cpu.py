"""GSPO on the CPU tier: `_ref_grpo_loss(importance_level="sequence")`, the formula of record,
against the fp64 closed forms of tests/_refs64_gspo.py (the agreement check of test_refs64_cpu.py),
the properties that tie the sequence level to the token level, the edge cases of the definition,
the argument and start-up checks, the shipped config and a micro-batched GRPO update."""
import math
from pathlib import Path

import pytest
import torch

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.ops.losses import GRPO_IMPORTANCE_LEVELS, _ref_grpo_loss
from distributed_llm_alignment_amd.utils.config import load_config

import _branch32_gspo as BG
import _refs64 as R
import _refs64_gspo as RG
import _refs64_is as RI
from test_refs64_cpu import agree

ROOT = Path(__file__).resolve().parents[1]


def test_levels_are_exported():
    assert GRPO_IMPORTANCE_LEVELS == ("token", "sequence")


# ------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
@pytest.mark.parametrize("S,T", RG.GSPO_SHAPES)
def test_sequence_level_against_fp64(S, T, mode, beta, weighted):
    c = RG.gspo_case(S, T)
    kw = dict(beta=beta, mode=mode, max_len=T, w=RI.weight_case((S, T)) if weighted else None)
    cpu, ref = BG.gspo(**c, **kw), RG.gspo64(**c, **kw)
    agree("grpo_loss_seq", cpu, ref)
    for k in ref:
        assert math.isfinite(R.e32_of(cpu[k], ref[k]))
    # decisions are the same in fp32 and fp64: the clipped-token count and the token count are exact
    n = c["m"].sum().item()
    assert cpu["metrics"][3].item() == n
    assert round(cpu["metrics"][0].item() * n) == RG.clipped_tokens64(c["lp"], c["old"], c["m"])
    assert (cpu["dlp"][c["m"] == 0] == 0).all()


@pytest.mark.parametrize("weighted", [False, True])
def test_sequence_level_against_fp64_denom(weighted):
    c = RG.gspo_case(257, 5)
    kw = dict(beta=0.04, mode="token", max_len=5, denom=R.GRPO_DENOM,
              w=RI.weight_case((257, 5)) if weighted else None)
    agree("grpo_loss_seq_denom", BG.gspo(**c, **kw), RG.gspo64(**c, **kw))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_fp64_closed_form_gradient_is_the_autograd_gradient(mode, beta, weighted):
    c = RG.gspo_case(300, 257)
    kw = dict(beta=beta, mode=mode, max_len=257, w=RI.weight_case((300, 257)) if weighted else None)
    closed, auto = RG.gspo64(**c, **kw), RG.gspo64(**c, **kw, autograd=True)
    assert torch.equal(closed["loss"], auto["loss"]) and torch.equal(closed["metrics"], auto["metrics"])
    scale = closed["dlp"].abs().max().item()
    assert scale > 0 and (closed["dlp"] - auto["dlp"]).abs().max().item() <= 1e-12 * scale


# ------------------------------------------------------- sequence level vs token level
def _on_policy_case(S=8, T=64, seed=0):
    """Rows of 1, 2, 4 ... action tokens and S a power of two: in `sequence` mode every factor of the
    gradient scale 1 / (c_s S) is then a power of two, so summing a row's c_s equal contributions and
    dividing by c_s again (the path through the row mean) is exact, as the token path's product is."""
    g = R.gen(17000 + seed)
    lp = -4.0 * torch.rand(S, T, generator=g)
    ref = lp + 0.3 * torch.randn(S, T, generator=g)
    adv = R._adv_away_from_zero((S,), g)
    lens = torch.tensor([2 ** (i % 7) for i in range(S)])
    m = (torch.arange(T)[None, :] < lens[:, None]).float()
    return lp, ref, adv, m


def test_on_policy_sequence_level_is_the_token_level():
    """old_logp=None: d = 0 exactly, so sr_s = rho = 1 and nothing is clipped at either level."""
    lp, ref, adv, m = _on_policy_case()
    out = {}
    for level in GRPO_IMPORTANCE_LEVELS:
        x = lp.clone().requires_grad_(True)
        loss, met = ops.grpo_loss(x, None, ref, adv, m, 0.2, 0.28, 0.0, "sequence", importance_level=level)
        (g,) = torch.autograd.grad(loss, x)
        assert met["clipfrac"].item() == 0 and met["approx_kl"].item() == 0
        out[level] = (loss.detach(), g)
    assert torch.equal(out["sequence"][0], out["token"][0]) and torch.equal(out["sequence"][1], out["token"][1])
    assert out["token"][1].abs().sum() > 0


@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_on_policy_general_rows_agree_to_round_off(mode, beta):
    """Any row lengths and beta: equal loss; the gradient through the row mean sums c_s equal
    terms and divides by c_s, which rounds (a few ulp of the gradient's scale)."""
    c = RG.gspo_case(300, 257)
    out = {}
    for level in GRPO_IMPORTANCE_LEVELS:
        x = c["lp"].clone().requires_grad_(True)
        loss, _ = ops.grpo_loss(x, None, c["ref"], c["adv"], c["m"], 0.2, 0.28, beta, mode, 257,
                                importance_level=level)
        (g,) = torch.autograd.grad(loss, x)
        out[level] = (loss.detach(), g)
    assert torch.equal(out["sequence"][0], out["token"][0])
    on = c["m"] != 0  # (off the mask the token level keeps beta * junk * 0 terms; the sequence level selects them away)
    torch.testing.assert_close(out["sequence"][1][on], out["token"][1][on], rtol=1e-5, atol=0)


@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_single_token_rows_fp64_sequence_level_is_grpo64(mode, beta):
    """c_s = 1: l_s = d and sr_s = rho at the row's one action token."""
    c = R.grpo_case(300, 257)
    pos = torch.randint(0, 257, (300,), generator=R.gen(5))
    m = torch.zeros(300, 257)
    m[torch.arange(300), pos] = 1.0
    m[150] = 0.0
    c["m"] = m
    a, b = RG.gspo64(**c, beta=beta, mode=mode, max_len=257), R.grpo64(**c, beta=beta, mode=mode, max_len=257)
    for k in b:
        assert torch.equal(a[k], b[k]), k
    assert a["metrics"][0] > 0 and a["dlp"].abs().sum() > 0


def test_token_level_keyword_is_todays_call():
    c = R.grpo_case(257, 5)
    w = RI.weight_case((257, 5))
    for iw in (None, w):
        for fn in (ops.grpo_loss, _ref_grpo_loss):
            res = []
            for kw in ({}, {"importance_level": "token"}):
                x = c["lp"].clone().requires_grad_(True)
                loss, met = fn(x, c["old"], c["ref"], c["adv"], c["m"], 0.2, 0.28, 0.04, "token", is_weight=iw, **kw)
                (g,) = torch.autograd.grad(loss, x)
                res.append((loss.detach(), g, met))
            (l0, g0, m0), (l1, g1, m1) = res
            assert torch.equal(l0, l1) and torch.equal(g0, g1) and all(torch.equal(m0[k], m1[k]) for k in m0)


# ------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_garbage_outside_the_mask_changes_no_output(mode, weighted):
    c = RG.gspo_case(6, 257)
    w = RI.weight_case((6, 257)) if weighted else None
    kw = dict(beta=0.04, mode=mode, max_len=257)
    base = BG.gspo(**c, **kw, w=w)
    off = c["m"] == 0
    for junk in (0.0, float("nan"), float("inf"), -1e30):
        g = {k: (torch.where(off, torch.full_like(v, junk), v) if v.dim() == 2 and k != "m" else v) for k, v in c.items()}
        gw = None if w is None else torch.where(off, torch.full_like(w, junk), w)
        got = BG.gspo(**g, **kw, w=gw)
        for k in base:
            assert torch.equal(got[k], base[k]), (junk, k)


@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_all_zero_mask(mode):
    c = RG.gspo_case(6, 257)
    c["m"] = torch.zeros_like(c["m"])
    got = BG.gspo(**c, beta=0.04, mode=mode, max_len=257, w=RI.weight_case((6, 257)))
    assert got["loss"].item() == 0 and (got["dlp"] == 0).all() and (got["metrics"] == 0).all()


def test_fully_masked_rows_contribute_nothing():
    c = RG.gspo_case(300, 257)
    dead = c["m"].sum(1) == 0
    assert dead.sum() >= 2
    got = BG.gspo(**c, beta=0.04, mode="token", max_len=257)
    assert (got["dlp"][dead] == 0).all()
    keep = {k: v[~dead] for k, v in c.items()}
    less = BG.gspo(**keep, beta=0.04, mode="token", max_len=257)
    torch.testing.assert_close(less["loss"], got["loss"], rtol=1e-6, atol=0)
    assert torch.equal(less["metrics"][3], got["metrics"][3])


# -------------------------------------------------------------------- argument checks
def test_bad_level_raises():
    c = R.grpo_case(3, 7)
    for fn in (ops.grpo_loss, _ref_grpo_loss):
        for bad in ("rollout", "seq", "", None, 1):
            with pytest.raises(ValueError, match="importance_level"):
                fn(c["lp"], c["old"], c["ref"], c["adv"], c["m"], importance_level=bad)
    with pytest.raises(TypeError):  # keyword-only in the public op
        ops.grpo_loss(c["lp"], c["old"], c["ref"], c["adv"], c["m"], 0.2, 0.28, 0.04, "sequence", None, None, None,
                      "sequence")


def test_start_up_validation():
    from distributed_llm_alignment_amd.training import train_rlhf as tr

    assert tr.importance_sampling_level({}, "grpo") == "token"
    for algo in ("reinforce", "ppo", "grpo"):
        assert tr.importance_sampling_level({"importance_sampling_level": "token"}, algo) == "token"
    assert tr.importance_sampling_level({"importance_sampling_level": "Sequence"}, "grpo") == "sequence"
    for bad in ("rollout", "batch", "", None, False, 1):
        with pytest.raises(ValueError, match="importance_sampling_level"):
            tr.importance_sampling_level({"importance_sampling_level": bad}, "grpo")
    for algo in ("ppo", "reinforce"):
        with pytest.raises(ValueError, match="importance_sampling_level"):
            tr.importance_sampling_level({"importance_sampling_level": "sequence"}, algo)


def test_shipped_config_loads_and_validates():
    from distributed_llm_alignment_amd.training import train_rlhf as tr

    ppo = load_config(ROOT / "config" / "rlhf_gspo_llama3_8b.yaml")["ppo"]
    assert ppo["algorithm"] == "grpo"
    assert tr.importance_sampling_level(ppo, ppo["algorithm"]) == "sequence"
    assert (ppo["clip_range"], ppo["clip_range_high"], ppo["kl_coef"]) == (3e-4, 4e-4, 0.0)
    assert ppo["loss_type"] in R.GRPO_MODES and ppo["batch_size"] % ppo["group_size"] == 0
    assert ppo["ppo_epochs"] * ppo["num_minibatches"] > 1  # else every update is on-policy and sr_s = 1
    tr.rollout_is_settings(ppo)
    assert tr.logprob_temperature(ppo, "grpo") == 1.0 and tr.rollout_logprobs_mode(ppo, "grpo") == "off"
    base = load_config(ROOT / "config" / "rlhf_grpo_llama3_8b.yaml")["ppo"]
    differ = {k for k in set(ppo) | set(base) if ppo.get(k) != base.get(k)}
    assert differ == {"importance_sampling_level", "clip_range", "clip_range_high", "kl_coef", "num_minibatches"}


# --------------------------------------------------------------------- update, trainer
class _NoSyncEngine:
    def no_sync(self):
        import contextlib

        return contextlib.nullcontext()


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("loss_type", R.GRPO_MODES)
def test_grpo_update_micro_batches_sum_to_the_full_gradient(loss_type):
    """The tiny model, off-policy old log-probs: micro-batches of whole rows that share `denom` sum
    to the one-batch gradient (the tolerance of test_entropy_cpu's token-level counterpart)."""
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.objectives import grpo_rollout_stats
    from distributed_llm_alignment_amd.training.train_rlhf import grpo_update

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
    stats = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04, need_old=True)
    rows = {k: stats.get(k) for k in ("act", "advantages", "ref_logp", "old_logp")}
    # row means of d = 0.25, -0.25, 0.1, -0.1 (+ noise): rows on both sides of the clip range
    shift = torch.tensor([0.25, -0.25, 0.1, -0.1])[:, None]
    rows["old_logp"] = (rows["old_logp"] - shift + 0.05 * torch.randn(S, T, generator=g)) * rows["act"]
    args = (0.2, 0.1, 0.04, loss_type, 9)
    policy.zero_grad(set_to_none=True)
    full, mf = grpo_update(policy, _NoSyncEngine(), seqs, mask, rows, *args, micro=0, importance_level="sequence")
    gf = _grads(policy)
    policy.zero_grad(set_to_none=True)
    part, mp = grpo_update(policy, _NoSyncEngine(), seqs, mask, rows, *args, micro=2, importance_level="sequence")
    gp = _grads(policy)
    policy.zero_grad(set_to_none=True)
    assert math.isfinite(float(full)) and all(k in mf for k in ("clipfrac", "approx_kl", "kl_ref", "kl", "tokens"))
    assert 0 < float(mf["clipfrac"]) < 1 and float(mf["approx_kl"]) > 0
    assert gf.keys() == gp.keys() and len(gf) == len(list(policy.parameters()))
    assert any(gf[k].abs().sum() > 0 for k in gf)
    for k in gf:
        assert torch.allclose(gp[k], gf[k], atol=1e-7, rtol=1e-5), k
    assert abs(float(part) - float(full)) < 1e-6
    for k in ("clipfrac", "approx_kl", "kl_ref"):  # token-weighted aggregation over micro-batches is exact
        torch.testing.assert_close(mp[k], mf[k], rtol=1e-5, atol=1e-7)
    # and it is not the token level
    tok, mt = grpo_update(policy, _NoSyncEngine(), seqs, mask, rows, *args, micro=0)
    policy.zero_grad(set_to_none=True)
    assert float(tok) != float(full)


@pytest.fixture(scope="module")
def prompts(tmp_path_factory):
    d = tmp_path_factory.mktemp("gspodata")
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


def test_trainer_runs_at_the_sequence_level_and_logs_it_once(tmp_path, prompts):
    import json

    from distributed_llm_alignment_amd.training import train_rlhf

    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, [
        "ppo.algorithm=grpo", "ppo.importance_sampling_level=sequence", "ppo.ppo_epochs=2",
        "ppo.update_micro_batch=2", "ppo.clip_range=3e-4", "ppo.clip_range_high=4e-4"])) == 0
    m = [json.loads(l) for l in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(m) == 2 and all(math.isfinite(r["train/loss"]) for r in m)
    assert all(math.isfinite(r["train/clipfrac"]) and math.isfinite(r["train/approx_kl"]) for r in m)
    assert [("train/importance_sampling_level" in r) for r in m] == [True, False]
    assert m[0]["train/importance_sampling_level"] == 1


def test_trainer_rejects_bad_or_misplaced_level(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    for extra in (["ppo.algorithm=grpo", "ppo.importance_sampling_level=rollout"],
                  ["ppo.algorithm=ppo", "ppo.importance_sampling_level=sequence"],
                  ["ppo.algorithm=reinforce", "ppo.importance_sampling_level=sequence"]):
        with pytest.raises(ValueError, match="importance_sampling_level"):
            train_rlhf.main(_rlhf_args(tmp_path, prompts, extra))
