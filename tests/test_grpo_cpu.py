"""GRPO on the CPU tier: the torch formulas of `ops.group_advantages` / `ops.grpo_loss` against
independent implementations written here, the micro-batch identity of `denom`, group rollouts
of `generate(num_return_sequences=G)` on the fallback paths, and the trainer branch."""
from pathlib import Path

import numpy as np
import pytest
import torch

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.models import KVCache, build_model, generate, get_config, prefill_shared
from distributed_llm_alignment_amd.utils.config import load_config

ROOT = Path(__file__).resolve().parents[1]
LOSS_TYPES = ("sequence", "token", "constant")
CLIP_LOW, CLIP_HIGH = 0.2, 0.28
S, T, MAX_LEN = 6, 37, 40


# ------------------------------------------------------------------------- group_advantages
@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("scale_std", [True, False])
def test_group_advantages_matches_numpy(G, scale_std):
    P, eps = 4, 1e-4
    g = torch.Generator().manual_seed(G)
    r = torch.randn(P, G, generator=g)
    r[2] = 0.7  # one group of constant rewards
    adv, met = ops.group_advantages(r.reshape(-1), G, scale_std=scale_std, eps=eps)
    x = r.numpy().astype(np.float64)
    want = np.zeros_like(x)
    sds = np.zeros(P)
    for p in range(P):
        mu = x[p].sum() / G
        sds[p] = np.sqrt(((x[p] - mu) ** 2).sum() / G)
        want[p] = (x[p] - mu) / (sds[p] + eps) if scale_std else x[p] - mu
    want[2], sds[2] = 0.0, 0.0
    assert adv.shape == (P * G,) and not adv.requires_grad
    got = adv.reshape(P, G)
    assert torch.isfinite(got).all()
    assert (got[2] == 0).all()  # exactly zero, never NaN
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-4, atol=1e-6)
    assert abs(float(met["frac_zero_std"]) - 0.25) < 1e-7
    assert abs(float(met["reward_std"]) - sds.mean()) < 1e-5
    if not scale_std:  # the plain centred rewards
        centred = x - x.mean(1, keepdims=True)
        centred[2] = 0.0
        np.testing.assert_allclose(got.numpy(), centred, rtol=1e-5, atol=1e-6)


def test_group_advantages_rejects_ragged_groups():
    with pytest.raises(ValueError):
        ops.group_advantages(torch.zeros(7), 2)


# -------------------------------------------------------------------------------- grpo_loss
def grpo_inputs(seed=0, S=S, T=T, device="cpu"):
    """[S, T] grids with one fully masked row, advantages of both signs and one zero, and
    old = lp + 0.3 * randn (about 40 % of |d| outside the clip range)."""
    g = torch.Generator().manual_seed(seed)
    lp = -torch.rand(S, T, generator=g) * 3 - 0.05
    old = lp + 0.3 * torch.randn(S, T, generator=g)
    ref = lp + 0.2 * torch.randn(S, T, generator=g)
    mask = (torch.rand(S, T, generator=g) > 0.3).float()
    mask[:, :5] = 0  # prompt
    mask[3] = 0  # a fully masked row
    adv = torch.tensor([1.3, -0.8, 0.0, 0.5, -1.7, 0.9])[:S].clone()
    if S > 6:
        adv = torch.cat([adv, torch.randn(S - 6, generator=g)])
    return [t.to(device) for t in (lp, old, ref, adv, mask)]


def independent_grpo(lp, old, ref, adv, mask, clip_low, clip_high, beta, loss_type, max_len):
    """An implementation that shares no code with ops.losses: plain torch ops, autograd."""
    A = adv[:, None].expand_as(lp)
    ratio = torch.exp(lp - old)
    surr1 = A * ratio
    surr2 = A * torch.clamp(ratio, 1.0 - clip_low, 1.0 + clip_high)
    per = -torch.minimum(surr1, surr2)
    log_r = ref - lp
    k3 = torch.exp(log_r) - log_r - 1.0
    per = per + beta * k3
    rows = lp.shape[0]
    if loss_type == "sequence":
        loss = sum((per[s] * mask[s]).sum() / max(float(mask[s].sum()), 1.0) for s in range(rows)) / rows
    elif loss_type == "token":
        loss = (per * mask).sum() / max(float(mask.sum()), 1.0)
    else:
        loss = (per * mask).sum() / (rows * max_len)
    n = max(float(mask.sum()), 1.0)
    ratio, k3 = ratio.detach(), k3.detach()
    lp = lp.detach()
    metrics = {
        "clipfrac": float((((ratio < 1 - clip_low) | (ratio > 1 + clip_high)).float() * mask).sum() / n),
        "approx_kl": float((((ratio - 1) - (lp - old)) * mask).sum() / n),
        "kl_ref": float((k3 * mask).sum() / n),
        "tokens": float(mask.sum()),
    }
    return loss, metrics


def assert_inputs_exercise_every_branch(lp, old, adv, mask):
    rho = torch.exp(lp - old)
    A = adv[:, None].expand_as(lp)
    m = mask.bool()
    assert (m & (rho >= 1 - CLIP_LOW) & (rho <= 1 + CLIP_HIGH) & (A != 0)).any()  # unclipped
    assert (m & (rho > 1 + CLIP_HIGH) & (A > 0)).any()  # clipped high, A > 0
    assert (m & (rho < 1 - CLIP_LOW) & (A < 0)).any()  # clipped low, A < 0
    assert (mask.sum(1) == 0).any() and (adv == 0).any() and (adv > 0).any() and (adv < 0).any()


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("beta", [0.0, 0.04])
def test_grpo_loss_matches_independent_autograd(loss_type, beta):
    lp, old, ref, adv, mask = grpo_inputs()
    assert_inputs_exercise_every_branch(lp, old, adv, mask)
    a = lp.clone().requires_grad_(True)
    loss, met = ops.grpo_loss(a, old, ref, adv, mask, clip_low=CLIP_LOW, clip_high=CLIP_HIGH, beta=beta,
                              loss_type=loss_type, max_len=MAX_LEN)
    loss.backward()
    b = lp.clone().requires_grad_(True)
    want, wmet = independent_grpo(b, old, ref, adv, mask, CLIP_LOW, CLIP_HIGH, beta, loss_type, MAX_LEN)
    want.backward()
    assert abs(loss.item() - want.item()) < 1e-6
    for k, v in wmet.items():
        assert abs(float(met[k]) - v) < 1e-6, k
    assert torch.allclose(a.grad, b.grad, atol=1e-7, rtol=1e-5)
    assert (a.grad[3] == 0).all()  # the fully masked row


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_grpo_micro_batches_with_denom_sum_to_full_gradient(loss_type):
    lp, old, ref, adv, mask = grpo_inputs(1)
    kw = dict(clip_low=CLIP_LOW, clip_high=CLIP_HIGH, beta=0.04, loss_type=loss_type, max_len=MAX_LEN)
    a = lp.clone().requires_grad_(True)
    full, _ = ops.grpo_loss(a, old, ref, adv, mask, **kw)
    full.backward()
    denom = {"sequence": torch.tensor([float(S)]), "token": mask.sum().clamp(min=1).reshape(1),
             "constant": torch.tensor([float(S * MAX_LEN)])}[loss_type]
    b = lp.clone().requires_grad_(True)
    tot = 0.0
    for s0 in range(0, S, 2):
        sl = slice(s0, s0 + 2)
        part, _ = ops.grpo_loss(b[sl], old[sl], ref[sl], adv[sl], mask[sl], denom=denom, **kw)
        part.backward()
        tot = tot + part.detach()
    assert torch.allclose(b.grad, a.grad, atol=1e-7, rtol=1e-5)
    assert abs(tot.item() - full.item()) < 1e-6


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_grpo_on_policy_gradient_is_minus_advantage(loss_type):
    lp, _, _, adv, mask = grpo_inputs(2)
    a = lp.clone().requires_grad_(True)
    loss, met = ops.grpo_loss(a, None, None, adv, mask, clip_low=CLIP_LOW, clip_high=CLIP_HIGH, beta=0.0,
                              loss_type=loss_type, max_len=MAX_LEN)
    loss.backward()
    c = mask.sum(1).clamp(min=1)
    w = 1.0 / c if loss_type == "sequence" else torch.ones(S)
    div = {"sequence": float(S), "token": float(mask.sum()), "constant": float(S * MAX_LEN)}[loss_type]
    want = -adv[:, None] * mask * w[:, None] / div
    torch.testing.assert_close(a.grad, want, rtol=1e-6, atol=0)
    assert float(met["clipfrac"]) == 0 and float(met["approx_kl"]) == 0 and float(met["kl_ref"]) == 0


def test_grpo_loss_argument_checks():
    lp, old, ref, adv, mask = grpo_inputs()
    with pytest.raises(ValueError):
        ops.grpo_loss(lp, old, None, adv, mask, beta=0.04)  # no reference with beta != 0
    with pytest.raises(ValueError):
        ops.grpo_loss(lp, old, ref, adv, mask, loss_type="constant")  # needs max_len
    with pytest.raises(ValueError):
        ops.grpo_loss(lp, old, ref, adv, mask, loss_type="mean")
    # clip_high=None means clip_low
    a, _ = ops.grpo_loss(lp, old, ref, adv, mask, clip_low=0.2)
    b, _ = ops.grpo_loss(lp, old, ref, adv, mask, clip_low=0.2, clip_high=0.2)
    assert float(a) == float(b)


# ------------------------------------------------------------------------- group rollouts
@pytest.fixture(scope="module")
def tiny():
    cfg = get_config("tiny-llama")
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=0).eval()
    g = torch.Generator().manual_seed(3)
    P, Tp = 3, 11
    ids = torch.randint(3, cfg.vocab_size, (P, Tp), generator=g)
    am = torch.ones(P, Tp, dtype=torch.long)
    am[1, :4] = 0  # one left-padded prompt
    ids[1, :4] = 0
    return model, ids, am


def test_generate_group_shapes_order_and_greedy_rows(tiny):
    model, ids, am = tiny
    P, Tp = ids.shape
    G, n = 3, 6
    kw = dict(max_new_tokens=n, do_sample=False, eos_token_id=-1, pad_token_id=0, return_mask=True)
    one, one_m = generate(model, ids, am, **kw)
    seqs, mask = generate(model, ids, am, num_return_sequences=G, **kw)
    assert seqs.shape == (P * G, Tp + n) and mask.shape == (P * G, Tp + n)
    for p in range(P):
        for g in range(G):  # row p*G + g is sample g of prompt p; greedy: exactly the G = 1 row
            assert torch.equal(seqs[p * G + g], one[p])
            assert torch.equal(mask[p * G + g], one_m[p])
    rep, rep_m = generate(model, ids, am, num_return_sequences=G, share_prefill=False, **kw)
    assert torch.equal(rep, seqs) and torch.equal(rep_m, mask)


def test_generate_group_of_one_is_todays_call(tiny):
    model, ids, am = tiny
    kw = dict(max_new_tokens=5, do_sample=True, temperature=0.9, eos_token_id=-1, pad_token_id=0,
              return_mask=True)
    a, am_a = generate(model, ids, am, generator=torch.Generator().manual_seed(5), **kw)
    b, am_b = generate(model, ids, am, generator=torch.Generator().manual_seed(5), num_return_sequences=1, **kw)
    assert torch.equal(a, b) and torch.equal(am_a, am_b)


def test_generate_group_samples_differ_within_a_group(tiny):
    model, ids, am = tiny
    G = 4
    torch.manual_seed(0)
    seqs = generate(model, ids, am, max_new_tokens=8, do_sample=True, temperature=1.0, eos_token_id=-1,
                    pad_token_id=0, num_return_sequences=G)
    new = seqs[:, ids.shape[1]:].reshape(ids.shape[0], G, -1)
    assert any(not torch.equal(new[p, 0], new[p, g]) for p in range(ids.shape[0]) for g in range(1, G))
    assert torch.equal(seqs[:, :ids.shape[1]], ids.repeat_interleave(G, 0))


def test_prefill_shared_matches_repeated_prefill(tiny):
    model, ids, am = tiny
    P, Tp = ids.shape
    G, max_len = 3, Tp + 4
    from distributed_llm_alignment_amd.models import attention_layout

    with torch.no_grad():
        cache, h_last = prefill_shared(model, ids, am, G, max_len)
        kv_start = attention_layout(am)[0].repeat_interleave(G)
        full = KVCache(model, P * G, max_len, kv_start)
        h = model(ids.repeat_interleave(G, 0), cache=full)
    assert cache.len == Tp == full.len and cache.batch == P * G
    assert torch.equal(cache.kv_start, full.kv_start)
    assert torch.allclose(cache.k[:, :, :Tp], full.k[:, :, :Tp], atol=1e-5)
    assert torch.allclose(cache.v[:, :, :Tp], full.v[:, :, :Tp], atol=1e-5)
    assert torch.allclose(h_last, h[:, -1], atol=1e-5)
    assert torch.equal(cache.pos, full.pos) and torch.equal(cache.slot, full.slot)


def test_kv_replicate_fallback_leaves_the_tail_alone():
    L, P, G, Tp, H, D = 2, 3, 2, 5, 2, 8
    g = torch.Generator().manual_seed(0)
    sk, sv = torch.randn(L, P, Tp, H, D, generator=g), torch.randn(L, P, Tp, H, D, generator=g)
    dk = torch.full((L, P * G, H, Tp + 3, D), 7.0).transpose(2, 3)  # head-major storage behind the view
    dv = torch.full((L, P * G, Tp + 3, H, D), 7.0)
    ops.decode.kv_replicate(sk, sv, dk, dv, G)
    assert torch.equal(dk[:, :, :Tp], sk.repeat_interleave(G, 1)) and torch.equal(dv[:, :, :Tp], sv.repeat_interleave(G, 1))
    assert (dk[:, :, Tp:] == 7).all() and (dv[:, :, Tp:] == 7).all()
    # the layer-split list form: per layer
    lk, lv = [sk[i] for i in range(L)], [sv[i] for i in range(L)]
    ok = [torch.zeros(P * G, Tp + 3, H, D) for _ in range(L)]
    ov = [torch.zeros(P * G, Tp + 3, H, D) for _ in range(L)]
    ops.decode.kv_replicate(lk, lv, ok, ov, G)
    assert all(torch.equal(ok[i][:, :Tp], sk[i].repeat_interleave(G, 0)) for i in range(L))
    assert all((ov[i][:, Tp:] == 0).all() for i in range(L))


# ---------------------------------------------------------------------------------- trainer
@pytest.fixture(scope="module")
def prompts(tmp_path_factory):
    d = tmp_path_factory.mktemp("grpodata")
    write_jsonl(d / "prompts.jsonl", synthetic_prompt_records(6, seed=4))
    return d / "prompts.jsonl"


def _rlhf_args(tmp, prompts, extra):
    ov = ["optimization.max_train_steps=2", f"logging.output_dir={tmp / 'ck'}", f"logging.log_dir={tmp / 'logs'}",
          "logging.save_every_steps=0", "logging.use_wandb=false", "data.num_workers=0",
          "hardware.gradient_accumulation_steps=1",
          "model.policy_model_name_or_path=tiny-llama", "model.reference_model_name_or_path=tiny-llama",
          "model.max_seq_length=48", "reward_model.path=null", "reward_model.base_model_name_or_path=tiny-llama",
          "ppo.batch_size=2", "ppo.steps=2", "ppo.generation_params.max_new_tokens=4",
          "sampling.source=local", f"sampling.prompt_path={prompts}", *extra]
    args = ["--config", str(ROOT / "config" / "rlhf_config.yaml")]
    for o in ov:
        args += ["--override", o]
    return args


@pytest.mark.parametrize("extra", [[], ["ppo.update_micro_batch=2", "ppo.loss_type=token"],
                                   ["ppo.ppo_epochs=2", "ppo.loss_type=constant", "ppo.scale_rewards=false"]])
def test_grpo_trainer_runs(tmp_path, prompts, extra):
    from distributed_llm_alignment_amd.training import train_rlhf

    grpo = ["ppo.algorithm=grpo", "ppo.group_size=2", "ppo.batch_size=4", "logging.log_every_steps=1"]
    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, grpo + extra)) == 0


def test_grpo_trainer_rejects_a_batch_that_splits_a_group(tmp_path, prompts):
    from distributed_llm_alignment_amd.training import train_rlhf

    with pytest.raises(ValueError, match="group_size"):
        train_rlhf.main(_rlhf_args(tmp_path, prompts, ["ppo.algorithm=grpo", "ppo.group_size=2", "ppo.batch_size=3"]))


def test_grpo_shipped_config_loads():
    cfg = load_config(ROOT / "config" / "rlhf_grpo_llama3_8b.yaml")
    ppo = cfg["ppo"]
    assert ppo["algorithm"] == "grpo" and "critic" not in cfg
    assert (ppo["batch_size"], ppo["group_size"], ppo["update_micro_batch"]) == (64, 8, 8)
    assert ppo["batch_size"] % ppo["group_size"] == 0 and ppo["loss_type"] in LOSS_TYPES
