"""CPU tier: the policy-entropy output of the LM-head log-prob path (ops.linear_logprob_entropy,
the vocab-parallel twin, token_logprobs(with_entropy=True)) and the PPO / GRPO entropy bonus
(`ppo.entropy_coef`, `ppo.log_entropy`). The torch paths tested here are the formula of record
the HIP kernels are held to in test_entropy_gpu.py."""
import json
import math

import pytest
import torch

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import write_jsonl
from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records
from distributed_llm_alignment_amd.models import build_model, get_config
from distributed_llm_alignment_amd.objectives import (action_mask, grpo_loss, grpo_rollout_stats, ppo_loss,
                                                      ppo_rollout_stats)
from distributed_llm_alignment_amd.parallel.tensor_parallel import _local_bwd_entropy, _local_fwd_entropy

from test_distributed_cpu import run_ranks
from test_grpo_cpu import _rlhf_args

NINF = float("-inf")


# ------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("V", [7, 1000])
def test_forward_matches_torch_categorical(V):
    g = torch.Generator().manual_seed(V)
    N, H = 12, 16
    hidden = torch.randn(N, H, generator=g, dtype=torch.float64).float()
    weight = torch.randn(V, H, generator=g, dtype=torch.float64).float()
    targets = torch.randint(0, V, (N,), generator=g)
    targets[3] = -100
    targets[8] = -1
    lp, ent = ops.linear_logprob_entropy(hidden, weight, targets)
    assert lp.dtype == torch.float32 and ent.dtype == torch.float32 and lp.shape == ent.shape == (N,)
    want = torch.distributions.Categorical(logits=hidden.double() @ weight.double().t()).entropy().float()
    live = targets >= 0
    torch.testing.assert_close(ent[live], want[live], rtol=1e-5, atol=1e-6)
    assert (lp[~live] == 0).all() and (ent[~live] == 0).all()
    assert torch.equal(lp, ops.linear_logprob(hidden, weight, targets))


# ------------------------------------------------------------------------------ 2. backward
def _autograd_reference(logits, targets, a, b):
    """d/dlogits of sum(a * logp + b * ent) through log_softmax, in fp64."""
    z = logits.double().clone().requires_grad_(True)
    lsm = torch.log_softmax(z, -1)
    live = targets >= 0
    lp = lsm.gather(-1, targets.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    ent = -(lsm.exp() * lsm).sum(-1)
    (torch.where(live, a.double() * lp + b.double() * ent, torch.zeros_like(lp))).sum().backward()
    return z.grad


@pytest.mark.parametrize("V", [7, 1000])
def test_backward_formula_matches_autograd(V):
    g = torch.Generator().manual_seed(10 + V)
    N = 9
    logits = 3 * torch.randn(N, V, generator=g)
    targets = torch.randint(0, V, (N,), generator=g)
    targets[2] = -100
    a, b = torch.randn(N, generator=g), torch.randn(N, generator=g)
    lp, lse, ent = _local_fwd_entropy(logits, targets, 0)
    got = _local_bwd_entropy(logits, targets, lse, ent, a, b, 0)
    want = _autograd_reference(logits, targets, a, b)
    torch.testing.assert_close(got, want.float(), atol=1e-6, rtol=1e-5)
    assert (got[2] == 0).all()
    torch.testing.assert_close(ent, torch.distributions.Categorical(logits=logits).entropy(), rtol=1e-5, atol=1e-6)
    # the op's own autograd (the plain-torch formula of record) agrees with the hand-written one
    H = 5
    hidden = torch.randn(N, H, generator=g).requires_grad_(True)
    weight = torch.randn(V, H, generator=g).requires_grad_(True)
    olp, oent = ops.linear_logprob_entropy(hidden, weight, targets)
    (a * olp + b * oent).sum().backward()
    with torch.no_grad():
        lg = hidden @ weight.t()
        _, lse2, ent2 = _local_fwd_entropy(lg, targets, 0)
        dl = _local_bwd_entropy(lg, targets, lse2, ent2, a, b, 0)
    torch.testing.assert_close(hidden.grad, dl @ weight.detach(), atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(weight.grad, dl.t() @ hidden.detach(), atol=1e-5, rtol=1e-4)


def test_minus_inf_logits_have_finite_entropy_and_zero_gradient():
    g = torch.Generator().manual_seed(5)
    N, V = 4, 11
    logits = torch.randn(N, V, generator=g)
    logits[1, 0] = NINF
    logits[1, 6] = NINF
    targets = torch.tensor([3, 2, 5, 9])
    a, b = torch.randn(N, generator=g), torch.randn(N, generator=g)
    lp, lse, ent = _local_fwd_entropy(logits, targets, 0)
    assert torch.isfinite(ent).all()
    keep = [v for v in range(V) if v not in (0, 6)]
    want = torch.distributions.Categorical(logits=logits[1, keep]).entropy()
    torch.testing.assert_close(ent[1], want, rtol=1e-5, atol=1e-6)
    d = _local_bwd_entropy(logits, targets, lse, ent, a, b, 0)
    assert torch.isfinite(d).all()
    assert (d[1, [0, 6]] == 0).all()
    sub = _autograd_reference(logits[1:2, keep], torch.tensor([keep.index(2)]), a[1:2], b[1:2])
    torch.testing.assert_close(d[1, keep], sub[0].float(), atol=1e-6, rtol=1e-5)


# -------------------------------------------------------------------- 3. vocabulary parallel
VP_N, VP_V, VP_H = 10, 64, 12


def _vp_inputs():
    g = torch.Generator().manual_seed(21)
    hidden = torch.randn(VP_N, VP_H, generator=g)
    weight = 0.25 * torch.randn(VP_V, VP_H, generator=g)  # O(1) gradients under the absolute tolerance
    targets = torch.tensor([1, 17, 33, 49, 62, 15, -100, 40, 31, 5])  # a target on each of 4 shards
    a, b = torch.randn(VP_N, generator=g), torch.randn(VP_N, generator=g)
    return hidden, weight, targets, a, b


def _vp_rank(rank, world):
    import torch

    from distributed_llm_alignment_amd.parallel.tensor_parallel import vocab_parallel_logprob_entropy

    hidden, weight, targets, a, b = _vp_inputs()
    Vl = VP_V // world
    h = hidden.clone().requires_grad_(True)
    w = weight[rank * Vl:(rank + 1) * Vl].clone().requires_grad_(True)
    lp, ent = vocab_parallel_logprob_entropy(h, w, targets, rank * Vl, None)
    (a * lp + b * ent).sum().backward()
    return {"lp": lp, "ent": ent, "dh": h.grad, "dw": w.grad}


@pytest.mark.parametrize("world", [2, 4])
def test_vocab_parallel_matches_unsharded(world):
    hidden, weight, targets, a, b = _vp_inputs()
    h = hidden.clone().requires_grad_(True)
    w = weight.clone().requires_grad_(True)
    lp, ent = ops.linear_logprob_entropy(h, w, targets)
    (a * lp + b * ent).sum().backward()
    assert lp[6] == 0 and ent[6] == 0
    out = run_ranks(_vp_rank, world=world)
    Vl = VP_V // world
    for r in range(world):
        o = out[r]
        torch.testing.assert_close(o["lp"], lp.detach(), atol=1e-5, rtol=0)
        torch.testing.assert_close(o["ent"], ent.detach(), atol=1e-5, rtol=0)
        torch.testing.assert_close(o["dh"], h.grad, atol=1e-5, rtol=0)
        torch.testing.assert_close(o["dw"], w.grad[r * Vl:(r + 1) * Vl], atol=1e-5, rtol=0)
        assert o["lp"][6] == 0 and o["ent"][6] == 0


# ----------------------------------------------------------------------------- 4. objectives
@pytest.fixture(scope="module")
def rollouts():
    cfg = get_config("tiny-llama")
    policy = build_model(cfg, device="cpu", dtype=torch.float32, seed=0)
    ref = build_model(cfg, device="cpu", dtype=torch.float32, seed=1).requires_grad_(False)
    g = torch.Generator().manual_seed(7)
    S, Tp, T = 4, 5, 14
    seqs = torch.randint(3, cfg.vocab_size, (S, T), generator=g)
    mask = torch.ones(S, T, dtype=torch.long)
    mask[1, 11:] = 0  # padding after an early EOS
    mask[3, :2] = 0  # a left-padded prompt
    scores = torch.randn(S, generator=g)
    return cfg, policy, ref, seqs, mask, Tp, scores


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_token_logprobs_with_entropy(rollouts):
    cfg, policy, _, seqs, mask, _, _ = rollouts
    with torch.no_grad():
        lp = policy.token_logprobs(seqs, mask)
        lp2, ent = policy.token_logprobs(seqs, mask, with_entropy=True)
        logits = policy.logits(policy(seqs, mask)).float()
    assert torch.equal(lp, lp2) and ent.shape == lp.shape
    tgt, _ = ops.shifted_targets(seqs, mask)
    want = torch.distributions.Categorical(logits=logits).entropy()
    torch.testing.assert_close(ent, torch.where(tgt >= 0, want, torch.zeros_like(want)), rtol=1e-5, atol=1e-6)
    assert (ent[tgt >= 0] > 0).all() and (ent <= math.log(cfg.vocab_size) + 1e-5).all()


def test_grpo_loss_entropy_bonus(rollouts):
    cfg, policy, ref, seqs, mask, Tp, scores = rollouts
    stats = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04)
    base, m0 = grpo_loss(policy, seqs, mask, stats)
    assert "entropy" not in m0
    loss, m = grpo_loss(policy, seqs, mask, stats, entropy_coef=0.01)
    assert 0 < float(m["entropy"]) <= math.log(cfg.vocab_size)
    assert abs(loss.item() - (base.item() - 0.01 * m["entropy"].item())) < 1e-6
    with torch.no_grad():
        _, ent = policy.token_logprobs(seqs, mask, with_entropy=True)
    act = action_mask(mask, Tp)
    torch.testing.assert_close(m["entropy"], (ent * act).sum() / act.sum(), rtol=1e-6, atol=0)
    # log_entropy alone: the metric, the same loss and bitwise the same gradients
    policy.zero_grad(set_to_none=True)
    base.backward()
    g0 = _grads(policy)
    policy.zero_grad(set_to_none=True)
    logged, ml = grpo_loss(policy, seqs, mask, stats, log_entropy=True)
    logged.backward()
    g1 = _grads(policy)
    policy.zero_grad(set_to_none=True)
    assert torch.equal(logged, base) and torch.equal(ml["entropy"], m["entropy"])
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)
    # and the bonus does reach the gradients
    loss.backward()
    g2 = _grads(policy)
    policy.zero_grad(set_to_none=True)
    assert any(not torch.equal(g0[k], g2[k]) for k in g0)


def test_ppo_loss_entropy_bonus(rollouts):
    from distributed_llm_alignment_amd.models import build_value_model

    cfg, policy, ref, seqs, mask, Tp, scores = rollouts
    critic, _ = build_value_model("tiny-llama", device="cpu", seed=2)
    critic = critic.float()
    stats = ppo_rollout_stats(policy, ref, critic, seqs, mask, Tp, scores)
    base, m0 = ppo_loss(policy, critic, seqs, mask, stats)
    assert "entropy" not in m0
    loss, m = ppo_loss(policy, critic, seqs, mask, stats, entropy_coef=0.01)
    assert 0 < float(m["entropy"]) <= math.log(cfg.vocab_size)
    assert abs(loss.item() - (base.item() - 0.01 * m["entropy"].item())) < 1e-6
    logged, ml = ppo_loss(policy, critic, seqs, mask, stats, log_entropy=True)
    assert torch.equal(logged, base) and torch.equal(ml["entropy"], m["entropy"])


class _NoSyncEngine:
    def no_sync(self):
        import contextlib

        return contextlib.nullcontext()


@pytest.mark.parametrize("loss_type", ["sequence", "token"])
def test_grpo_update_micro_batches_sum_to_full_gradient(rollouts, loss_type):
    from distributed_llm_alignment_amd.training.train_rlhf import grpo_update

    cfg, policy, ref, seqs, mask, Tp, scores = rollouts
    stats = grpo_rollout_stats(policy, ref, seqs, mask, Tp, scores, 2, beta=0.04)
    rows = {k: stats.get(k) for k in ("act", "advantages", "ref_logp", "old_logp")}
    args = (0.2, None, 0.04, loss_type, 9)
    policy.zero_grad(set_to_none=True)
    full, mf = grpo_update(policy, _NoSyncEngine(), seqs, mask, rows, *args, micro=0, entropy_coef=0.01)
    gf = _grads(policy)
    policy.zero_grad(set_to_none=True)
    part, mp_ = grpo_update(policy, _NoSyncEngine(), seqs, mask, rows, *args, micro=2, entropy_coef=0.01)
    gp = _grads(policy)
    policy.zero_grad(set_to_none=True)
    assert gf.keys() == gp.keys() and len(gf) == len(list(policy.parameters()))
    for k in gf:
        assert torch.allclose(gp[k], gf[k], atol=1e-7, rtol=1e-5), k
    assert abs(float(part) - float(full)) < 1e-6
    torch.testing.assert_close(mp_["entropy"], mf["entropy"], rtol=1e-5, atol=1e-6)


# -------------------------------------------------------------------------------- 5. trainer
@pytest.fixture(scope="module")
def prompts(tmp_path_factory):
    d = tmp_path_factory.mktemp("entdata")
    write_jsonl(d / "prompts.jsonl", synthetic_prompt_records(6, seed=4))
    return d / "prompts.jsonl"


GRPO = ["ppo.algorithm=grpo", "ppo.group_size=2", "ppo.batch_size=4"]


@pytest.mark.parametrize("extra", [GRPO, GRPO + ["ppo.update_micro_batch=2"], ["ppo.algorithm=ppo"]],
                         ids=["grpo", "grpo-micro", "ppo"])
def test_trainer_logs_entropy(tmp_path, prompts, extra):
    from distributed_llm_alignment_amd.training import train_rlhf

    ov = extra + ["ppo.entropy_coef=0.01", "logging.log_every_steps=1"]
    assert train_rlhf.main(_rlhf_args(tmp_path, prompts, ov)) == 0
    recs = [json.loads(l) for l in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines() if l.strip()]
    recs = [r for r in recs if "train/loss" in r]
    assert len(recs) == 2
    top = math.log(get_config("tiny-llama").vocab_size)
    for r in recs:
        assert 0 < r["train/entropy"] <= top
