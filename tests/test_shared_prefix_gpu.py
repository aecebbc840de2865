"""Prefix sharing in the GRPO update on the GPU (tiny-llama-d128, bf16, native kernels): groups of
G = 4 rollouts of a 70-token prompt plus 40 generated tokens, one group left-padded.

  * hidden states of the segment slots against each rollout run alone: rel_err < 2e-2, the
    tolerance test_packed_model_matches_separate_gpu uses for the same kind of comparison;
  * log-probs: err_shared = max |lp_shared - lp32| against err_plain = max |lp_plain - lp32|,
    lp32 the same weights in fp32 on the CPU path. Both are bf16 roundings of one function:
    err_shared <= 2 * err_plain (the factor covers the maximum over a few thousand samples);
  * grpo_loss backward: parameter gradients against the plain path, rel_err < 2e-2;
  * two runs bitwise equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
G, P, N, GROUPS, LPAD = 4, 70, 40, 2, 9
T = P + N


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture(scope="module")
def setup():
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.ops import _ext

    _ext.require()
    cfg = get_config("tiny-llama-d128")
    model = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    g = torch.Generator().manual_seed(0)
    prompts = torch.randint(3, cfg.vocab_size, (GROUPS, P), generator=g)
    seqs = torch.cat([prompts.repeat_interleave(G, 0), torch.randint(3, cfg.vocab_size, (GROUPS * G, N), generator=g)], 1)
    mask = torch.ones_like(seqs)
    mask[G:2 * G, :LPAD] = 0  # the second group's prompt is left-padded
    mask[2, -7:] = 0  # right padding after an early EOS
    return cfg, model, seqs.to(DEV), mask.to(DEV)


def test_hidden_states_match_each_rollout_alone(setup):
    from distributed_llm_alignment_amd.models.transformer import shared_prefix_pack

    _, model, seqs, mask = setup
    S, Lp, n1 = seqs.shape[0], P - 1, T - P + 1
    with torch.no_grad():
        ids, pos, segs, prefix, _ = shared_prefix_pack(seqs, mask, P, G)
        hp = model(ids, None, packed=(pos, segs, prefix))
        worst = 0.0
        for i in range(S):
            end = int(mask[i].sum().item()) + (LPAD if i >= G else 0)  # one past the last real column
            hs = model(seqs[i:i + 1], mask[i:i + 1])
            o = Lp + (i % G) * n1
            e = rel_err(hp[i // G, o:o + end - Lp], hs[0, Lp:end])
            worst = max(worst, e)
            assert e < 2e-2, (i, e)
    print(f"FIG shared_prefix gpu hidden: worst rel_err {worst:.3e}")


def test_logprobs_against_fp32(setup):
    from distributed_llm_alignment_amd.models import build_model

    cfg, model, seqs, mask = setup
    m32 = build_model(cfg, device="cpu", dtype=torch.float32, seed=0)
    m32.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        lp32 = m32.token_logprobs(seqs.cpu(), mask.cpu())[:, P - 1:]
        plain = model.token_logprobs(seqs, mask)
        shared = model.token_logprobs(seqs, mask, shared_prefix=(G, P))
        again = model.token_logprobs(seqs, mask, shared_prefix=(G, P))
    assert torch.equal(shared, again)
    assert (shared[:, :P - 1] == 0).all()
    err_plain = (plain[:, P - 1:].cpu() - lp32).abs().max().item()
    err_shared = (shared[:, P - 1:].cpu() - lp32).abs().max().item()
    print(f"FIG shared_prefix gpu logprobs: err_shared {err_shared:.3e} err_plain {err_plain:.3e}")
    assert ((shared[:, P - 1:] == 0) == (plain[:, P - 1:] == 0)).all()
    assert err_shared <= 2.0 * err_plain


def test_grpo_loss_backward_matches_plain(setup):
    from distributed_llm_alignment_amd import objectives as O

    _, model, seqs, mask = setup
    S = seqs.shape[0]
    scores = torch.linspace(-1, 1, S, device=DEV)
    stats = O.grpo_rollout_stats(model, model, seqs, mask, P, scores, G, beta=0.04, need_old=True)
    stats["old_logp"] = stats["old_logp"] - 0.05
    stats["ref_logp"] = stats["ref_logp"] + 0.03
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]

    def run(**kw):
        model.zero_grad(set_to_none=True)
        loss, _ = O.grpo_loss(model, seqs, mask, stats, beta=0.04, **kw)
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for _, p in named]

    model.train()
    try:
        l0, g0 = run()
        l1, g1 = run(shared_prefix=(G, P))
        l2, g2 = run(shared_prefix=(G, P))
    finally:
        model.eval()
    worst = ("", 0.0)
    for (n, _), a, b, c in zip(named, g0, g1, g2):
        assert torch.equal(b, c), f"{n}: gradient differs between two shared runs"
        e = rel_err(b, a)
        worst = max(worst, (n, e), key=lambda x: x[1])
        assert e < 2e-2, (n, e)
    assert torch.equal(l1, l2)
    print(f"FIG shared_prefix gpu grpo_loss: loss {float(l0):.6f} / {float(l1):.6f} worst grad rel_err "
          f"{worst[1]:.3e} ({worst[0]})")
