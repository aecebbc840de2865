"""Prefix sharing in the GRPO update on the CPU path (fp32, tiny llama config): pack / unpack,
`token_logprobs(shared_prefix=)` and `grpo_loss(shared_prefix=)` against the plain calls, the
variants (entropy, temperature, keep mask) and the start-up errors of `ppo.share_prefix_update`.

Tolerance: the shared and the plain call evaluate one function in two fp32 summation orders. The
yardstick for such a difference is measured in place: the plain call on the whole batch against
the plain call row by row (`err_rows`). The shared call may differ from the plain one by 4 x that
figure, floor 1e-6. Both figures are printed.

On this CPU path a row's result does not depend on the other rows of the batch, so `err_rows` comes
out exactly 0 and says nothing about reorderings. The variants therefore also measure a second
yardstick of the same kind, `err_shift`: the plain call on the same rollouts with k = 1 .. 8 more
left-padding columns (every alignment of an 8-wide fp32 vector). Positions and the visible keys are
unchanged, so it is the same function, but the keys sit at other offsets of the row, which is what
packing does to them; the attention sums then run in another order. The log-prob variants keep
the rule above; the entropy, a second quantity the rule's yardstick does not cover, allows 4 x the
larger of its two yardsticks, floor 1e-6; `err_shift` is printed for all. (Why the entropy moves more than the log-prob: the formula
of record is -sum_v p_v lsm_v with p = exp(lsm) not renormalised, so one fp32 ulp on the row's lse
shifts every lsm and scales sum_v p_v, and the entropy moves by (1 + H) ulps, H about 6.2 here.)"""
import pytest
import torch

G, P, N = 3, 7, 5
T = P + N
CFG = "tiny-llama"


def _rollouts(vocab, groups=2, lpad=(2, 0), seed=0):
    g = torch.Generator().manual_seed(seed)
    prompts = torch.randint(3, vocab, (groups, P), generator=g)
    seqs = torch.cat([prompts.repeat_interleave(G, 0), torch.randint(3, vocab, (groups * G, N), generator=g)], 1)
    mask = torch.ones_like(seqs)
    for b, n in enumerate(lpad):
        mask[b * G:(b + 1) * G, :n] = 0
    mask[1, -2:] = 0  # right padding after an early EOS
    mask[4, -1:] = 0
    return seqs, mask


@pytest.fixture(scope="module")
def setup():
    from distributed_llm_alignment_amd.models import build_model, get_config

    cfg = get_config(CFG)
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=0)
    seqs, mask = _rollouts(cfg.vocab_size)
    with torch.no_grad():
        plain = model.token_logprobs(seqs, mask)
        rows = torch.cat([model.token_logprobs(seqs[i:i + 1], mask[i:i + 1]) for i in range(seqs.shape[0])])
    err_rows = (plain - rows)[:, P - 1:].abs().max().item()
    return model, seqs, mask, plain, err_rows


def _tol(err_rows):
    return max(4.0 * err_rows, 1e-6)


def test_pack_unpack_round_trip(setup):
    from distributed_llm_alignment_amd.models.transformer import shared_prefix_pack, shared_prefix_unpack

    _, seqs, mask, _, _ = setup
    S = seqs.shape[0]
    ids, pos, segs, prefix, slot_map = shared_prefix_pack(seqs, mask, P, G)
    L = P - 1 + G * (T - P + 1)
    assert ids.shape == (S // G, L) and slot_map.shape == (S // G, L)
    back = shared_prefix_unpack(ids.float(), slot_map, S, T)
    assert torch.equal(back[:, P - 1:], seqs[:, P - 1:].float())
    assert (back[:, :P - 1] == 0).all()
    x = torch.randn(S // G, L, 4)  # trailing dims ride along
    back = shared_prefix_unpack(x, slot_map, S, T)
    assert back.shape == (S, T, 4) and (back[:, :P - 1] == 0).all()
    assert torch.equal(back[G + 1, P + 1], x[1, P - 1 + 1 * (T - P + 1) + 2])
    assert torch.equal(prefix, torch.tensor([[2, P - 1, L], [0, P - 1, L]], dtype=torch.int32))


def test_token_logprobs_shared_matches_plain(setup):
    model, seqs, mask, plain, err_rows = setup
    with torch.no_grad():
        shared = model.token_logprobs(seqs, mask, shared_prefix=(G, P))
    err = (shared - plain)[:, P - 1:].abs().max().item()
    print(f"FIG shared_prefix cpu logprobs: err_shared {err:.3e} err_rows {err_rows:.3e} tol {_tol(err_rows):.3e}")
    assert shared.shape == plain.shape
    assert (shared[:, :P - 1] == 0).all()
    assert err <= _tol(err_rows)
    # masked targets stay exactly 0, as in the plain call
    assert (shared[:, P - 1:][plain[:, P - 1:] == 0] == 0).all()


def test_token_logprobs_shared_variants(setup):
    from distributed_llm_alignment_amd.objectives import keep_row_grid, action_mask

    model, seqs, mask, _, _ = setup
    S, V = seqs.shape[0], model.cfg.vocab_size

    def by_rows(**kw):  # the yardstick of each variant: its own plain call, row by row
        outs = [model.token_logprobs(seqs[i:i + 1], mask[i:i + 1],
                                     **{k: (v[i:i + 1] if k == "keep_rows" else v) for k, v in kw.items()})
                for i in range(S)]
        if isinstance(outs[0], tuple):
            return tuple(torch.cat(x) for x in zip(*outs))
        return torch.cat(outs)

    def shifted(**kw):  # the same rollouts behind k more left-padding columns, k = 1 .. 8
        outs = []
        for k in range(1, 9):
            s2 = torch.cat([seqs.new_full((S, k), 5), seqs], 1)
            m2 = torch.cat([mask.new_zeros((S, k)), mask], 1)
            kw2 = dict(kw)
            if "keep_rows" in kw2:
                kw2["keep_rows"] = torch.cat([kw2["keep_rows"].new_full((S, k), -1), kw2["keep_rows"]], 1)
            o = model.token_logprobs(s2, m2, **kw2)
            outs.append(tuple(x[:, k:] for x in o) if isinstance(o, tuple) else o[:, k:])
        return outs

    def worst(a, outs, pick=None):
        return max((a - (o if pick is None else o[pick]))[:, P - 1:].abs().max().item() for o in outs)

    with torch.no_grad():
        lp0, e0 = model.token_logprobs(seqs, mask, with_entropy=True)
        lp1, e1 = model.token_logprobs(seqs, mask, with_entropy=True, shared_prefix=(G, P))
        t0 = model.token_logprobs(seqs, mask, temperature=0.7)
        t1 = model.token_logprobs(seqs, mask, temperature=0.7, shared_prefix=(G, P))
        g = torch.Generator().manual_seed(1)
        keep = (torch.rand(S, N, V, generator=g) < 0.5)
        keep.scatter_(2, seqs[:, P:].unsqueeze(-1), True)  # the drawn token is always kept
        packed = torch.zeros(S, N, V // 8, dtype=torch.uint8)
        for bit in range(8):
            packed |= keep[..., bit::8].to(torch.uint8) << bit
        kr = keep_row_grid(action_mask(mask, P), P, N)
        k0 = model.token_logprobs(seqs, mask, keep=packed.view(-1, V // 8), keep_rows=kr)
        k1 = model.token_logprobs(seqs, mask, keep=packed.view(-1, V // 8), keep_rows=kr, shared_prefix=(G, P))
        lpr, er = by_rows(with_entropy=True)
        tr = by_rows(temperature=0.7)
        kr_ = by_rows(keep=packed.view(-1, V // 8), keep_rows=kr)
        sh_e = shifted(with_entropy=True)
        shift = {"lp": worst(lp0, sh_e, 0), "entropy": worst(e0, sh_e, 1),
                 "temperature": worst(t0, shifted(temperature=0.7)),
                 "keep": worst(k0, shifted(keep=packed.view(-1, V // 8), keep_rows=kr))}
    for name, a, b, r in (("lp", lp0, lp1, lpr), ("entropy", e0, e1, er), ("temperature", t0, t1, tr),
                          ("keep", k0, k1, kr_)):
        err = (a - b)[:, P - 1:].abs().max().item()
        err_rows = (a - r)[:, P - 1:].abs().max().item()
        tol = _tol(max(err_rows, shift[name])) if name == "entropy" else _tol(err_rows)
        print(f"FIG shared_prefix cpu {name}: err_shared {err:.3e} err_rows {err_rows:.3e} "
              f"err_shift {shift[name]:.3e} tol {tol:.3e}")
        assert err <= tol, name
        assert (b[:, :P - 1] == 0).all(), name
    assert not torch.equal(k0, lp0)  # the keep mask did something


def test_grpo_loss_shared_matches_plain(setup):
    from distributed_llm_alignment_amd import objectives as O

    model, seqs, mask, _, _ = setup
    S = seqs.shape[0]
    scores = torch.linspace(-1, 1, S)
    stats = O.grpo_rollout_stats(model, model, seqs, mask, P, scores, G, beta=0.04, need_old=True)
    stats_s = O.grpo_rollout_stats(model, model, seqs, mask, P, scores, G, beta=0.04, need_old=True,
                                   shared_prefix=(G, P))
    stats["old_logp"] = stats["old_logp"] - 0.05  # rho != 1, kl_ref != 0: every term of the loss is live
    stats["ref_logp"] = stats["ref_logp"] + 0.03
    act = stats["act"]
    assert ((stats_s["ref_logp"] - (stats["ref_logp"] - 0.03)) * act).abs().max() < 1e-5
    params = [p for p in model.parameters() if p.requires_grad]

    def run(**kw):
        model.zero_grad(set_to_none=True)
        loss, m = O.grpo_loss(model, seqs, mask, stats, beta=0.04, **kw)
        loss.backward()
        return loss.detach(), [p.grad.clone() for p in params]

    def run_rows():
        model.zero_grad(set_to_none=True)
        denom = O.grpo_denominator(stats["act"], "sequence")
        tot = 0.0
        for i in range(S):
            mb = {k: (v[i:i + 1] if torch.is_tensor(v) and v.dim() and v.shape[0] == S else v) for k, v in stats.items()}
            loss, _ = O.grpo_loss(model, seqs[i:i + 1], mask[i:i + 1], mb, beta=0.04, denom=denom)
            loss.backward()
            tot = tot + loss.detach()
        return tot, [p.grad.clone() for p in params]

    l0, g0 = run()
    l1, g1 = run(shared_prefix=(G, P))
    lr, gr = run_rows()
    gmax = max(x.abs().max().item() for x in g0)
    err_rows = max(max((a - b).abs().max().item() for a, b in zip(g0, gr)), abs(float(l0 - lr)))
    err = max(max((a - b).abs().max().item() for a, b in zip(g0, g1)), abs(float(l0 - l1)))
    tol = max(4.0 * err_rows, 1e-6)
    print(f"FIG shared_prefix cpu grpo_loss: loss {float(l0):.6f} / {float(l1):.6f} max|grad| {gmax:.3e} "
          f"err_shared {err:.3e} err_rows {err_rows:.3e} tol {tol:.3e}")
    assert gmax > 0
    assert err <= tol


def test_shared_prefix_errors(setup):
    from distributed_llm_alignment_amd import objectives as O
    from distributed_llm_alignment_amd.training.train_rlhf import grpo_update, share_prefix_update

    model, seqs, mask, _, _ = setup
    with pytest.raises(ValueError):
        model.token_logprobs(seqs, mask, shared_prefix=(4, P))  # 6 rows, groups of 4
    with pytest.raises(ValueError):
        model.token_logprobs(seqs, mask, shared_prefix=(G, 1))
    with pytest.raises(ValueError):
        model.token_logprobs(seqs, mask, shared_prefix=(G, T))
    model.vocab_parallel = (0, model.cfg.vocab_size)
    try:
        with pytest.raises(ValueError):
            model.token_logprobs(seqs, mask, shared_prefix=(G, P))
    finally:
        model.vocab_parallel = None
    model.sp = object()
    try:
        with pytest.raises(ValueError):
            model.token_logprobs(seqs, mask, shared_prefix=(G, P))
    finally:
        model.sp = None
    ok = {"share_prefix_update": True, "group_size": 8, "batch_size": 64, "num_minibatches": 2, "update_micro_batch": 8}
    assert share_prefix_update(ok, "grpo") is True
    # the step's 8 prompts are split between the data-parallel replicas before the minibatches are cut
    assert share_prefix_update({**ok, "num_minibatches": 4}, "grpo", None, 2) is True
    for nmb, world in ((8, 2), (2, 3), (4, 4)):
        with pytest.raises(ValueError):
            share_prefix_update({**ok, "num_minibatches": nmb}, "grpo", None, world)
    with pytest.raises(ValueError):  # the stats call's tuple must repeat its own G and prompt_len
        O.grpo_rollout_stats(model, model, seqs, mask, P, torch.zeros(seqs.shape[0]), G, shared_prefix=(G, P + 1))
    assert share_prefix_update({}, "ppo") is False and share_prefix_update({"share_prefix_update": False}, "ppo") is False
    for bad, algo, hw in (({**ok}, "ppo", None), ({**ok}, "reinforce", None),
                          ({**ok, "share_prefix_update": "yes"}, "grpo", None),
                          ({**ok}, "grpo", {"tp_size": 2}), ({**ok}, "grpo", {"sp_size": 2}),
                          ({**ok}, "grpo", {"tp_sequence_parallel": True}),
                          ({**ok, "num_minibatches": 16}, "grpo", None),
                          ({**ok, "update_micro_batch": 4}, "grpo", None),
                          ({**ok, "update_micro_batch": 12}, "grpo", None)):
        with pytest.raises(ValueError):
            share_prefix_update(bad, algo, hw)
    with pytest.raises(ValueError):  # a minibatch that cuts a group
        grpo_update(model, None, seqs[:4], mask[:4], {}, 0.2, None, 0.04, "sequence", N, shared_prefix=(G, P))
    with pytest.raises(ValueError):  # micro-batches that cut groups
        grpo_update(model, None, seqs, mask, {}, 0.2, None, 0.04, "sequence", N, micro=2, shared_prefix=(G, P))
