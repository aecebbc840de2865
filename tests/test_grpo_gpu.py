"""GRPO on the MI355X: the `kv_replicate`, `group_advantages` and `grpo_loss` HIP kernels against
torch / the CPU path of the same ops, graph capture of the loss op (no host sync), the shared
prompt prefill against a full-batch prefill, group rollouts of `generate`, and one GRPO step."""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext
from distributed_llm_alignment_amd.ops.losses import _ref_group_advantages, _ref_grpo_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LOSS_TYPES = ("sequence", "token", "constant")
CLIP_LOW, CLIP_HIGH = 0.2, 0.28
MAX_LEN = 40


def rel_l2(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-12)).item()


# ------------------------------------------------------------------------------ kv_replicate
def _dst(L, B, T, H, D, head_major, sentinel):
    """The destination the way KVCache builds it: storage + the [L, B, T, Hkv, D] view."""
    if head_major:
        store = torch.full((L, B, H, T, D), sentinel, device=DEV, dtype=torch.bfloat16)
        return store, store.transpose(2, 3)
    store = torch.full((L, B, T, H, D), sentinel, device=DEV, dtype=torch.bfloat16)
    return store, store


@pytest.mark.parametrize("D", [64, 80, 128])
@pytest.mark.parametrize("G", [1, 2, 5])
def test_kv_replicate_bitwise_equals_repeat_interleave(G, D):
    _ext.require()
    L, P, H = 2, 3, 2
    g = torch.Generator().manual_seed(G * 1000 + D)
    for Tp in (1, 7, 64, 130):
        T_max = Tp + 5
        for head_major in (True, False):
            _, sk = _dst(L, P, Tp, H, D, head_major, 0.0)
            _, sv = _dst(L, P, Tp, H, D, head_major, 0.0)
            sk.copy_(torch.randn(L, P, Tp, H, D, generator=g))
            sv.copy_(torch.randn(L, P, Tp, H, D, generator=g))
            kstore, dk = _dst(L, P * G, T_max, H, D, head_major, -3.0)
            vstore, dv = _dst(L, P * G, T_max, H, D, head_major, -3.0)
            wk, wv = dk.clone(), dv.clone()  # expected: sentinel everywhere but [0, Tp)
            wk[:, :, :Tp] = sk.repeat_interleave(G, dim=1)
            wv[:, :, :Tp] = sv.repeat_interleave(G, dim=1)
            ops.decode.kv_replicate(sk, sv, dk, dv, G)
            assert torch.equal(dk, wk) and torch.equal(dv, wv), (Tp, head_major)
            assert (dk[:, :, Tp:] == -3.0).all() and (dv[:, :, Tp:] == -3.0).all()  # tail untouched
            assert kstore.data_ptr() == dk.data_ptr()


# -------------------------------------------------------------------------- group_advantages
@pytest.mark.parametrize("G", [2, 8, 64, 96])
@pytest.mark.parametrize("scale_std", [True, False])
def test_group_advantages_kernel_matches_cpu_path(G, scale_std):
    """The summation order differs (wave shuffles vs torch): the mean of G values of size <= R
    moves by at most G * 2^-24 * R, which the 1 / sd scaling (sd ~ 1 here) passes on to the
    advantage: 96 * 6e-8 * 4 = 2.3e-5 absolute in the worst case."""
    P = 4
    g = torch.Generator().manual_seed(G)
    r = torch.randn(P, G, generator=g)
    r[2] = 0.7  # a constant-reward group
    adv, met = ops.group_advantages(r.reshape(-1).to(DEV), G, scale_std=scale_std)
    want, wmet = ops.group_advantages(r.reshape(-1), G, scale_std=scale_std)
    assert adv.is_cuda and torch.isfinite(adv).all()
    assert (adv.view(P, G)[2] == 0).all()
    assert torch.allclose(adv.cpu(), want, atol=2.3e-5, rtol=1e-5)
    assert abs(met["frac_zero_std"].item() - 0.25) < 1e-7
    assert abs(met["reward_std"].item() - wmet["reward_std"].item()) < 1e-5
    ref_adv, _ = _ref_group_advantages(r.reshape(-1).to(DEV), G, scale_std)  # the formula, on the GPU
    assert torch.allclose(adv, ref_adv, atol=2.3e-5, rtol=1e-5)


# --------------------------------------------------------------------------------- grpo_loss
def grpo_inputs(T, seed=0, S=6):
    """The CPU tier's inputs: one fully masked row, advantages of both signs and one zero,
    old = lp + 0.3 * randn."""
    g = torch.Generator().manual_seed(seed)
    lp = -torch.rand(S, T, generator=g) * 3 - 0.05
    old = lp + 0.3 * torch.randn(S, T, generator=g)
    ref = lp + 0.2 * torch.randn(S, T, generator=g)
    mask = (torch.rand(S, T, generator=g) > 0.3).float()
    mask[:, :5] = 0
    mask[3] = 0
    adv = torch.tensor([1.3, -0.8, 0.0, 0.5, -1.7, 0.9])
    return lp, old, ref, adv, mask


@pytest.mark.parametrize("T", [37, 1280])
@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("beta", [0.0, 0.04])
def test_grpo_loss_kernel_matches_cpu_path(T, loss_type, beta):
    lp, old, ref, adv, mask = grpo_inputs(T)
    rho = torch.exp(lp - old)
    m = mask.bool()
    A = adv[:, None].expand_as(lp)
    assert (m & (rho > 1 + CLIP_HIGH) & (A > 0)).any() and (m & (rho < 1 - CLIP_LOW) & (A < 0)).any()
    assert (m & (rho >= 1 - CLIP_LOW) & (rho <= 1 + CLIP_HIGH) & (A != 0)).any()
    kw = dict(clip_low=CLIP_LOW, clip_high=CLIP_HIGH, beta=beta, loss_type=loss_type, max_len=MAX_LEN)
    a = lp.clone().requires_grad_(True)
    want, wmet = ops.grpo_loss(a, old, ref, adv, mask, **kw)
    want.backward()
    dev = [t.to(DEV) for t in (old, ref, adv, mask)]
    b = lp.to(DEV).requires_grad_(True)
    loss, met = ops.grpo_loss(b, *dev, **kw)
    loss.backward()
    print(f"T={T} {loss_type} beta={beta}: loss diff {abs(loss.item() - want.item()):.3e}, "
          f"grad max diff {(b.grad.cpu() - a.grad).abs().max().item():.3e}")
    assert abs(loss.item() - want.item()) < 1e-4
    for k in ("clipfrac", "approx_kl", "kl_ref"):
        assert abs(met[k].item() - wmet[k].item()) < 1e-5, k
    assert met["tokens"].item() == wmet["tokens"].item()
    assert torch.allclose(b.grad.cpu(), a.grad, atol=1e-6, rtol=1e-4)
    assert (b.grad[3] == 0).all()
    # no float atomics: a second call is bitwise equal
    c = lp.to(DEV).requires_grad_(True)
    loss2, _ = ops.grpo_loss(c, *dev, **kw)
    loss2.backward()
    assert torch.equal(loss2, loss) and torch.equal(c.grad, b.grad)


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_grpo_loss_kernel_denom_and_on_policy(loss_type):
    lp, old, ref, adv, mask = [t.to(DEV) for t in grpo_inputs(37, seed=1)]
    kw = dict(clip_low=CLIP_LOW, clip_high=CLIP_HIGH, beta=0.04, loss_type=loss_type, max_len=MAX_LEN)
    a = lp.clone().requires_grad_(True)
    ops.grpo_loss(a, old, ref, adv, mask, **kw)[0].backward()
    S = lp.shape[0]
    denom = {"sequence": torch.full((1,), float(S), device=DEV), "token": mask.sum().clamp(min=1).reshape(1),
             "constant": torch.full((1,), float(S * MAX_LEN), device=DEV)}[loss_type]
    b = lp.clone().requires_grad_(True)
    for s0 in range(0, S, 2):
        sl = slice(s0, s0 + 2)
        ops.grpo_loss(b[sl], old[sl], ref[sl], adv[sl], mask[sl], denom=denom, **kw)[0].backward()
    assert torch.allclose(b.grad, a.grad, atol=1e-7, rtol=1e-5)
    # on-policy, beta = 0: the gradient is -A_s m w_s / divisor
    c = lp.clone().requires_grad_(True)
    ops.grpo_loss(c, None, None, adv, mask, beta=0.0, loss_type=loss_type, max_len=MAX_LEN)[0].backward()
    w = 1.0 / mask.sum(1).clamp(min=1) if loss_type == "sequence" else torch.ones(S, device=DEV)
    div = {"sequence": float(S), "token": float(mask.sum()), "constant": float(S * MAX_LEN)}[loss_type]
    assert torch.allclose(c.grad, -adv[:, None] * mask * w[:, None] / div, atol=0, rtol=1e-6)


def test_grpo_loss_op_has_no_host_sync_graph_capture():
    """The raw op (two launches on one stream: a linear graph) captured in a hipGraph, replayed
    on inputs overwritten in place, equals an eager call on the new inputs bitwise."""
    dla_ops = _ext.require()
    first = [t.to(DEV).contiguous() for t in grpo_inputs(37, seed=2)]
    new = [t.to(DEV).contiguous() for t in grpo_inputs(37, seed=3)]
    denom = torch.full((1,), 5.0, device=DEV)
    args = (CLIP_LOW, CLIP_HIGH, 0.04, 1, float(MAX_LEN))
    dla_ops.grpo_loss(*first, denom, *args)  # warm: nothing lazy left for the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dla_ops.grpo_loss(*first, denom, *args)
    for dst, src in zip(first, new):
        dst.copy_(src)
    denom.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    want = dla_ops.grpo_loss(*new, torch.full((1,), 7.0, device=DEV), *args)
    for got, w in zip(out, want):
        assert torch.equal(got, w)


# ------------------------------------------------------------------------------ rollouts
@pytest.fixture(scope="module")
def rollout_model():
    from distributed_llm_alignment_amd.models import build_model, get_config

    _ext.require()
    cfg = get_config("tiny-llama-d128")
    m = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    g = torch.Generator(device=DEV).manual_seed(3)
    ids = torch.randint(3, cfg.vocab_size, (3, 20), device=DEV, generator=g)
    am = torch.ones_like(ids)
    am[1, :5] = 0  # left padding
    ids[1, :5] = 0
    return m, ids, am


def test_prefill_shared_matches_full_batch_prefill(rollout_model):
    from distributed_llm_alignment_amd.models import KVCache, attention_layout, prefill_shared

    m, ids, am = rollout_model
    (P, Tp), G = ids.shape, 4
    m.eval()
    with torch.no_grad():
        cache, h_last = prefill_shared(m, ids, am, G, Tp + 8)
        full = KVCache(m, P * G, Tp + 8, attention_layout(am)[0].repeat_interleave(G))
        h = m(ids.repeat_interleave(G, 0), cache=full)
    assert cache.len == Tp and torch.equal(cache.kv_start, full.kv_start)
    assert torch.equal(cache.pos, full.pos) and torch.equal(cache.kv_len, full.kv_len)
    starts = cache.kv_start.tolist()
    for name, got, want in (("k", cache.k, full.k), ("v", cache.v, full.v)):
        for row in range(P * G):
            a, b = got[:, row, starts[row]:Tp], want[:, row, starts[row]:Tp]
            assert rel_l2(a, b) < 1e-2, (name, row, rel_l2(a, b))
        grouped = got[:, :, :Tp].reshape(got.shape[0], P, G, Tp, *got.shape[3:])
        assert torch.equal(grouped, grouped[:, :, :1].expand_as(grouped))  # one group: bitwise equal rows
    assert rel_l2(h_last, h[:, -1]) < 1e-2
    assert torch.equal(h_last.view(P, G, -1), h_last.view(P, G, -1)[:, :1].expand(P, G, -1))


def test_generate_group_greedy(rollout_model):
    from distributed_llm_alignment_amd.models import generate

    m, ids, am = rollout_model
    (P, Tp), G, n = ids.shape, 4, 24
    kw = dict(max_new_tokens=n, do_sample=False, eos_token_id=-1, return_mask=True)
    one, _ = generate(m, ids, am, **kw)
    seqs, mask = generate(m, ids, am, num_return_sequences=G, **kw)
    assert seqs.shape == (P * G, Tp + n) and mask.shape == (P * G, Tp + n)
    assert torch.equal(seqs[:, :Tp], ids.repeat_interleave(G, 0))
    assert torch.equal(mask[:, :Tp], am.repeat_interleave(G, 0)) and (mask[:, Tp:] == 1).all()
    grouped = seqs.view(P, G, Tp + n)
    assert torch.equal(grouped, grouped[:, :1].expand_as(grouped))  # the rows of a group are identical
    assert torch.equal(grouped[:, 0, Tp:Tp + 8], one[:, Tp:Tp + 8])  # and equal the G = 1 call's row
    rep, rep_mask = generate(m, ids, am, num_return_sequences=G, share_prefill=False, **kw)
    assert rep.shape == (P * G, Tp + n) and torch.equal(rep_mask, mask)
    assert torch.equal(rep[:, :Tp], seqs[:, :Tp])


def test_generate_group_sampled(rollout_model):
    from distributed_llm_alignment_amd.models import generate

    m, ids, am = rollout_model
    (P, Tp), G, n = ids.shape, 4, 24
    kw = dict(max_new_tokens=n, do_sample=True, temperature=0.8, eos_token_id=-1, seed=11,
              num_return_sequences=G)
    a = generate(m, ids, am, use_graph=True, **kw)
    b = generate(m, ids, am, use_graph=False, **kw)
    assert a.shape == (P * G, Tp + n)
    assert torch.equal(a, b)  # graph replay and the eager loop draw the same tokens
    new = a[:, Tp:].view(P, G, n)
    for p in range(P):  # the G rows of a group sample independently
        assert any(not torch.equal(new[p, 0], new[p, g]) for g in range(1, G)), p
    assert torch.equal(generate(m, ids, am, use_graph=True, **kw), a)  # same seed: same rollouts
    c, cm = generate(m, ids, am, share_prefill=False, return_mask=True, **kw)
    assert c.shape == (P * G, Tp + n) and cm.shape == (P * G, Tp + n)
    assert torch.equal(cm[:, :Tp], am.repeat_interleave(G, 0))


# ------------------------------------------------------------------------------- one step
def _grpo_setup(seed=0):
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.parallel.data_parallel import DataParallelEngine

    cfg = get_config("tiny-llama-d128", num_layers=2)
    pol = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    ref = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0).requires_grad_(False).eval()
    eng = DataParallelEngine(pol, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(seed)
    Tp, R, G, P = 16, 16, 4, 2
    seqs = torch.randint(3, cfg.vocab_size, (P * G, Tp + R), generator=g).to(DEV)
    mask = torch.ones_like(seqs)
    mask[1, Tp + 10:] = 0  # one rollout ended early
    scores = torch.randn(P * G, generator=g).to(DEV)
    return pol, ref, eng, seqs, mask, scores, Tp, G


@pytest.mark.parametrize("loss_type", ["sequence", "token"])
def test_grpo_step_two_layer_model(loss_type):
    from distributed_llm_alignment_amd.objectives import grpo_loss, grpo_rollout_stats

    _ext.require()
    pol, ref, eng, seqs, mask, scores, Tp, G = _grpo_setup()
    stats = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, G, beta=0.0, scale_std=True, need_old=False)
    assert stats["ref_logp"] is None and stats["old_logp"] is None
    assert stats["advantages"].shape == (seqs.shape[0],)
    loss, m = grpo_loss(pol, seqs, mask, stats, CLIP_LOW, CLIP_HIGH, 0.0, loss_type, 16)
    loss.backward()
    got = eng.grad_buf.float().clone()
    # the same objective through plain autograd on the torch formula
    pol2, _, eng2, *_ = _grpo_setup()
    lp = pol2.token_logprobs(seqs, mask)
    want_loss, _ = _ref_grpo_loss(lp, None, None, stats["advantages"], stats["act"], CLIP_LOW, CLIP_HIGH, 0.0,
                                  loss_type, 16)
    want_loss.backward()
    want = eng2.grad_buf.float()
    assert want.abs().sum() > 0 and rel_l2(got, want) < 1e-2, rel_l2(got, want)
    assert abs(loss.item() - want_loss.item()) < 1e-4
    p0 = eng.param_buf.detach().float().clone()
    norm = float(eng.step())
    assert torch.isfinite(loss).item() and 0 < norm < float("inf")
    assert ((eng.param_buf.detach().float() - p0).abs() > 0).any()  # the parameters move


def test_grpo_step_with_reference_and_old_policy():
    """beta > 0 and two updates per rollout batch: reference and old-policy grids are used."""
    from distributed_llm_alignment_amd.objectives import grpo_loss, grpo_rollout_stats

    pol, ref, eng, seqs, mask, scores, Tp, G = _grpo_setup(1)
    stats = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, G, beta=0.04, need_old=True)
    assert stats["ref_logp"].shape == seqs.shape and stats["old_logp"].shape == seqs.shape
    for _ in range(2):
        loss, m = grpo_loss(pol, seqs, mask, stats, CLIP_LOW, CLIP_HIGH, 0.04, "sequence")
        loss.backward()
        norm = float(eng.step())
        assert torch.isfinite(loss).item() and 0 < norm < float("inf")
    assert m["kl_ref"].item() > 0 and m["approx_kl"].item() > 0  # the policy has moved off both
