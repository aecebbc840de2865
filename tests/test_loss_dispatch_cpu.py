"""CPU tier: `ops.losses` picks the op of the clipped surrogate and its positional arguments.

The tables below are written out from the if-ladders that `grpo_loss` / `ppo_policy_loss` and their
five autograd Functions held: {is_weight None / given} x {importance level token / sequence} maps
to `grpo_loss` | `grpo_loss_w` | `grpo_loss_seq`, and {is_weight None / given} to `ppo_policy_loss` |
`ppo_policy_loss_w`. The extension is a recorder that returns canned (loss, dlp, metrics), so a real
`backward()` runs through the Functions: the first input takes dlp * gloss, the others nothing.
"""
import pytest
import torch

from distributed_llm_alignment_amd.ops import _ext
from distributed_llm_alignment_amd.ops import losses as L

S, T = 3, 7
DN, LO, HI, BETA, MAXLEN = "denom", 0.2, 0.28, 0.04, 7.0
TAIL = (DN, LO, HI, BETA, 1, MAXLEN)

# (w given, importance level) -> (op, args); plain strings stand in for the tensors
GRPO = {
    (False, "token"): ("grpo_loss", ("lp", "old", "ref", "adv", "m") + TAIL),
    (True, "token"): ("grpo_loss_w", ("lp", "old", "ref", "adv", "m", "w") + TAIL),
    (False, "sequence"): ("grpo_loss_seq", ("lp", "old", "ref", "adv", "m", None) + TAIL),
    (True, "sequence"): ("grpo_loss_seq", ("lp", "old", "ref", "adv", "m", "w") + TAIL),
}
# w given -> (op, args)
PPO = {
    False: ("ppo_policy_loss", ("lp", "old", "adv", "m", 0.2)),
    True: ("ppo_policy_loss_w", ("lp", "old", "adv", "m", "w", 0.2)),
}


@pytest.mark.parametrize("key", list(GRPO), ids=str)
def test_grpo_op_table(key):
    with_w, level = key
    assert L._grpo_op("lp", "old", "ref", "adv", "m", "w" if with_w else None, level, *TAIL) == GRPO[key]


@pytest.mark.parametrize("with_w", list(PPO))
def test_ppo_policy_op_table(with_w):
    assert L._ppo_policy_op("lp", "old", "adv", "m", "w" if with_w else None, 0.2) == PPO[with_w]


class _Recorder:
    """Stands in for `torch.ops.dla`: every op records (name, args) and returns (loss, dlp, metrics)."""

    def __init__(self, n_metrics):
        self.calls = []
        self.dlp = torch.arange(S * T, dtype=torch.float32).reshape(S, T) - 5.0
        self.loss = torch.tensor(1.5)
        self.metrics = torch.arange(n_metrics, dtype=torch.float32)

    def __getattr__(self, name):
        def op(*args):
            self.calls.append((name, args))
            return self.loss.clone(), self.dlp.clone(), self.metrics.clone()
        return op


def _fake_ext(monkeypatch, n_metrics):
    r = _Recorder(n_metrics)
    monkeypatch.setattr(_ext, "require", lambda: r)
    monkeypatch.setattr(_ext, "use_native", lambda *t: True)
    return r


def _grids():
    g = torch.Generator().manual_seed(0)
    t = {k: torch.randn(S, T, generator=g) for k in ("lp", "old", "ref", "adv_grid", "w")}
    t["m"] = (torch.rand(S, T, generator=g) > 0.3).float()
    t["adv"] = torch.randn(S, generator=g)
    # every floating input asks for a gradient: only the first may get one
    return {k: v.requires_grad_() for k, v in t.items()}


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, torch.Tensor):
            assert isinstance(g, torch.Tensor) and g.dtype == torch.float32 and torch.equal(g, w.detach())
            assert not g.requires_grad or w is want[0]  # all but logp arrive detached
        else:
            assert type(g) is type(w) and g == w


def _backward_checks(loss, rec, t, first):
    (loss * 3.0).backward()  # gloss = 3; autograd itself refuses a backward of the wrong arity
    assert torch.equal(t[first].grad, rec.dlp * 3.0)
    assert all(v.grad is None for k, v in t.items() if k != first)


@pytest.mark.parametrize("key", list(GRPO), ids=str)
def test_grpo_loss_dispatch_and_backward(monkeypatch, key):
    with_w, level = key
    rec = _fake_ext(monkeypatch, 4)
    t = _grids()
    denom = torch.tensor([11.0])
    loss, met = L.grpo_loss(t["lp"], t["old"], t["ref"], t["adv"], t["m"], clip_low=LO, clip_high=HI, beta=BETA,
                            loss_type="token", max_len=7, denom=denom, is_weight=t["w"] if with_w else None,
                            importance_level=level)
    name, names = GRPO[key]
    (got_name, got), = rec.calls
    assert got_name == name
    want = tuple(t[n] if n in t else n for n in names[:-6]) + (denom, LO, HI, BETA, 1, MAXLEN)
    _same(got, want)
    assert torch.equal(loss, rec.loss)
    assert {k: float(v) for k, v in met.items()} == {"clipfrac": 0.0, "approx_kl": 1.0, "kl_ref": 2.0, "tokens": 3.0}
    _backward_checks(loss, rec, t, "lp")


@pytest.mark.parametrize("with_w", list(PPO))
def test_ppo_policy_loss_dispatch_and_backward(monkeypatch, with_w):
    rec = _fake_ext(monkeypatch, 3)
    t = _grids()
    loss, met = L.ppo_policy_loss(t["lp"], t["old"], t["adv_grid"], t["m"], 0.2, is_weight=t["w"] if with_w else None)
    name, names = PPO[with_w]
    (got_name, got), = rec.calls
    assert got_name == name
    _same(got, tuple(t["adv_grid" if n == "adv" else n] for n in names[:-1]) + (0.2,))
    assert torch.equal(loss, rec.loss)
    assert {k: float(v) for k, v in met.items()} == {"clipfrac": 0.0, "approx_kl": 1.0}
    _backward_checks(loss, rec, t, "lp")


def test_absent_old_and_ref_alias_logp(monkeypatch):
    """old_logp=None / ref_logp=None (beta 0): both operands are logp, detached, whatever the op."""
    for level in L.GRPO_IMPORTANCE_LEVELS:
        rec = _fake_ext(monkeypatch, 4)
        t = _grids()
        L.grpo_loss(t["lp"], None, None, t["adv"], t["m"], beta=0.0, importance_level=level)
        (_, got), = rec.calls
        assert torch.equal(got[1], t["lp"].detach()) and torch.equal(got[2], t["lp"].detach())
        assert not got[1].requires_grad and not got[2].requires_grad
        assert got[-6] is None  # denom
