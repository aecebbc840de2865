"""Argument contract of the 14 objective torch ops (csrc/bindings_losses.cpp): what they refuse on the
host, before any launch. Every tensor operand of every op must be fp32, on the GPU, contiguous, of the
stated shape and on the first operand's device. The ops allocate their outputs and write nothing in
place, so a refused call has written nothing: asserting the raise is enough. The accepted calls use
one tiny shape (grids S = 3, T = 7; B = 3 pairs; 2 groups of G = 3)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S, T, B, G, P = 3, 7, 3, 3, 2
GRPO_TAIL = (0.2, 0.28, 0.04, 1, 7.0)  # clip_low != clip_high, token mode

# op -> (arguments: a string names a tensor of `_pool`, anything else is passed as it stands; output shapes)
OPS = {
    "seq_reduce": (("lp", "mask"), [(S,), (S,)]),
    "seq_expand_grad": (("coef", "mask", "cnt", True), [(S, T)]),
    "dpo_loss": (("pol", "pol_ref", 0.1, 0.0), [(), (2 * B,), (2 * B,), (4,)]),
    "pairwise_loss": (("sc", "sr"), [(), (B,), (B,), ()]),
    "kl_penalty_pg": (("sc", "sr", "reward", 0.1), [(), (), (B,), (B,)]),
    "gae": (("rewards", "values", "mask", 1.0, 0.95), [(S, T), (S, T)]),
    "ppo_policy_loss": (("lp", "old", "adv_grid", "mask", 0.2), [(), (S, T), (3,)]),
    "ppo_policy_loss_w": (("lp", "old", "adv_grid", "mask", "w", 0.2), [(), (S, T), (3,)]),
    "ppo_value_loss": (("values", "old", "returns", "mask", 0.2), [(), (S, T)]),
    "group_advantages": (("scores", G, True, 1e-4), [(P * G,), (P,)]),
    "grpo_loss": (("lp", "old", "ref", "adv", "mask", "denom") + GRPO_TAIL, [(), (S, T), (4,)]),
    "grpo_loss_w": (("lp", "old", "ref", "adv", "mask", "w", "denom") + GRPO_TAIL, [(), (S, T), (4,)]),
    "grpo_loss_seq": (("lp", "old", "ref", "adv", "mask", "w", "denom") + GRPO_TAIL, [(), (S, T), (4,)]),
    "rollout_is_weights": (("lp", "old", "mask", 2.0, 0.5, 0, 0), [(S, T), (5,)]),
}
ALL = list(OPS)
S0_REFUSED = ["grpo_loss", "grpo_loss_w", "grpo_loss_seq", "rollout_is_weights"]


@pytest.fixture(scope="module")
def C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def _pool(s=S):
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *shape: 0.3 * torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    pool = {k: r(s, T) for k in ("lp", "old", "ref", "adv_grid", "rewards", "values", "returns")}
    pool.update({k: r(s) for k in ("coef", "adv")})
    pool.update({k: r(B) for k in ("sc", "sr", "reward")})
    pool.update(pol=r(2 * B), pol_ref=r(2 * B), scores=r(P * G), denom=torch.full((1,), 11.0, device=DEV))
    pool["mask"] = (torch.rand(s, T, device=DEV, generator=g) > 0.3).float()
    pool["w"] = r(s, T).exp()
    pool["cnt"] = pool["mask"].sum(1)
    return pool


def _call(C, op, pool, replace=None):
    """`replace`: {argument position: value} put in place of the valid argument."""
    args = [pool[a] if isinstance(a, str) else a for a in OPS[op][0]]
    for i, v in (replace or {}).items():
        args[i] = v
    return getattr(C, op)(*args)


def _tensor_positions(op):
    return [i for i, a in enumerate(OPS[op][0]) if isinstance(a, str)]


def _strided(t):
    """A non-contiguous view of t's shape and values; None where none exists (one element)."""
    if t.numel() == 1:
        return None
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=t.device, dtype=t.dtype)
    wide[..., ::2] = t
    v = wide[..., ::2]
    assert v.shape == t.shape and not v.is_contiguous()
    return v


def _spoiled(t):
    """(what, spoiled copy) for one valid operand."""
    out = [("double", t.double()), ("cpu", t.cpu()), ("strided", _strided(t)),
           ("one row or element short", t[:-1].contiguous())]
    if t.dim() == 2:
        out.append(("one column short", t[:, :-1].contiguous()))
    return [(what, v) for what, v in out if v is not None]


@pytest.mark.parametrize("op", ALL)
def test_accepted(C, op):
    """The calls the cases below spoil, unspoiled: fp32 outputs of the documented shapes."""
    pool = _pool()
    out = _call(C, op, pool)
    out = out if isinstance(out, (tuple, list)) else (out,)
    assert [tuple(o.shape) for o in out] == OPS[op][1]
    assert all(o.dtype == torch.float32 and o.device == DEV for o in out)
    assert all(torch.isfinite(o).all() for o in out)


@pytest.mark.parametrize("op", ALL)
def test_spoiled_operand_is_refused(C, op):
    pool = _pool()
    for i in _tensor_positions(op):
        name = OPS[op][0][i]
        for what, bad in _spoiled(pool[name]):
            # seq_expand_grad's mask alone fixes T (coef and cnt are [S]): one column short, it is
            # another valid call, not a spoiled one. One row short, coef and cnt no longer fit it.
            if (op, name, what) == ("seq_expand_grad", "mask", "one column short"):
                continue
            with pytest.raises(RuntimeError):
                _call(C, op, pool, {i: bad})
                pytest.fail(f"{op}: argument {i} ({name}) {what} was accepted")


def test_optional_operands(C):
    """denom and grpo_loss_seq's w may be None; given, they are checked like every operand. A one-element
    tensor has no non-contiguous view, so denom's cases are dtype, device and length."""
    pool = _pool()
    for op in ("grpo_loss", "grpo_loss_w", "grpo_loss_seq"):
        i = OPS[op][0].index("denom")
        out = _call(C, op, pool, {i: None})
        assert [tuple(o.shape) for o in out] == OPS[op][1]
        for bad in (pool["denom"].double(), pool["denom"].cpu(), torch.ones(2, device=DEV), torch.ones(0, device=DEV)):
            with pytest.raises(RuntimeError):
                _call(C, op, pool, {i: bad})
    i = OPS["grpo_loss_seq"][0].index("w")
    out = _call(C, "grpo_loss_seq", pool, {i: None})
    assert [tuple(o.shape) for o in out] == OPS["grpo_loss_seq"][1]


def test_other_device_is_refused(C):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    pool = _pool()
    for op in ALL:
        positions = _tensor_positions(op)
        if len(positions) == 1:  # group_advantages, one operand: nothing to differ from
            continue
        for i in positions:
            with pytest.raises(RuntimeError):
                _call(C, op, pool, {i: pool[OPS[op][0][i]].to("cuda:1")})
                pytest.fail(f"{op}: argument {i} ({OPS[op][0][i]}) on another device was accepted")


def test_empty_inputs(C):
    """S = 0: seq_reduce and gae return empty tensors; the GRPO ops and rollout_is_weights refuse, and
    kl_penalty_pg refuses n = 0."""
    pool = _pool(0)
    total, cnt = _call(C, "seq_reduce", pool)
    assert total.shape == (0,) and cnt.shape == (0,)
    adv, ret = _call(C, "gae", pool)
    assert adv.shape == (0, T) and ret.shape == (0, T)
    for op in S0_REFUSED:
        with pytest.raises(RuntimeError):
            _call(C, op, pool)
    empty = torch.empty(0, device=DEV)
    with pytest.raises(RuntimeError):
        C.kl_penalty_pg(empty, empty, empty, 0.1)
