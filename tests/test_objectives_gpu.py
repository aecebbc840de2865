"""GPU tier: every kernel of csrc/losses.hip against the plain fp64 references of tests/_refs64.py.

All checks are elementwise (max abs error) on every output, metrics and non-differentiable
outputs included; each kernel is launched twice and the two results must be bitwise equal (the
file promises no atomics). Shapes sit on the loop strides, grid caps and lane splits of the
kernels: 255 / 256 / 257 around the 256-thread stride, 1023 / 1024 / 1025 around the 1024-thread
PPO blocks, 64 k +- 1 around gae's lane split, S > 256 in grpo_grad's partial sums, and one grid
past seq_expand_grad's 2048-block cap.

Bound (see _refs64): 8 * E32 + 4 ulp32(max |ref|) (+ a derived term where one is stated), E32
being the error of the package's fp32 CPU branch against fp64 on the same inputs.
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext

import _branch32 as B32
import _refs64 as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def twice(fn):
    """Launch twice; the outputs must be bitwise equal. Returns the first result."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two launches differ bitwise"
    return a


def compare(kernel, got, ref, cpu):
    assert set(got) == set(ref)
    for k in ref:
        R.check(kernel, k, got[k], ref[k], R.e32_of(cpu[k], ref[k]))


# --------------------------------------------------------------- seq_reduce / seq_expand_grad
@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("S,T", R.SEQ_SHAPES + [R.SEQ_BIG])
def test_seq_reduce(S, T, mean):
    k = _ext.require()
    c = R.seq_case(S, T)
    g = dev(c)
    x = g["lp"].clone().requires_grad_(True)
    out = ops.seq_reduce(x, g["mask"], mean=mean)
    (grad,) = torch.autograd.grad(out, x, g["coef"])
    s, cnt = twice(lambda: k.seq_reduce(g["lp"], g["mask"]))
    twice(lambda: (k.seq_expand_grad(g["coef"], g["mask"], cnt, mean),))
    assert torch.equal(cnt.cpu(), c["mask"].sum(1))  # counts of 0/1 below 2^24 are exact
    assert torch.equal(out.detach(), s / cnt.clamp(min=1) if mean else s)
    compare("seq_reduce", {"out": out, "grad": grad}, R.seq_reduce64(**c, mean=mean),
            B32.seq_reduce(**c, mean=mean))
    if S >= 3:  # the all-zero mask row
        assert out[1].item() == 0 and (grad[1] == 0).all()


# ---------------------------------------------------------------------------------- dpo_loss
def _dpo_gpu(c, beta, ls):
    k = _ext.require()
    g = dev(c)
    loss, dpol, rewards, metrics = twice(lambda: k.dpo_loss(g["pol"], g["ref"], beta, ls))
    return {"loss": loss, "dpol": dpol, "rewards": rewards, "metrics": metrics}


@pytest.mark.parametrize("ls", R.DPO_LS)
@pytest.mark.parametrize("beta", R.DPO_BETAS)
@pytest.mark.parametrize("B", R.PAIR_B)
def test_dpo_loss(B, beta, ls):
    c = R.dpo_case(B)
    got = _dpo_gpu(c, beta, ls)
    ref = R.dpo64(**c, beta=beta, ls=ls)
    compare("dpo_loss", got, ref, B32.dpo(**c, beta=beta, ls=ls))
    # through the public op: the metrics dict and autograd carry the same tensors
    pol = dev(c)["pol"].clone().requires_grad_(True)
    loss, met = ops.dpo_loss(pol[:B], pol[B:], dev(c)["ref"][:B], dev(c)["ref"][B:], beta=beta, label_smoothing=ls)
    (gp,) = torch.autograd.grad(loss, pol)
    assert torch.equal(loss.detach(), got["loss"]) and torch.equal(gp, got["dpol"])
    assert torch.equal(met["rewards_per_seq"], got["rewards"])
    for i, name in enumerate(["rewards/chosen", "rewards/rejected", "rewards/accuracy", "rewards/margin"]):
        assert torch.equal(met[name], got["metrics"][i])


def _sat_check(kernel, got, ref):
    """Saturated margins: finite, and relative 1e-5 of each fp64 value (2^-126, the smallest
    normal fp32, absolute: below it fp32 holds nothing)."""
    for name in ref:
        a, b = R.d(got[name].cpu()).reshape(-1), R.d(ref[name]).reshape(-1)
        assert torch.isfinite(a).all(), f"{kernel}/{name}: not finite"
        rel = ((a - b).abs() / b.abs().clamp(min=2.0 ** -126)).max().item()
        print(f"FIG {kernel}_sat {name}: max rel err {rel:.3e} bound 1e-5")
        assert ((a - b).abs() <= 1e-5 * b.abs() + 2.0 ** -126).all(), f"{kernel}/{name}: rel {rel:.3e}"


@pytest.mark.parametrize("ls", R.DPO_LS)
@pytest.mark.parametrize("beta", R.DPO_BETAS)
def test_dpo_loss_saturated(beta, ls):
    for zs in [R.SAT_Z] + [[z] for z in R.SAT_Z]:  # all six margins, then each alone (B = 1)
        c = R.dpo_sat_case(beta, zs)
        got = _dpo_gpu(c, beta, ls)
        ref = R.dpo64(**c, beta=beta, ls=ls)
        _sat_check("dpo_loss", got, ref)
        if len(zs) == 1 and ls == 0:  # the loss is |z| or 0, the gradient 0 or -+ beta / B
            z = zs[0]
            assert got["loss"].item() == pytest.approx(max(-z, 0.0), rel=1e-5, abs=1e-12)
            assert got["dpol"][0].item() == pytest.approx(-beta if z < 0 else 0.0, rel=1e-5, abs=1e-12)


# ----------------------------------------------------------------------------- pairwise_loss
def _pairwise_gpu(c):
    k = _ext.require()
    g = dev(c)
    loss, dsc, dsr, acc = twice(lambda: k.pairwise_loss(g["sc"], g["sr"]))
    return {"loss": loss, "dsc": dsc, "dsr": dsr, "acc": acc}


@pytest.mark.parametrize("B", R.PAIR_B)
def test_pairwise_loss(B):
    c = R.pairwise_case(B)
    compare("pairwise_loss", _pairwise_gpu(c), R.pairwise64(**c), B32.pairwise(**c))


def test_pairwise_loss_saturated():
    for zs in [R.SAT_Z] + [[z] for z in R.SAT_Z]:
        c = R.pairwise_sat_case(zs)
        got = _pairwise_gpu(c)
        _sat_check("pairwise_loss", got, R.pairwise64(**c))
        if len(zs) == 1:
            z = zs[0]
            assert got["loss"].item() == pytest.approx(max(-z, 0.0), rel=1e-5, abs=1e-12)
            assert got["dsc"][0].item() == pytest.approx(-1.0 if z < 0 else 0.0, rel=1e-5, abs=1e-12)


# ----------------------------------------------------------------------------- kl_penalty_pg
@pytest.mark.parametrize("n", R.KLPG_N)
def test_kl_penalty_pg(n):
    k = _ext.require()
    c = R.klpg_case(n)
    g = dev(c)
    loss, klm, dlp, adv = twice(lambda: k.kl_penalty_pg(g["lp"], g["lr"], g["reward"], R.KL_COEF))
    compare("kl_penalty_pg", {"loss": loss, "kl_mean": klm, "adv": adv, "dlp": dlp}, R.klpg64(**c), B32.klpg(**c))


# --------------------------------------------------------------------------------------- gae
@pytest.mark.parametrize("T,mask,gl", R.GAE_CASES)
def test_gae(T, mask, gl):
    k = _ext.require()
    c = R.gae_case(T, mask)
    g = dev(c)
    adv, ret = twice(lambda: k.gae(g["r"], g["v"], g["m"], gl[0], gl[1]))
    compare("gae", {"adv": adv, "ret": ret}, R.gae64(**c, gamma=gl[0], lam=gl[1]),
            B32.gae(**c, gamma=gl[0], lam=gl[1]))


# ---------------------------------------------------------- ppo_policy_loss / ppo_value_loss
@pytest.mark.parametrize("n,masked", [(n, False) for n in R.PPO_N] + [(1025, True)])
def test_ppo_policy_loss(n, masked):
    k = _ext.require()
    c = R.ppo_policy_case(n, masked)
    g = dev(c)
    loss, dlp, met = twice(lambda: k.ppo_policy_loss(g["lp"], g["old"], g["adv"], g["m"], R.PPO_EPS))
    got = {"loss": loss, "dlp": dlp, "clipfrac": met[0], "approx_kl": met[1], "count": met[2]}
    ref = R.ppo_policy64(**c)
    compare("ppo_policy_loss", got, ref, B32.ppo_policy(**c))
    assert met[2].item() == c["m"].sum().item()
    if masked:  # loss 0, gradient 0, count 0
        assert loss.item() == 0 and (dlp == 0).all() and (met == 0).all()


@pytest.mark.parametrize("n,masked", [(n, False) for n in R.PPO_N] + [(1025, True)])
def test_ppo_value_loss(n, masked):
    k = _ext.require()
    c = R.ppo_value_case(n, masked)
    g = dev(c)
    loss, dval = twice(lambda: k.ppo_value_loss(g["val"], g["old"], g["ret"], g["m"], R.PPO_VCLIP))
    compare("ppo_value_loss", {"loss": loss, "dval": dval}, R.ppo_value64(**c), B32.ppo_value(**c))
    if masked:
        assert loss.item() == 0 and (dval == 0).all()


# -------------------------------------------------------------------------- group_advantages
@pytest.mark.parametrize("scale_std", [True, False])
@pytest.mark.parametrize("G", R.GROUP_G)
def test_group_advantages(G, scale_std):
    k = _ext.require()
    c = R.group_case(G)
    s = c["scores"].to(DEV)
    adv, sd = twice(lambda: k.group_advantages(s, G, scale_std, R.GROUP_EPS))
    compare("group_advantages", {"adv": adv, "sd": sd}, R.group_advantages64(**c, scale_std=scale_std),
            B32.group_advantages(**c, scale_std=scale_std))
    assert (adv.view(-1, G)[2] == 0).all() and sd[2].item() == 0  # the constant group
    if G == 1:
        assert (adv == 0).all() and (sd == 0).all()


# --------------------------------------------------------------------------------- grpo_loss
def _grpo_gpu(c, beta, mode, max_len, denom=None):
    k = _ext.require()
    g = dev(c)
    dn = None if denom is None else torch.tensor([denom], dtype=torch.float32, device=DEV)
    loss, dlp, met = twice(lambda: k.grpo_loss(g["lp"], g["old"], g["ref"], g["adv"], g["m"], dn, R.GRPO_CLIP[0],
                                               R.GRPO_CLIP[1], beta, R.GRPO_MODES.index(mode), float(max_len)))
    return {"loss": loss, "dlp": dlp, "metrics": met}


@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
@pytest.mark.parametrize("S,T", R.GRPO_SHAPES)
def test_grpo_loss(S, T, mode, beta):
    c = R.grpo_case(S, T)
    kw = dict(beta=beta, mode=mode, max_len=T)
    got = _grpo_gpu(c, **kw)
    compare("grpo_loss", got, R.grpo64(**c, **kw), B32.grpo(**c, **kw))
    assert got["metrics"][3].item() == c["m"].sum().item()
    if S >= 3:  # fully masked rows take no gradient
        assert (got["dlp"][S // 2] == 0).all() and (got["dlp"][S - 1] == 0).all()


def test_grpo_loss_denom():
    c = R.grpo_case(257, 5)
    kw = dict(beta=0.04, mode="token", max_len=5, denom=R.GRPO_DENOM)
    compare("grpo_loss", _grpo_gpu(c, **kw), R.grpo64(**c, **kw), B32.grpo(**c, **kw))
