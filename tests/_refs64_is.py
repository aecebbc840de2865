"""Plain fp64 references and input builders for the truncated importance weights and the weighted
surrogates (test_rollout_is_cpu.py, test_rollout_is_gpu.py), in the style of tests/_refs64.py,
whose helpers, bound and constants they share. Nothing here imports the package.

The formulas are written from the docstring of `ops.rollout_is_weights` and the kernel comments of
csrc/losses.hip:

    d = trainer_lp - rollout_lp;  token: l = d;  sequence: l_s = sum_t m d / max(c_s, 1)
    r = exp(l);  truncate: w = min(r, C);  mask: w = r if F <= r <= C else 0;  w = 0 off the mask
    metrics over the n action tokens: mean w, #{r > C} / n, #{r < F} / n (mask mode), ESS fraction
    min((sum w)^2 / (n sum w^2), 1) (0 when sum w^2 = 0), n       (n -> max(n, 1) in the divisors)

The builders place values and never drop them: every r (token level) or every row's r_s
(sequence level) is at least 2 SEP from C and from F, so a truncation, a mask decision and both
fractions are the same in fp32 and in fp64; each builder asserts that about its own output.
"""
import math

import torch

import _refs64 as R

F64 = R.F64
IS_SHAPES = [(1, 1), (3, 255), (5, 256), (257, 5), (300, 257)]
IS_LEVELS = ["token", "sequence"]
IS_MODES = ["truncate", "mask"]
IS_CAP = 2.0
IS_FLOOR = 0.5  # 1 / cap, the default of the public wrapper
GAP = 3 * R.SEP  # placed this far from a boundary; asserted >= 2 SEP after the fp32 rounding


def _ratio(trainer_lp, rollout_lp, m, level):
    """r in fp64 from the fp32 inputs: per token, or the row's geometric mean over the mask."""
    m = R.d(m)
    dd = torch.where(m != 0, R.d(trainer_lp) - R.d(rollout_lp), torch.zeros_like(m))
    if level == "sequence":
        dd = (dd.sum(1, keepdim=True) / m.sum(1, keepdim=True).clamp(min=1)).expand_as(m)
    return dd.exp()


def _special_rows(S):
    """(above, below, masked a, masked b). Three rows cannot hold four different special rows: there
    the two fully masked rows carry the values above C and below F (values that must not be read)."""
    if S < 3:
        return None
    if S < 5:
        return S // 2, S - 1, S // 2, S - 1
    return 0, 1, S // 2, S - 1


def is_case(S, T, level, seed=0, cap=IS_CAP, floor=IS_FLOOR):
    """trainer_lp / rollout_lp / m [S, T]: d ~ N(0, 0.3), rows of mixed length; with S >= 3 two
    fully masked rows, a row entirely above C and a row entirely below F."""
    g = R.gen(14000 + 3 * S + T + seed)
    rollout = -4.0 * torch.rand(S, T, generator=g)
    dd = 0.3 * torch.randn(S, T, generator=g, dtype=F64)
    lens = torch.randint(1, T + 1, (S,), generator=g)
    m = (torch.arange(T)[None, :] < lens[:, None]).float()
    rows = _special_rows(S)
    if rows is not None:
        above, below, ma, mb = rows
        dd[above] = math.log(cap) + 0.05 + 0.3 * torch.rand(T, generator=g, dtype=F64)
        dd[below] = math.log(floor) - 0.05 - 0.3 * torch.rand(T, generator=g, dtype=F64)
        m[ma] = 0.0
        m[mb] = 0.0
    if level == "token":  # place every r
        r = R._push(R._push(dd.exp(), cap, GAP), floor, GAP)
        dd = r.log()
    else:  # shift a row whose mean ratio is near a boundary, as a whole
        m64 = R.d(m)
        mean = (dd * m64).sum(1) / m64.sum(1).clamp(min=1)
        r = R._push(R._push(mean.exp(), cap, GAP), floor, GAP)
        dd = dd + (r.log() - mean)[:, None]
    trainer = (rollout.double() + dd).float()
    c = {"trainer_lp": trainer, "rollout_lp": rollout, "m": m}
    r = _ratio(trainer, rollout, m, level)[m != 0]
    assert ((r - cap).abs() >= 2 * R.SEP).all() and ((r - floor).abs() >= 2 * R.SEP).all()
    if rows is not None:
        assert (m.sum(1) == 0).sum() >= 2
        if S >= 5:
            full = _ratio(trainer, rollout, torch.ones_like(m), "token")
            assert (full[rows[0]] > cap).all() and (full[rows[1]] < floor).all()
            assert m[rows[0]].sum() > 0 and m[rows[1]].sum() > 0
    # the same decisions in fp32
    r32 = torch.where(m != 0, trainer - rollout, torch.zeros_like(m))
    if level == "sequence":
        r32 = (r32.sum(1, keepdim=True) / m.sum(1, keepdim=True).clamp(min=1)).expand_as(m)
    r32 = r32.exp()[m != 0]
    assert torch.equal(r32 > cap, r > cap) and torch.equal(r32 < floor, r < floor)
    return c


def is_sat_case():
    """d = +100 / -100 (exact in fp32) on single tokens of row 0, on the whole of rows 1 / 2; row 3
    has d = 0 and a fully masked row 4 carries d = +100. Row 0's mean is exactly 0."""
    S, T = 5, 6
    trainer, rollout = torch.zeros(S, T), torch.zeros(S, T)
    rollout[0, 2], trainer[0, 4] = -100.0, -100.0  # d = +100, d = -100
    rollout[1], trainer[2], rollout[4] = -100.0, -100.0, -100.0
    m = torch.ones(S, T)
    m[4] = 0.0
    return {"trainer_lp": trainer, "rollout_lp": rollout, "m": m}


def check_saturated(got, level, mode):
    """The exact values of is_sat_case: d = +100 gives exactly C (truncate) or 0 (mask), d = 0
    exactly 1, the masked row exactly 0, and nothing is non-finite."""
    w, met = got["w"].cpu(), got["metrics"].cpu()
    assert torch.isfinite(w).all() and torch.isfinite(met).all()
    top = IS_CAP if mode == "truncate" else 0.0
    assert (w[1] == top).all() and (w[3] == 1).all() and (w[4] == 0).all()
    if mode == "mask":
        assert (w[2] == 0).all()
    if level == "token":
        assert w[0, 2].item() == top and (w[0, [0, 1, 3, 5]] == 1).all()
    else:
        assert (w[0] == 1).all()  # the row's mean d is exactly 0
    assert met[4].item() == 24


def is_weights64(trainer_lp, rollout_lp, m, level, mode, cap=IS_CAP, floor=IS_FLOOR):
    r = _ratio(trainer_lp, rollout_lp, m, level)
    m = R.d(m)
    on = m != 0
    high = (r > cap) & on
    low = (r < floor) & on if mode == "mask" else torch.zeros_like(on)
    w = r.clamp(max=cap) if mode == "truncate" else torch.where(high | low, torch.zeros_like(r), r)
    w = torch.where(on, w, torch.zeros_like(w))
    n = m.sum()
    n1 = n.clamp(min=1)
    sw, sw2 = w.sum(), (w * w).sum()
    ess = (sw * sw / (n1 * sw2)).clamp(max=1.0) if sw2 > 0 else torch.zeros((), dtype=F64)
    return {"w": w, "metrics": torch.stack([sw / n1, high.double().sum() / n1, low.double().sum() / n1, ess, n])}


def weight_case(shape, seed=0):
    """Weights in [0, 2] with exact zeros (the masked variant) and exact caps."""
    g = R.gen(15000 + sum(shape) + seed)
    w = 2.0 * torch.rand(shape, generator=g)
    u = torch.rand(shape, generator=g)
    w[u < 0.15] = 0.0
    w[u > 0.85] = 2.0
    return w


def grpo_w64(lp, old, ref, adv, m, w, beta, mode, max_len=None, denom=None, clip=R.GRPO_CLIP):
    """R.grpo64 with per = w max(l1, l2) + beta k3; divisors and metrics are the unweighted ones."""
    lp, old, ref, m, w = R.d(lp), R.d(old), R.d(ref), R.d(m), R.d(w)
    a = R.d(adv).view(-1, 1)
    lo, hi = 1 - clip[0], 1 + clip[1]
    S = lp.shape[0]
    dd = lp - old
    rho = dd.exp()
    l1, l2 = -a * rho, -a * rho.clamp(lo, hi)
    dr = ref - lp
    k3 = dr.exp() - dr - 1
    per = w * torch.maximum(l1, l2) + beta * k3
    c = m.sum(1)
    ws = torch.ones_like(c)
    if mode == "sequence":
        num, div, ws = ((per * m).sum(1) / c.clamp(min=1)).sum(), float(S), 1.0 / c.clamp(min=1)
    elif mode == "token":
        num, div = (per * m).sum(), m.sum().clamp(min=1).item()
    else:
        num, div = (per * m).sum(), float(S) * float(max_len)
    if denom is not None:
        div = float(denom)
    n = m.sum()
    inv = 1.0 / n.clamp(min=1)
    out = ((rho < lo) | (rho > hi)).double()
    dlp = m * ws[:, None] * (w * torch.where(l1 >= l2, l1, torch.zeros_like(l1)) - beta * (dr.exp() - 1)) / div
    metrics = torch.stack([(out * m).sum() * inv, (((rho - 1) - dd) * m).sum() * inv, (k3 * m).sum() * inv, n])
    return {"loss": num / div, "dlp": dlp, "metrics": metrics}


def ppo_policy_w64(lp, old, adv, m, w, eps=R.PPO_EPS):
    """R.ppo_policy64 with the weight on the surrogate; the divisor stays sum m."""
    lp, old, a, m, w = R.d(lp), R.d(old), R.d(adv), R.d(m), R.d(w)
    dd = lp - old
    rho = dd.exp()
    l1, l2 = -a * rho, -a * rho.clamp(1 - eps, 1 + eps)
    cnt = m.sum()
    inv = 1.0 / cnt.clamp(min=1)
    return {"loss": (m * w * torch.maximum(l1, l2)).sum() * inv,
            "dlp": torch.where(l1 >= l2, m * w * l1 * inv, torch.zeros_like(l1)),
            "clipfrac": (m * ((rho - 1).abs() > eps).double()).sum() * inv,
            "approx_kl": (m * ((rho - 1) - dd)).sum() * inv,
            "count": cnt}
