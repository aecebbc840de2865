"""Plain fp64 reference and input builder for the sequence-level importance ratio of the GRPO loss
(GSPO; test_gspo_cpu.py, test_gspo_gpu.py), in the style of tests/_refs64.py, whose helpers, bound
and constants they share. Nothing here imports the package.

The formulas are written from the docstring of `ops.grpo_loss` and the kernel comments of
csrc/losses.hip (per rollout s, m the action mask, c_s = sum_t m, A = adv[s]):

    d = lp - old;  l_s = sum_{t: m != 0} d / max(c_s, 1);  sr_s = exp(l_s)     (c_s = 0: l_s = 0, sr_s = 1)
    l1 = -A sr_s;  l2 = -A clamp(sr_s, lo, hi);  pg_s = max(l1, l2)
    dr = ref - lp;  k3 = exp(dr) - dr - 1;  per = w pg_s + beta k3               (w = 1 without weights)
    loss: the three normalisations of sum m per (and `denom`) of R.grpo64
    dlp_u = m_u scale_s [g_s (l1 >= l2 ? l1 : 0) - beta (exp(dr_u) - 1)],  g_s = sum_t m w / max(c_s, 1)
    metrics: sum_t m [sr_s outside (lo, hi)] / n,  sum_t m ((sr_s - 1) - l_s) / n,  k3 mean,  n

Entries outside the mask are selected away before any sum. The builder places every row's ratio
and never drops one: every live row's sr_s is at least SEP from lo and hi (asserted), so a clip
decision is the same in fp32 and in fp64.
"""
import torch

import _refs64 as R

F64 = R.F64
# the issue's shapes (around the 256-thread row stride; S > 256 for the finalising loops; both) and
# three more: with S = 3 two of the three rows are fully masked, so one live row (A = 0.8, inside the
# clip range: surrogate and gradient both depend on its row sum) is all they can hold; the row-stride
# shapes are repeated at S = 6 (live rows 0, 1, 2, 4: a clipped and an unclipped row, all three signs of A)
GSPO_SHAPES = [(1, 1), (3, 255), (3, 256), (3, 257), (257, 5), (300, 257), (6, 255), (6, 256), (6, 257)]
JUNK = 50.0  # outside the mask lp = +JUNK, old = -JUNK: d = 100 would wreck a row sum that read it


def _rows(lp, old, m):
    """(l_s, sr_s, c_s) [S, 1] in fp64 from the fp32 inputs."""
    m = R.d(m)
    c = m.sum(1, keepdim=True)
    dd = torch.where(m != 0, R.d(lp) - R.d(old), torch.zeros_like(m))
    ls = dd.sum(1, keepdim=True) / c.clamp(min=1)
    return ls, ls.exp(), c


def gspo_case(S, T, seed=0, clip=R.GRPO_CLIP):
    """lp / old / ref / m [S, T], adv [S]: the advantage placement, the prefix masks and the two
    fully masked rows of R.grpo_case; per-token d ~ N(0, 0.3) shifted row by row so that sr_s is a
    drawn value in [0.5, 1.7] at least 2 SEP from lo and hi; +-JUNK outside the mask of lp / old."""
    g = R.gen(16000 + 3 * S + T + seed)
    lo, hi = 1 - clip[0], 1 + clip[1]
    old = -4.0 * torch.rand(S, T, generator=g)
    dd = 0.3 * torch.randn(S, T, generator=g, dtype=F64)
    noise = 0.3 * torch.randn(S, T, generator=g)
    adv = R._adv_away_from_zero((S,), g)
    lens = torch.randint(1, T + 1, (S,), generator=g)
    m = (torch.arange(T)[None, :] < lens[:, None]).float()
    sr = 0.5 + 1.2 * torch.rand(S, generator=g, dtype=F64)
    if S >= 3:
        adv[0], adv[1], adv[2] = 0.0, 0.8, -0.6  # 0 and both signs
        sr[0], sr[1], sr[2] = 1.05, 1.5, 0.6  # unclipped; above hi with A > 0 and below lo with A < 0: clipped
        dead = (S // 2, S - 1)  # two fully masked rows
        if S == 3:  # the one live row is the A = 0.8 row, inside the range so that its gradient flows
            dead, sr[1] = (0, 2), 1.1
        m[dead[0]] = 0.0
        m[dead[1]] = 0.0
    sr = R._push(R._push(sr, lo, 2 * R.SEP), hi, 2 * R.SEP)
    m64 = R.d(m)
    mean = (dd * m64).sum(1) / m64.sum(1).clamp(min=1)
    dd = dd + (sr.log() - mean)[:, None]
    on = m != 0
    lp = torch.where(on, (old.double() + dd).float(), torch.full((S, T), JUNK))
    old = torch.where(on, old, torch.full((S, T), -JUNK))
    ref = torch.where(on, lp + noise, noise)
    c = {"lp": lp, "old": old, "ref": ref, "adv": adv, "m": m}
    _, got, cnt = _rows(lp, old, m)
    live = cnt.view(-1) > 0
    got = got.view(-1)
    assert ((got[live] - lo).abs() >= R.SEP).all() and ((got[live] - hi).abs() >= R.SEP).all()
    assert (got[~live] == 1).all()
    # the same decisions from an fp32 row mean
    l32 = torch.where(on, lp - old, torch.zeros(S, T)).sum(1) / m.sum(1).clamp(min=1)
    assert torch.equal(l32.exp().double() > hi, got > hi) and torch.equal(l32.exp().double() < lo, got < lo)
    if S >= 3:
        assert (m.sum(1) == 0).sum() >= 2
        assert (adv == 0).any() and (adv > 0).any() and (adv < 0).any()
        out = (sr < lo) | (sr > hi)  # the placed ratios (S = 3: two of these rows are masked, see GSPO_SHAPES)
        assert out.any() and (~out).any()
    if S >= 6:  # ... and among the live rows
        a, out = adv[live], ((got < lo) | (got > hi))[live]
        assert out.any() and (~out).any() and (a > 0).any() and (a < 0).any() and (a == 0).any()
    return c


def gspo64(lp, old, ref, adv, m, beta, mode, max_len=None, denom=None, clip=R.GRPO_CLIP, w=None, autograd=False):
    """fp64 loss, gradient and metrics. `autograd=True`: the gradient by autograd on the fp64
    formula instead of the closed form (they agree to fp64 round-off: at a tie l1 == l2 torch's
    maximum splits the gradient between two branches whose derivatives are equal)."""
    c = R.d(m).sum(1, keepdim=True)
    lp = R.d(lp).requires_grad_(autograd)
    old, ref, m = R.d(old), R.d(ref), R.d(m)
    a = R.d(adv).view(-1, 1)
    lo, hi = 1 - clip[0], 1 + clip[1]
    S = lp.shape[0]
    on = m != 0
    zero = torch.zeros_like(m)
    ls = torch.where(on, lp - old, zero).sum(1, keepdim=True) / c.clamp(min=1)
    sr = ls.exp()
    l1, l2 = -a * sr, -a * sr.clamp(lo, hi)
    dr = torch.where(on, ref - lp, zero)
    k3 = dr.exp() - dr - 1
    ww = torch.ones_like(m) if w is None else torch.where(on, R.d(w), zero)
    per = torch.where(on, ww * torch.maximum(l1, l2) + beta * k3, zero)
    cs = c.view(-1)
    ws = torch.ones_like(cs)
    if mode == "sequence":
        num, div, ws = ((per * m).sum(1) / cs.clamp(min=1)).sum(), float(S), 1.0 / cs.clamp(min=1)
    elif mode == "token":
        num, div = (per * m).sum(), m.sum().clamp(min=1).item()
    else:
        num, div = (per * m).sum(), float(S) * float(max_len)
    if denom is not None:
        div = float(denom)
    loss = num / div
    if autograd:
        (dlp,) = torch.autograd.grad(loss, lp)
    else:
        gs = (m * ww).sum(1, keepdim=True) / c.clamp(min=1)
        pgl = torch.where(l1 >= l2, l1, torch.zeros_like(l1))
        dlp = m * ws[:, None] * (gs * pgl - beta * (dr.exp() - 1)) / div
    n = m.sum()
    inv = 1.0 / n.clamp(min=1)
    sr, ls = sr.detach(), ls.detach()
    out = ((sr < lo) | (sr > hi)).double()
    metrics = torch.stack([(out * m).sum() * inv, (((sr - 1) - ls) * m).sum() * inv, (k3.detach() * m).sum() * inv, n])
    return {"loss": loss.detach(), "dlp": dlp.detach(), "metrics": metrics}


def clipped_tokens64(lp, old, m, clip=R.GRPO_CLIP):
    """The number of action tokens in rows whose sr_s lies outside (lo, hi)."""
    _, sr, c = _rows(lp, old, m)
    return int((c * ((sr < 1 - clip[0]) | (sr > 1 + clip[1])).double()).sum().item())
