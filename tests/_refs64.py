"""Plain fp64 references, input builders and the error bound for the objective, optimizer and
LM-head row kernel tests (test_refs64_cpu.py, test_objectives_gpu.py, test_optimizer_gpu.py,
test_logprob_rows_gpu.py).

The formulas are written from the docstrings of ops/losses.py, ops/logprob.py, optim/adamw.py and
the comments of csrc/losses.hip, csrc/adamw.hip, csrc/logprob.hip; nothing here imports the
package's ops and nothing needs a GPU. Every reference takes the fp32 (or bf16) CPU tensors that
the kernels see, widens them to fp64 and returns a dict of fp64 tensors, one entry per output.

Gradients: autograd on the fp64 formula where the objective is smooth; where the kernel defines a
branch convention (`l1 >= l2` in the clipped surrogates, the three-way choice in the value loss)
the closed form of the kernel comment. The builders keep every clipped quantity at least `SEP`
away from its boundary, so a branch, a clip fraction or an accuracy is decided identically in
fp32 and in fp64; each builder asserts that about its own output (values are placed, never
dropped or filtered).

Scalars that a kernel takes as fp32 arguments (beta, gamma, lam, lr, the AdamW betas ...) are used
here as the stated constants. The AdamW hyper-parameters of `ADAMW_HP` are chosen exactly
representable in fp32: the kernel forms `1 - b1` and `1 - b2` in fp32, so with b2 = 0.999 (not
representable) it would run a slightly different, equally valid AdamW (b2 = fp32(0.999)) whose
second moment differs by 1.3e-5 relative from the fp64 one with b2 = 0.999.

Bound (fp32 outputs):   |out - ref64| <= MARGIN * E32 + FLOOR_ULPS ulp32(max |ref64|) + extra
  E32   = max |fp32 CPU branch - ref64| on the same inputs,
  extra = a term derived next to its use from the two things the CPU branch does not have
          (__expf / __logf, a different summation order); 0 unless stated.
bf16 outputs add one bf16 ulp of the reference element.
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
SEP = 1e-3  # minimum distance of a clipped quantity from its boundary
MARGIN = 8.0
FLOOR_ULPS = 4.0
EPS32 = 2.0 ** -23
NINF = float("-inf")


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def d(x):
    return x.detach().to(F64)


def bf16_ulp(x):
    """One bf16 ulp (8 significand bits) of each element of x (fp64); 2^-133 at 0."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 7)


def check(kernel, name, got, ref, e32, extra=0.0, bf16=False):
    """Elementwise check of one output against fp64; prints the figure before it asserts."""
    got, ref = d(got.cpu()).reshape(-1), d(ref).reshape(-1)
    assert got.shape == ref.shape, f"{kernel}/{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin], ref[~fin]), f"{kernel}/{name}: non-finite reference entries differ"
    assert torch.isfinite(got[fin]).all(), f"{kernel}/{name}: non-finite output"
    scale = ref[fin].abs().max().item() if fin.any() else 0.0
    bound = MARGIN * float(e32) + FLOOR_ULPS * EPS32 * scale + float(extra)
    diff = (got[fin] - ref[fin]).abs()
    if bf16:
        diff = (diff - bf16_ulp(ref[fin])).clamp(min=0.0)
    err = diff.max().item() if fin.any() else 0.0
    print(f"FIG {kernel} {name}: err {err:.3e} bound {bound:.3e} (E32 {float(e32):.3e}, extra {float(extra):.3e})")
    assert err <= bound, f"{kernel}/{name}: max abs err {err:.3e} > bound {bound:.3e}"
    return err, bound


def e32_of(cpu, ref):
    """Max abs error of a fp32 CPU-branch output against fp64 (finite entries)."""
    a, b = d(cpu).reshape(-1), d(ref).reshape(-1)
    fin = torch.isfinite(b)
    return (a[fin] - b[fin]).abs().max().item() if fin.any() else 0.0


def _push(x, center, gap):
    """Move the entries of x that lie within `gap` of `center` out to center +- gap."""
    near = (x - center).abs() < gap
    side = torch.where(x >= center, torch.ones_like(x), -torch.ones_like(x))
    return torch.where(near, center + side * gap, x)


# ============================================================ seq_reduce / seq_expand_grad
SEQ_SHAPES = [(1, 1), (3, 255), (3, 256), (3, 257), (5, 1000)]
SEQ_BIG = (9, 65536)  # 589824 elements = 2304 blocks of 256: crosses seq_expand_grad's 2048-block cap


def seq_case(S, T, seed=0):
    g = gen(1000 + 7 * S + T + seed)
    lp = -6.0 * torch.rand(S, T, generator=g)
    mask = (torch.rand(S, T, generator=g) < 0.7).float()
    if S >= 3:
        mask[1] = 0.0  # max(cnt, 1)
    coef = torch.randn(S, generator=g)
    return {"lp": lp, "mask": mask, "coef": coef}


def seq_reduce64(lp, mask, coef, mean):
    lp, mask, coef = d(lp), d(mask), d(coef)
    cnt = mask.sum(1)
    s = (lp * mask).sum(1)
    div = cnt.clamp(min=1) if mean else torch.ones_like(cnt)
    return {"out": s / div, "grad": coef[:, None] * mask / div[:, None]}


# ============================================================================== dpo_loss
PAIR_B = [1, 4, 255, 256, 257, 600]
DPO_BETAS = [0.1, 0.5]
DPO_LS = [0.0, 0.1]
SAT_Z = [30.0, -30.0, 100.0, -100.0, 1e4, -1e4]


def dpo_case(B, seed=0):
    """pol / ref [2B] (chosen then rejected). |z| <= 8 and |c_r - r_r| >= SEP for every beta of
    DPO_BETAS (asserted)."""
    g = gen(2000 + B + seed)
    ref = -2.0 - 4.0 * torch.rand(2 * B, generator=g)
    dc = 8.0 * torch.rand(B, generator=g) - 4.0
    dr = 8.0 * torch.rand(B, generator=g) - 4.0
    dc = dr + _push(dc - dr, 0.0, 0.05)
    pol = ref + torch.cat([dc, dr])
    for beta in DPO_BETAS:
        z = beta * ((d(pol[:B]) - d(ref[:B])) - (d(pol[B:]) - d(ref[B:])))
        assert z.abs().min() >= SEP and z.abs().max() <= 8.0
    return {"pol": pol, "ref": ref}


def dpo_sat_case(beta, zs=SAT_Z):
    """Margins z = beta * (pol_c - 0) at the saturated values, ref = 0, rejected = 0."""
    zc = torch.tensor(zs, dtype=torch.float32) / beta
    B = zc.numel()
    return {"pol": torch.cat([zc, torch.zeros(B)]), "ref": torch.zeros(2 * B)}


def dpo64(pol, ref, beta, ls):
    pol = d(pol).requires_grad_(True)
    ref = d(ref)
    B = pol.numel() // 2
    cr = beta * (pol[:B] - ref[:B])
    rr = beta * (pol[B:] - ref[B:])
    z = cr - rr
    loss = (-(1 - ls) * F.logsigmoid(z) - ls * F.logsigmoid(-z)).mean()
    (dpol,) = torch.autograd.grad(loss, pol)
    cr, rr, z = cr.detach(), rr.detach(), z.detach()
    metrics = torch.stack([cr.mean(), rr.mean(), (cr > rr).double().mean(), z.mean()])
    return {"loss": loss.detach(), "dpol": dpol, "rewards": torch.cat([cr, rr]), "metrics": metrics}


# ========================================================================= pairwise_loss
def pairwise_case(B, seed=0):
    g = gen(3000 + B + seed)
    sc = 3.0 * torch.randn(B, generator=g)
    z = _push(14.0 * torch.rand(B, generator=g) - 7.0, 0.0, 0.01)
    sr = sc - z
    z64 = d(sc) - d(sr)
    assert z64.abs().min() >= SEP and z64.abs().max() <= 8.0
    return {"sc": sc, "sr": sr}


def pairwise_sat_case(zs=SAT_Z):
    sc = torch.tensor(zs, dtype=torch.float32)
    return {"sc": sc, "sr": torch.zeros_like(sc)}


def pairwise64(sc, sr):
    sc = d(sc).requires_grad_(True)
    sr = d(sr).requires_grad_(True)
    loss = -F.logsigmoid(sc - sr).mean()
    dsc, dsr = torch.autograd.grad(loss, (sc, sr))
    return {"loss": loss.detach(), "dsc": dsc, "dsr": dsr, "acc": (sc > sr).double().mean().detach()}


# ========================================================================= kl_penalty_pg
KLPG_N = [1, 255, 256, 257, 600]
KL_COEF = 0.1


def klpg_case(n, seed=0):
    g = gen(4000 + n + seed)
    lp = -4.0 * torch.rand(n, generator=g)
    return {"lp": lp, "lr": lp + 0.5 * torch.randn(n, generator=g), "reward": torch.randn(n, generator=g)}


def klpg64(lp, lr, reward, kl_coef=KL_COEF):
    lp, lr, r = d(lp), d(lr), d(reward)
    n = lp.numel()
    kl = lp - lr
    shaped = r - kl_coef * kl
    adv = shaped - shaped.mean()
    return {"loss": -(adv * lp).mean(), "kl_mean": kl.mean(), "adv": adv, "dlp": -adv / n}


# =================================================================================== gae
GAE_T = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097]
GAE_MASKS = ["ones", "zeros", "holes", "right", "left"]
GAE_GL = [(1.0, 0.95), (0.99, 0.95), (1.0, 1.0), (0.9, 0.0)]
GAE_CASES = ([(T, "holes", (0.99, 0.95)) for T in GAE_T]
             + [(T, mk, gl) for T in (65, 129) for mk in GAE_MASKS for gl in GAE_GL
                if not (mk == "holes" and gl == (0.99, 0.95))])


def gae_case(T, mask_kind, S=3, seed=0):
    g = gen(5000 + T + seed)
    r = 0.5 * torch.randn(S, T, generator=g)
    v = torch.randn(S, T, generator=g)
    t = torch.arange(T)[None, :].expand(S, T)
    lens = torch.tensor([max(1, (T * k) // (S + 1)) for k in range(1, S + 1)])[:, None]
    if mask_kind == "ones":
        m = torch.ones(S, T)
    elif mask_kind == "zeros":
        m = torch.zeros(S, T)
    elif mask_kind == "holes":
        m = (torch.rand(S, T, generator=g) < 0.8).float()
    elif mask_kind == "right":
        m = (t < lens).float()
    else:
        m = (t >= T - lens).float()
    return {"r": r, "v": v, "m": m}


def gae64(r, v, m, gamma, lam):
    """The serial reverse recurrence of the `gae` docstring."""
    r, v, m = d(r), d(v), d(m)
    S, T = r.shape
    adv = torch.zeros_like(r)
    nxt = torch.zeros(S, dtype=F64)
    for t in range(T - 1, -1, -1):
        mn = m[:, t + 1] if t + 1 < T else torch.zeros(S, dtype=F64)
        vn = v[:, t + 1] if t + 1 < T else torch.zeros(S, dtype=F64)
        delta = r[:, t] + gamma * mn * vn - v[:, t]
        nxt = m[:, t] * (delta + gamma * lam * mn * nxt)
        adv[:, t] = nxt
    return {"adv": adv, "ret": adv + v}


# =========================================================== ppo_policy_loss / ppo_value_loss
PPO_N = [1, 1023, 1024, 1025, 5000]
PPO_EPS = 0.2
PPO_VCLIP = 0.2


def _ratio_logp(old, g, lo, hi):
    """lp with rho = exp(lp - old) in [0.5, 1.7], at least 2 SEP away from lo and hi."""
    rho = 0.5 + 1.2 * torch.rand(old.shape, generator=g, dtype=F64)
    rho = _push(_push(rho, lo, 2 * SEP), hi, 2 * SEP)
    return (old.double() + rho.log()).float()


def _adv_away_from_zero(shape, g):
    a = torch.randn(shape, generator=g)
    return _push(a, 0.0, 0.05)


def ppo_policy_case(n, masked=False, seed=0):
    g = gen(6000 + n + seed)
    old = -4.0 * torch.rand(n, generator=g)
    lp = _ratio_logp(old, g, 1 - PPO_EPS, 1 + PPO_EPS)
    adv = _adv_away_from_zero((n,), g)
    m = torch.zeros(n) if masked else (torch.rand(n, generator=g) < 0.7).float()
    rho = (d(lp) - d(old)).exp()
    assert ((rho - (1 - PPO_EPS)).abs() >= SEP).all() and ((rho - (1 + PPO_EPS)).abs() >= SEP).all()
    l1, l2 = -d(adv) * rho, -d(adv) * rho.clamp(1 - PPO_EPS, 1 + PPO_EPS)
    clipped = (rho - 1).abs() > PPO_EPS
    assert ((l1 - l2).abs()[clipped] >= 0.05 * SEP).all()  # |a| >= 0.05 times |rho - bound| >= SEP
    assert (l1 == l2)[~clipped].all()
    return {"lp": lp, "old": old, "adv": adv, "m": m}


def ppo_policy64(lp, old, adv, m, eps=PPO_EPS):
    lp, old, a, m = d(lp), d(old), d(adv), d(m)
    dd = lp - old
    rho = dd.exp()
    l1, l2 = -a * rho, -a * rho.clamp(1 - eps, 1 + eps)
    cnt = m.sum()
    inv = 1.0 / cnt.clamp(min=1)
    return {"loss": (m * torch.maximum(l1, l2)).sum() * inv,
            "dlp": torch.where(l1 >= l2, m * l1 * inv, torch.zeros_like(l1)),
            "clipfrac": (m * ((rho - 1).abs() > eps).double()).sum() * inv,
            "approx_kl": (m * ((rho - 1) - dd)).sum() * inv,
            "count": cnt}


def ppo_value_case(n, masked=False, seed=0):
    """|V - V_old| at least 2 SEP from the clip; where the clip acts, |u1 - u2| >= SEP (asserted).
    Inside the clip V_clip = V, u1 = u2 by definition and both branches give the same gradient."""
    g = gen(7000 + n + seed)
    old = torch.randn(n, generator=g)
    dv = _push(_push(1.2 * torch.rand(n, generator=g) - 0.6, PPO_VCLIP, 2 * SEP), -PPO_VCLIP, 2 * SEP)
    val = old + dv
    vc = old + (val - old).clamp(-PPO_VCLIP, PPO_VCLIP)
    mid = 0.5 * (val + vc)
    ret = mid + _push(torch.randn(n, generator=g), 0.0, 0.3)
    m = torch.zeros(n) if masked else (torch.rand(n, generator=g) < 0.7).float()
    v64, o64, r64 = d(val), d(old), d(ret)
    dv64 = v64 - o64
    assert ((dv64.abs() - PPO_VCLIP).abs() >= SEP).all()
    vc64 = o64 + dv64.clamp(-PPO_VCLIP, PPO_VCLIP)
    u1, u2 = (v64 - r64) ** 2, (vc64 - r64) ** 2
    assert ((u1 - u2).abs()[dv64.abs() > PPO_VCLIP] >= SEP).all()
    return {"val": val, "old": old, "ret": ret, "m": m}


def ppo_value64(val, old, ret, m, clip=PPO_VCLIP):
    v, o, R, m = d(val), d(old), d(ret), d(m)
    dv = v - o
    vc = o + dv.clamp(-clip, clip)
    u1, u2 = (v - R) ** 2, (vc - R) ** 2
    inv = 1.0 / m.sum().clamp(min=1)
    g = torch.where(u1 >= u2, v - R, torch.where(dv.abs() <= clip, vc - R, torch.zeros_like(v)))
    return {"loss": 0.5 * (m * torch.maximum(u1, u2)).sum() * inv, "dval": m * g * inv}


# ====================================================================== group_advantages
GROUP_G = [1, 63, 65, 200]
GROUP_EPS = 1e-4


def group_case(G, P=5, seed=0):
    g = gen(8000 + G + seed)
    r = torch.randn(P, G, generator=g)
    r[2] = 0.75  # a constant group: exactly 0, sd 0
    return {"scores": r.reshape(-1), "G": G}


def group_advantages64(scores, G, scale_std, eps=GROUP_EPS):
    r = d(scores).reshape(-1, G)
    mu = r.mean(1, keepdim=True)
    sd = ((r - mu) ** 2).mean(1, keepdim=True).sqrt()
    const = r.max(1, keepdim=True).values == r.min(1, keepdim=True).values
    sd = torch.where(const, torch.zeros_like(sd), sd)
    adv = (r - mu) / (sd + eps) if scale_std else r - mu
    adv = torch.where(const, torch.zeros_like(adv), adv)
    return {"adv": adv.reshape(-1), "sd": sd.reshape(-1)}


# ============================================================================= grpo_loss
GRPO_SHAPES = [(1, 1), (257, 5), (300, 257)]
GRPO_MODES = ["sequence", "token", "constant"]
GRPO_BETAS = [0.0, 0.04]
GRPO_CLIP = (0.2, 0.28)
GRPO_DENOM = 123.0


def grpo_case(S, T, seed=0):
    g = gen(9000 + 3 * S + T + seed)
    lo, hi = 1 - GRPO_CLIP[0], 1 + GRPO_CLIP[1]
    old = -4.0 * torch.rand(S, T, generator=g)
    lp = _ratio_logp(old, g, lo, hi)
    ref = lp + 0.3 * torch.randn(S, T, generator=g)
    adv = _adv_away_from_zero((S,), g)
    lens = torch.randint(1, T + 1, (S,), generator=g)
    m = (torch.arange(T)[None, :] < lens[:, None]).float()
    if S >= 3:
        adv[0], adv[1], adv[2] = 0.0, 0.8, -0.6  # 0 and both signs
        m[S // 2] = 0.0  # two fully masked rows
        m[S - 1] = 0.0
        assert (adv == 0).any() and (adv > 0).any() and (adv < 0).any()
    rho = (d(lp) - d(old)).exp()
    assert ((rho - lo).abs() >= SEP).all() and ((rho - hi).abs() >= SEP).all()
    return {"lp": lp, "old": old, "ref": ref, "adv": adv, "m": m}


def grpo64(lp, old, ref, adv, m, beta, mode, max_len=None, denom=None, clip=GRPO_CLIP):
    lp, old, ref, m = d(lp), d(old), d(ref), d(m)
    a = d(adv).view(-1, 1)
    lo, hi = 1 - clip[0], 1 + clip[1]
    S = lp.shape[0]
    dd = lp - old
    rho = dd.exp()
    l1, l2 = -a * rho, -a * rho.clamp(lo, hi)
    dr = ref - lp
    k3 = dr.exp() - dr - 1
    per = torch.maximum(l1, l2) + beta * k3
    c = m.sum(1)
    w = torch.ones_like(c)
    if mode == "sequence":
        num, div, w = ((per * m).sum(1) / c.clamp(min=1)).sum(), float(S), 1.0 / c.clamp(min=1)
    elif mode == "token":
        num, div = (per * m).sum(), m.sum().clamp(min=1).item()
    else:
        num, div = (per * m).sum(), float(S) * float(max_len)
    if denom is not None:
        div = float(denom)
    n = m.sum()
    inv = 1.0 / n.clamp(min=1)
    out = ((rho < lo) | (rho > hi)).double()
    dlp = m * w[:, None] * (torch.where(l1 >= l2, l1, torch.zeros_like(l1)) - beta * (dr.exp() - 1)) / div
    metrics = torch.stack([(out * m).sum() * inv, (((rho - 1) - dd) * m).sum() * inv, (k3 * m).sum() * inv, n])
    return {"loss": num / div, "dlp": dlp, "metrics": metrics}


# ================================================================================= AdamW
ADAMW_N = [8, 2040, 2048, 2056, 2_097_160]  # the last: nvec = 262145, one past the 1024 x 256 grid
# every value exactly representable in fp32 (see the module docstring)
ADAMW_HP = {"lr": 2.0 ** -7, "b1": 0.875, "b2": 0.9990234375, "eps": 2.0 ** -27}
ADAMW_WD = [0.0, 0.1]
ADAMW_CLIP = [None, 0.37]
ADAMW_GS = [1.0, 0.5]
ADAMW_STEPS = [1, 2, 3, 1000]  # 3 consecutive steps, then one call at step = 1000


def adamw_case(n, grad_dtype, seed=0):
    """w0 (fp32, bf16-representable so every layout starts from the same weights) and one gradient
    per step of ADAMW_STEPS."""
    g = gen(10000 + (n % 9973) + seed)
    w0 = torch.randn(n, generator=g).bfloat16().float()
    grads = [torch.randn(n, generator=g).to(grad_dtype) for _ in ADAMW_STEPS]
    return {"w0": w0, "grads": grads}


def adamw64(w, grad, m, v, step, wd, clip=None, grad_scale=1.0, lr=ADAMW_HP["lr"], b1=ADAMW_HP["b1"],
            b2=ADAMW_HP["b2"], eps=ADAMW_HP["eps"]):
    """One decoupled-decay AdamW step in fp64 -> (w, m, v)."""
    g = d(grad) * grad_scale * (1.0 if clip is None else float(clip))
    w = d(w) * (1 - lr * wd)
    m = b1 * d(m) + (1 - b1) * g
    v = b2 * d(v) + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    w = w - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return w, m, v


def sumsq_case(n, dtype, seed=0, offset=0, total=None):
    g = gen(11000 + (n % 9973) + seed)
    total = n if total is None else total
    return torch.randn(total, generator=g).to(dtype)


def clip_coef64(sumsq, max_norm):
    norm = math.sqrt(float(sumsq))
    return norm, (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)


# ===================================================================== LM-head row kernels
ROW_V = [1003, 2048, 50264]
ROW_N = 9
DEAD_ROW = 2  # the row that carries the -inf logits


def rows_case(kind, N=ROW_N, seed=0, scale=3.0):
    """bf16 logits [N, V] (CPU): V = int(kind), or "sliced": a column-sliced view with ld != V."""
    g = gen(12000 + seed)
    if kind == "sliced":  # ld = 2112, V = 2048
        return (scale * torch.randn(N, 2112, generator=g)).bfloat16()[:, 8:2056]
    return (scale * torch.randn(N, int(kind), generator=g)).bfloat16()


def dead_mask(V, pattern):
    dead = torch.zeros(V, dtype=torch.bool)
    if pattern == "first16":  # a lane's whole first vector / the scalar path's first elements
        dead[:16] = True
    elif pattern == "scattered":
        dead[37::5] = True
    elif pattern == "last":
        dead[V - 1] = True
    else:
        raise ValueError(pattern)
    return dead


DEAD_PATTERNS = ["first16", "scattered", "last"]


def rows_targets(N, V, seed=1):
    t = torch.randint(0, V, (N,), generator=gen(seed))
    t[3] = -100
    return t


def logprob64(x, tgt):
    """lse = logsumexp, logp = log_softmax at the target (0 on ignored rows)."""
    z = d(x)
    lse = torch.logsumexp(z, -1)
    lp = z.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1) - lse
    return {"logp": torch.where(tgt >= 0, lp, torch.zeros_like(lp)), "lse": lse}


def logprob_bwd64(x, tgt, g):
    """dlogits = g (1[v == tgt] - softmax); ignored rows 0; a -inf logit (a masked vocabulary
    entry, p = 0) receives exactly 0."""
    z = d(x)
    p = torch.softmax(z, -1)
    onehot = torch.zeros_like(z)
    onehot.scatter_(-1, tgt.clamp(min=0).unsqueeze(-1), 1.0)
    out = d(g).unsqueeze(-1) * (onehot - p) * (tgt >= 0).double().unsqueeze(-1)
    return out.masked_fill(z == NINF, 0.0)


ENS_SHAPES = [(1, 1000), (33, 1003), (8, 50257)]
ENS_K = [1, 3]


def ensemble_case(N, V, K, seed=0):
    """Student [N, V], teachers [K, N, V] bf16; the last teacher has -inf logits on every row
    (never a whole row), so with K = 1 p_bar is 0 at those positions."""
    g = gen(13000 + V + 17 * K + seed)
    s = (2.0 * torch.randn(N, V, generator=g)).bfloat16()
    t = (2.0 * torch.randn(K, N, V, generator=g)).bfloat16()
    t[K - 1, :, 5::7] = NINF
    t[K - 1, :, :16] = NINF
    return {"s": s, "t": t, "g": torch.randn(N, generator=g)}


def ensemble_kl64(s, t, g):
    logq = torch.log_softmax(d(s), -1)
    pbar = torch.softmax(d(t), -1).mean(0)
    term = torch.where(pbar > 0, pbar * (pbar.clamp(min=1e-300).log() - logq), torch.zeros_like(pbar))
    return {"kl": term.sum(-1), "grad": d(g).unsqueeze(-1) * (logq.exp() - pbar)}
