"""Cases, inputs and fp64 reference for prefix-shared attention (`prefix=` of ops.attention, the
PFX path of attn_fwd_kernel and the non-monotone seg_end of the backward kernels):
test_attention_prefix_cpu.py, test_attention_prefix_gpu.py.

The fp64 `reference`, the elementwise `bounds`, `ratios` and the peaked builder's constants are
those of _attn_ref64.py, unchanged; this module supplies the visibility of the forward form

    visible = j <= i  and  ( j >= seg_start[b, i]  or  ( ps <= j < pe  and  pe <= i < qe ) )

to them for the duration of a call (`_attn_ref64.visibility` is swapped and restored), and a
builder that puts the sentinels of _attn_ref64 (score ~8, v / dO rows of magnitude ~6) on both
sides of every edge the prefix adds: ps, pe, every segment start, the last key of every 64-key
forward tile and of every 256-key backward block. A segment's queries take the edges in turn
(start, start + 1: the segment start and pe; start + 2: ps; start + 3 ...: one prefix tile edge
each), at most two per query as in _attn_ref64 (the e_ij budget).

A batch row is (ps, pe, qe, bounds): prefix slots [ps, pe), segments bounds[k] .. bounds[k+1]
from pe on (segments that start at or past qe are outside the prefix group: they do not see it);
ps == pe: a plain packed row. Slots below ps are left padding: (seg_start, seg_end) = (ps, 0).
"""
import contextlib
import math

import torch

import _attn_ref64 as R
from _attn_ref64 import F64

MUTATIONS = ("pe_plus1", "pe_minus1", "ps_plus1", "ps_minus1", "prefix_hidden", "prefix_external",
             "seg_start_plus1", "seg_start_minus1")


class PCase(R.Case):
    def __init__(self, name, rows, D=128, heads=(4, 2), entry="core", rot=0, ropesw=(1, 1, 0), fwd=(None, 1, 1),
                 bwd=(8, 1, 1)):
        L = rows[0][3][-1]
        assert all(r[3][-1] == L for r in rows)
        super().__init__(name, "peaked", L, D, heads, "causal", B=len(rows), entry=entry, rot=rot, fwd=fwd, bwd=bwd,
                         ropesw=ropesw)
        self.rows = rows
        self.pos = "leftpad" if rot else "default"


def _segs(pe, n, size, extra=()):
    return [pe + k * size for k in range(n + 1)] + list(extra)


def _row(ps, pe, n, size, extra=()):
    b = _segs(pe, n, size, extra)
    return (ps, pe, pe + n * size, b)


ROW_A = _row(0, 70, 4, 20)        # L 150: prefix end and two whole segments inside one 32-key sub-tile
ROW_B = _row(0, 128, 3, 64)       # L 320: edges on tile boundaries, crosses a 256-key block
ROW_C = _row(5, 100, 4, 130)      # L 620: left padding, whole skipped tiles, three key blocks
ROW_D0 = _row(0, 128, 2, 64, extra=(320,))  # qe 256 < L: the last segment is outside the group
ROW_D1 = (0, 0, 0, [0, 37, 64, 65, 256, 300, 320])  # plain packed row


def cases():
    return [PCase("pfx-a", [ROW_A, ROW_A]),
            PCase("pfx-b", [ROW_B, ROW_B]),
            PCase("pfx-c", [ROW_C, ROW_C]),
            PCase("pfx-d", [ROW_D0, ROW_D1]),
            PCase("pfx-a-D64", [ROW_A, ROW_A], D=64),
            PCase("pfx-c-qkv-rope", [ROW_C, ROW_C], entry="qkv", rot=128),
            PCase("pfx-b-qkv-ropefwd", [ROW_B, ROW_B], entry="qkv", rot=128, ropesw=(1, 1, 1))]


# ------------------------------------------------------------------------------------- mask
def layout(c):
    """(segs [2, B, L] int32, prefix [B, 3] int32, pos [B, L] long) of a case."""
    L = c.Tk
    st, en = torch.zeros(c.B, L, dtype=torch.int32), torch.zeros(c.B, L, dtype=torch.int32)
    pos = torch.zeros(c.B, L, dtype=torch.long)
    pf = torch.zeros(c.B, 3, dtype=torch.int32)
    for b, (ps, pe, qe, bd) in enumerate(c.rows):
        pf[b] = torch.tensor([ps, pe, qe])
        st[b, :pe], en[b, ps:pe] = ps, qe
        pos[b, :pe] = (torch.arange(pe) - ps).clamp(min=0)
        for lo, hi in zip(bd[:-1], bd[1:]):
            st[b, lo:hi], en[b, lo:hi] = lo, hi
            # a response segment continues the prompt's positions; a plain row restarts at 0
            pos[b, lo:hi] = torch.arange(hi - lo) + ((pe - ps) if pe > ps and lo < qe else 0)
    return torch.stack([st, en]).contiguous(), pf, pos


def visibility(c, inp, mut=None):
    """[B, T, T] bool: the forward form; `mut` one deliberate error of MUTATIONS."""
    dev = inp["q"].device
    B, T = c.B, c.Tk
    qi = torch.arange(T, device=dev).view(1, T, 1)
    kj = torch.arange(T, device=dev).view(1, 1, T)
    pf = inp["prefix"].long().to(dev).view(B, 3, 1, 1)
    ps, pe, qe = pf[:, 0], pf[:, 1], pf[:, 2]
    has = pe > ps
    dd = {"pe_plus1": (0, 1, 0), "pe_minus1": (0, -1, 0), "ps_plus1": (1, 0, 0), "ps_minus1": (-1, 0, 0),
          "seg_start_plus1": (0, 0, 1), "seg_start_minus1": (0, 0, -1)}.get(mut, (0, 0, 0))
    seg = kj >= inp["segs"][0].long().to(dev).view(B, T, 1) + dd[2]
    qhi = torch.full_like(qe, T) if mut == "prefix_external" else qe
    pre = has & (kj >= ps + dd[0]) & (kj < pe + dd[1]) & (qi >= pe) & (qi < qhi)
    if mut == "prefix_hidden":
        pre = torch.zeros_like(pre)
    return (kj <= qi) & (seg | pre)


def backward_form(c, inp):
    """[B, T, T] bool: j <= i < seg_end[b, j], what the backward kernels evaluate per element."""
    T = c.Tk
    qi = torch.arange(T).view(1, T, 1)
    kj = torch.arange(T).view(1, 1, T)
    return (kj <= qi) & (qi < inp["segs"][1].long().view(c.B, 1, T))


@contextlib.contextmanager
def _vis(mut=None):
    old = R.visibility
    R.visibility = lambda c, inp, _m=None: visibility(c, inp, mut)
    try:
        yield
    finally:
        R.visibility = old


def reference(inp, c, dtype=F64, mut=None):
    with _vis(mut):
        return R.reference(inp, c, dtype)


def bounds(inp, c, r, num):
    with _vis():
        return R.bounds(inp, c, r, num)


# --------------------------------------------------------------------------------- builder
def _edges(c, row):
    """(m, queries) per edge of one batch row: keys m - 1 | m straddle it."""
    ps, pe, qe, bd = row
    L = c.Tk
    near = lambda i: [x for x in (i - 1, i, i + 1) if 0 <= x < L]
    starts = bd[:-1]
    E = []
    if pe > ps:
        ptiles = [m for m in range(R.FWD_KEYS, pe, R.FWD_KEYS) if m > ps and m != pe]
        E.append((ps, near(ps) + [s + 2 for s in starts if s + 2 < L]))
        # pe: the first segment's neighbours, and the first two queries of every other segment
        # (inside the group they see key pe - 1 and not key pe; outside it neither)
        E.append((pe, near(pe) + [x for s in starts[1:] for x in (s, s + 1)]))
        for k, m in enumerate(ptiles):  # prefix tile ends, seen whole by every segment of the group
            E.append((m, near(m) + [s + 3 + k for s, e in zip(starts, bd[1:]) if s + 3 + k < e]))
    for s in starts[1:] if pe > ps else starts:
        E.append((s, near(s)))
    done = {m for m, _ in E}
    E.append((L, near(L)))
    E += [(m, near(m)) for m in range(R.FWD_KEYS, L, R.FWD_KEYS) if m not in done]  # 256-key block ends included
    return E


def build(c, seed=0):
    """Inputs of a case on the CPU, as _attn_ref64.build: q / do [B, L, Hq, D], k / v [B, L, Hkv, D]
    bf16; segs, prefix int32; cos / sin / pos with RoPE. Asserts max e_ij <= EMAX."""
    g = torch.Generator().manual_seed(4321 + seed + sum(map(ord, c.name)))
    B, L, Hq, Hkv, D = c.B, c.Tk, c.Hq, c.Hkv, c.D
    rn = lambda *s: torch.randn(*s, generator=g)
    segs, pf, pos = layout(c)
    inp = {"kv_start": None, "kv_end": None, "segs": segs, "prefix": pf, "cos": None, "sin": None, "pos": None}
    if c.rot:
        inp["cos"], inp["sin"] = R.rope_tables(c.rot)
        inp["pos"] = pos
    q, k, v, do = rn(B, L, Hq, D), rn(B, L, Hkv, D), rn(B, L, Hkv, D), rn(B, L, Hq, D)
    d1, pool = R._sent_dims(c)
    sig, A = math.sqrt(3.7 / c.scale), math.sqrt(8.0 / c.scale)
    q, k = 0.1 * q, 0.1 * k
    q[..., d1] = sig * rn(B, L, Hq).clamp(-1.6, 1.6)
    k[..., d1] = sig * rn(B, L, Hkv).clamp(-1.6, 1.6)
    big = lambda *s: 6.0 * (0.5 + torch.rand(*s, generator=g)) * (2.0 * (torch.rand(*s, generator=g) < 0.5).float() - 1.0)
    for b in range(B):
        kdim, qdim, nxt = {}, {}, 0
        for m, qs in _edges(c, c.rows[b]):
            keys = [j for j in (m - 1, m) if 0 <= j < L]
            dim = next((kdim[j] for j in keys if j in kdim), None)
            if dim is None:
                dim, nxt = pool[nxt % len(pool)], nxt + 1
            for j in keys:
                kdim.setdefault(j, dim)
            for i in qs:
                if dim not in qdim.setdefault(i, []) and len(qdim[i]) < 2:
                    qdim[i].append(dim)
        for j, dim in kdim.items():
            k[b, j, :, dim] = A
            v[b, j] = big(Hkv, D)
        for i, dims in qdim.items():
            q[b, i, :, d1] *= 0.1
            for dim in dims:
                q[b, i, :, dim] = A
            do[b, i] = big(Hq, D)
    inp.update(q=q, k=k, v=v.bfloat16(), do=do.bfloat16())
    num = c.numerics()
    shrink = 1.0
    with _vis():
        for _ in range(2):
            trial = dict(inp, q=(q * shrink).bfloat16(), k=(k * shrink).bfloat16())
            emax, _ = R.score_error(c, R._rotated(trial, c), num)
            if emax <= 0.9 * R.EMAX:
                break
            shrink *= math.sqrt(0.85 * R.EMAX / emax)
    assert emax <= R.EMAX, f"{c.name}: max e_ij {emax:.4f} > {R.EMAX}"
    trial["emax"], trial["shrink"] = emax, shrink
    return trial


_CACHE = {}


def with_bwd(c, waves):
    """The case under another backward variant (4 or 8 waves; same name, so the same inputs)."""
    return PCase(c.name, c.rows, c.D, (c.Hq, c.Hkv), c.entry, c.rot, c.ropesw, c.fwd, (waves, 1, 1))


def built(c, cus=256):
    """(inputs, fp64 reference, bounds, numerics) of a case, computed once per process and shared
    (callers must not modify them). Inputs and reference depend on the name alone, the bound also
    on the backward variant and the CU count (`Case.numerics`: the head split)."""
    if c.name not in _CACHE:
        inp = build(c)
        _CACHE[c.name] = (inp, reference(inp, c))
    inp, r = _CACHE[c.name]
    key = (c.name, c.bwd, cus)
    if key not in _CACHE:
        num = c.numerics(cus)
        _CACHE[key] = (bounds(inp, c, r, num), num)
    return inp, r, _CACHE[key][0], _CACHE[key][1]
