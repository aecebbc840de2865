"""fp64 reference, derived elementwise error bound, input builders and the case grid for the
training attention kernels of csrc/attention.hip (test_attention_ref_cpu.py,
test_attention_fp64_gpu.py). Pure torch, usable on the CPU and on the device; nothing here needs
the HIP extension.

Reference (`reference`): attention in fp64 on the bf16-rounded inputs under the mask contract of
`ops.attention._visibility` (causal with causal_off, window, kv_start / kv_end, segs, GQA), with
fp64 rotate-half RoPE (full or partial `rot`, optional positions, the fp32 cos / sin tables the
kernels read) for the fused-QKV path. Returns O, the natural-log LSE (compare with lse2 * ln 2),
the rows that see no key, and dQ / dK / dV for a given dO by the closed forms
    P = softmax(S),  dP = dO V^T,  Delta_i = sum_j P_ij dP_ij,  dS = P (dP - Delta),
    dQ' = scale dS K',  dK' = scale dS^T Q',  dV = P^T dO,   dq = R^T dQ', dk = R^T dK'
(primes = rotated space; no autograd, no nan_to_num: a row without a visible key has P = 0, so
O = 0, LSE = +inf, dQ = 0 and contributes nothing to dK / dV).

Bound (`bounds`). Every output element is checked as |kernel - ref64| <= bound with
    bound = 2 * first_order + ulp_bf16(ref) [bf16 outputs] + 8 * E32 + 4 ulp32(max |ref|)
Notation: u = 2^-9 per bf16 rounding (common.h f2bf / pack2bf: a plain fp32 -> __bf16 cast,
v_cvt_pk_bf16_f32, round to nearest even), a_ij = scale sum_d |q'_id| |k'_jd| the magnitude
companion of the score, p = P. One line per term, with the kernel line it comes from
(attention.hip unless stated):
  forward
   e_ij  = nf u a_ij            score error, natural units. nf counts the bf16 roundings of a score
                                operand: 1 for `qf[s] = pack_bf16x8(qv * scale2)` (prologue; with
                                RoPE on load the rotation happens in fp32 before that one cast);
                                +1 for K rounded by rope.hip (`f2bf(a * c - b * sn)`) or by
                                rope_rot_chunk as it is staged; +1 for Q rounded by rope.hip when
                                Q is not rotated on load (ROPE_Q_ON_LOAD = 0, or D = 80).
   ebar_i = sum_k p_ik e_ik     |dp_ij| <= p_ij (e_ij + ebar_i) (softmax of perturbed scores)
   LSE:  ebar_i                 `m + __log2f(lsum)`, lsum summed from the fp32 p
   O:    sum_j p_ij (e_ij + ebar_i + u) |v_jd|      `pf = pack8(sacc)`: P.V consumes bf16 p while
                                lsum keeps the fp32 p, so the rounding does not cancel
         + ulp_bf16(O_id)       `pack2bf(o * inv, ...)` (outside the factor 2: one ulp of the
                                reference already is twice the rounding's half ulp)
  backward (attn_bwd_kernel / attn_bwd8_kernel, attn_dq_reduce_kernel, attn_dkv_reduce_kernel)
   g_ij  = nb u a_ij + ebar_i [+ u^2 |LSE_i|]       `ex2(fmaf(sacc, scale2, -lse2))`: p recomputed
                                from the UNSCALED bf16 Q (nb = 0 without RoPE: exact products;
                                2 with RoPE: q_rot and the rotated K are each one bf16 rounding)
                                against the forward's lse2, which carries ebar_i. 8 waves: the row
                                constant enters the MFMA chain as two bf16, `pack2bf(x, x - xh)`,
                                x = -lse2 / scale2: the low half's rounding leaves u^2 |x|.
   dDelta_i = sum_d |dO_id| (EO_id + u |O_id|) [+ u^2 |Delta_i|]   attn_bwd_delta_kernel reads the
                                bf16 O (EO = the forward's first-order term); 8 waves: the same
                                two-bf16 split, `pack2bf(y, y - yh)`.
   EP_ij = p_ij (g_ij + u)      `pb0 = pack8(sacc, 0)`: P rounded for dV^T += dO^T P
   EdS_ij = p_ij g_ij |dP_ij - Delta_i| + p_ij dDelta_i + u |dS_ij|    `sb0 = pack8(dpacc, 0)`
   dV:   sum_{h,i} EP_ij |dO_id|
         [+ u sum_{h,i} p_ij |dO_id|]               bf16 head-split partials, `pack2bf(dv[dt]...)`
                                into dv_part16 (8 waves, hsplit > 1, DLA_ATTN_DKV_BF16 != 0)
   dK':  scale sum_{h,i} EdS_ij |q'_id|
         [+ u M^K_jd], M^K = scale sum |dS_ij| |q'_id|   with RoPE: q_rot is a bf16 rounding
         [+ u M^K_jd]                               bf16 partials (dk_part16), as dV
   dQ':  scale sum_j EdS_ij |k'_jd|
         [+ u M^Q_id], M^Q = scale sum_j |dS_ij| |k'_jd|   with RoPE: the rotated K is rounded
         [+ u M^Q_id]                               bf16 slab per 256-key block, `f2bf(acc[t][e] *
                                p.scale)` into dq_slab16 (8 waves, DLA_ATTN_DQ_BF16 != 0): the
                                blocks' magnitudes sum to M^Q
   RoPE: [+ u |dQ'|, u |dK'|]   only with the separate rope_bwd kernel (FUSED_ROPE_BWD = 0): the
                                attention passes round the rotated-space gradients to bf16 first.
         The un-rotation itself (rope_unrotate8 / the dK epilogue, fp32) adds nothing at this
         order; a rotated-space bound E' maps to |c| E'_d + |s| E'_partner.
   + ulp_bf16(ref) for the final `pack_bf16x8` of dQ / dK / dV.
  fp32 accumulation, v_exp_f32 / v_log_f32: the `MARGIN * E32 + FLOOR_ULPS ulp32` allowance of
   _refs64.py, with E32 = max |this reference evaluated in fp32 - in fp64| per output.
  factor 2: the neglected second-order terms; honest while max e_ij <= EMAX = 0.05 (e^0.05 - 1 =
   1.025 * 0.05), which `build` asserts over the visible scores with max(nf, nb) roundings.
  exact zeros: where the first-order term is exactly 0 (every element of a row without a visible
   key, of a key no query sees) the bound is 0: the fp32 allowance is not granted there.
No other constant enters. (u = 2^-9 is the mean-case unit roundoff of an 8-bit significand; its
worst case, 2^-8 at the bottom of a binade, is what the factor 2 reaches at first order.)

Builders (`build`): seeded, values held in fp32 and rounded to bf16 once.
  flat    N(0,1) q, k, v, dO as in test_kernels_gpu.py.
  peaked  scores of sd ~3: one "background" dim of q and k carries a clamped Gaussian (a rank-one
          score pattern; under RoPE modulated by cos of the position difference), every other dim
          0.1 N(0,1). At every mask edge of the case -- causal diagonal, kv_start, kv_end, the
          window's lower edge, every segment start, the last key of every 64-key forward tile and
          of every 256-key backward block -- the last visible and the first invisible key share a
          sentinel dim with the neighbouring queries (score ~8 against them, background damped
          there), carry a v row of magnitude ~6 and those queries a dO row of magnitude ~6. One
          key wrongly seen or dropped then moves O, dQ, dK, dV by many times the bound.
Both families shrink q and k by one common factor when the e_ij budget needs it (three bf16
roundings per score on the rope-kernel path), and say so in the returned dict.
"""
import math

import torch

F64 = torch.float64
U = 2.0 ** -9
EPS32 = 2.0 ** -23
MARGIN = 8.0  # as _refs64.py
FLOOR_ULPS = 4.0
EMAX = 0.05
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
FWD_KEYS = 64
BWD_KEYS = 256
OUTPUTS = ("o", "lse", "dq", "dk", "dv")


# ------------------------------------------------------------------------------------ cases
class Case:
    """One point of the grid. fwd = (persist, msub, ostage) with persist None = the kernel's own
    choice; bwd = (waves, dq_bf16, dkv_bf16); ropesw = (q_on_load, fused_bwd, fused_fwd)."""

    def __init__(self, name, fam, T, D, heads, mask, B=2, entry="core", rot=0, pos="default",
                 fwd=(None, 1, 1), bwd=(8, 1, 1), ropesw=(1, 1, 0), layout="contig", Tq=None,
                 off=None):
        self.name, self.fam, self.D, self.mask = name, fam, D, mask
        self.Hq, self.Hkv = heads
        self.Tk, self.Tq = T, (T if Tq is None else Tq)
        self.B = B
        self.entry, self.rot, self.pos, self.fwd, self.bwd, self.ropesw = entry, rot, pos, fwd, bwd, ropesw
        self.layout = layout
        self.causal = mask != "full"
        self.causal_off = (self.Tk - self.Tq) if off is None else off
        self.window = {"win1": 1, "win48": 48, "win300": 300}.get(mask, 0)
        self.scale = 1.0 / math.sqrt(D)
        T = self.Tk
        self.ks = self.ke = self.segb = None
        if mask == "lpad":
            self.ks = [0, T // 3 + 1]
        elif mask == "rpad":  # row 0 right padded, row 1 empty (kv_end == kv_start), row 2 full
            e = min(7, T)
            self.B = 3
            self.ks = [0, e, 0]
            self.ke = [max(T - T // 4, 1), e, T]
        elif mask == "segs":
            cand = [[0, 37, 64, 65, 256, 300, 512], [0, 1, 63, 128, 256, 257, 500]]
            self.segb = [[x for x in cand[b % 2] if x < T] + [T] for b in range(self.B)]
        if pos == "leftpad":
            assert mask == "lpad" and rot > 0

    def __repr__(self):
        return self.name

    def numerics(self, cus=256):
        """The rounding points the case's variant goes through (see the module docstring)."""
        D, rot = self.D, self.rot
        q_on_load, fused_bwd, fused_fwd = self.ropesw
        full = rot == D and D in (64, 128)
        on_load = rot > 0 and full and bool(fused_fwd)
        q_load = rot > 0 and full and bool(q_on_load) and not on_load
        nf = 1 if rot == 0 else (2 if (q_load or on_load) else 3)
        nb = 0 if rot == 0 else 2
        fused = (full or (D == 80 and rot == 32)) and (bool(fused_bwd) or on_load)
        waves, dq16, dkv16 = self.bwd
        nkb = (self.Tk + BWD_KEYS - 1) // BWD_KEYS
        group = self.Hq // self.Hkv
        base, target, hs = nkb * self.Hkv * self.B, (2 * cus if self.causal else cus), 1
        while base * hs < target and group % (2 * hs) == 0:  # bindings.cpp attn_bwd_hsplit
            hs *= 2
        return {"nf": nf, "nb": nb, "rope": rot > 0, "extra_round": rot > 0 and not fused,
                "w8": waves == 8, "slab16": waves == 8 and bool(dq16),
                "part16": waves == 8 and bool(dkv16) and hs > 1, "hs": hs, "nkb": nkb}


MASKS = ["causal", "full", "win1", "win48", "win300", "lpad", "rpad", "segs", "cross", "cross0"]
HEADS = [(4, 4), (6, 3), (8, 2), (8, 1), (3, 1)]
FWD_VARIANTS = [(1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 1, 0), (0, 0, 0)]
BWD_VARIANTS = [(8, 1, 1), (8, 0, 1), (8, 1, 0), (8, 0, 0), (4, 1, 1)]
FAMS = ["flat", "peaked"]
T_AXIS = [1, 31, 33, 64, 65, 255, 257, 300, 520, 577]


def _mk(name, fam, T, D, heads, mask, **kw):
    if mask == "cross":  # Tq < Tk, causal_off = Tk - Tq (the default of attention_core)
        return Case(name, fam, T, D, heads, "cross", Tq=5, **kw)
    if mask == "cross0":  # Tq < Tk with an explicit causal_off = 0
        return Case(name, fam, T, D, heads, "cross0", Tq=5, off=0, **kw)
    return Case(name, fam, T, D, heads, mask, **kw)


def grid():
    """The covering set (about 190 cases): every value of every axis with both families; every
    mask kind against every forward and every backward variant at T = 520 / 577 (cross: Tk)."""
    cs, n = [], 0
    # 1. mask x variant at a length past the 64-, 256- and 512-key boundaries, D = 128 (the only
    #    head dim with the msub / ostage paths)
    for mi, mask in enumerate(MASKS):
        for vi in range(5):
            fam = FAMS[(mi + vi) % 2]
            T = (520, 577)[(mi + vi) % 2] if mask not in ("cross", "cross0") else 577
            heads = HEADS[(mi + vi) % 5]
            cs.append(_mk(f"mv-{mask}-f{vi}-{fam}", fam, T, 128, heads, mask, fwd=FWD_VARIANTS[vi],
                          bwd=BWD_VARIANTS[vi]))
    for mask in ("cross", "cross0"):  # the issue's 5 against 300
        for fam in FAMS:
            cs.append(_mk(f"x300-{mask}-{fam}", fam, 300, 128, (8, 2), mask))
    # 2. every T with both families (default variants), masks / D / heads cycling
    tm = ["causal", "lpad", "win48", "rpad", "full", "segs", "win1", "win300"]
    for ti, T in enumerate(T_AXIS):
        for fi, fam in enumerate(FAMS):
            mask = tm[(ti + 3 * fi) % len(tm)]
            if mask == "segs" and T < 31:
                mask = "causal"
            cs.append(_mk(f"t{T}-{mask}-{fam}", fam, T, (64, 80, 128)[(ti + fi) % 3], HEADS[(ti + 2 * fi) % 5], mask,
                          bwd=BWD_VARIANTS[(ti + fi) % 5]))
    # 3. D x heads with both families at T = 300 (HP 1 / 2 / 4, hsplit, odd group)
    for di, D in enumerate((64, 80, 128)):
        for hi, heads in enumerate(HEADS):
            for fi, fam in enumerate(FAMS):
                mask = tm[(di + hi + fi) % len(tm)]
                cs.append(_mk(f"dh-D{D}-h{heads[0]}x{heads[1]}-{mask}-{fam}", fam, 300, D, heads, mask,
                              fwd=(None, 1, 1) if fi else (0, 1, 1), bwd=BWD_VARIANTS[(di + hi) % 5]))
    # 4. fused-QKV entry with RoPE
    rm = ["causal", "full", "win48", "rpad", "segs", "win300"]
    for D, rot in ((64, 64), (128, 128), (80, 32)):
        sws = [(1, 1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 0), (1, 1, 1)] if rot == D else [(1, 1, 0), (1, 0, 0)]
        for si, sw in enumerate(sws):
            for pi, pos in enumerate(("default", "leftpad")):
                for fi, fam in enumerate(FAMS):
                    n += 1
                    mask = "lpad" if pos == "leftpad" else rm[n % len(rm)]
                    T = (65, 257, 300, 577)[n % 4]
                    cs.append(_mk(f"rope-D{D}-sw{''.join(map(str, sw))}-{pos}-{mask}-T{T}-{fam}", fam, T, D,
                                  HEADS[n % 5], mask, entry="qkv", rot=rot, pos=pos, ropesw=sw,
                                  bwd=BWD_VARIANTS[n % 5], fwd=(None, 1, 1) if n % 3 else (0, 0, 1)))
    # 5. fused-QKV entry without RoPE, and the layouts of the core entry
    for fi, fam in enumerate(FAMS):
        for di, D in enumerate((64, 80, 128)):
            cs.append(_mk(f"qkv-norope-D{D}-{fam}", fam, 257, D, HEADS[(di + fi + 1) % 5], tm[(di + fi) % 5],
                          entry="qkv", bwd=BWD_VARIANTS[(di + 2 * fi) % 5]))
        for li, layout in enumerate(("qkvview", "do_nc")):
            for di, D in enumerate((64, 128)):
                cs.append(_mk(f"lay-{layout}-D{D}-{fam}", fam, 300, D, HEADS[(li + di + 2) % 5],
                              ("lpad", "causal", "full")[(li + di + fi) % 3], layout=layout,
                              bwd=BWD_VARIANTS[(li + di + fi) % 5]))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


# ------------------------------------------------------------------------------------- RoPE
def rope_tables(rot, max_pos=1024, theta=10000.0):
    """fp32 cos / sin [max_pos, rot/2], the formula of ops.attention.RotaryCache."""
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=F64) / rot))
    fr = torch.outer(torch.arange(max_pos, dtype=F64), inv)
    return fr.cos().float(), fr.sin().float()


def rope(x, cos, sin, pos, rot, inverse=False, sign=1.0):
    """x [B, H, T, D] (any float dtype), pos [B, T] long: rotate-half over the first rot dims, or
    with inverse the gradient un-rotation (lo = a c + b s, hi = b c - a s)."""
    c = cos.to(x.dtype)[pos].unsqueeze(1)
    s = sin.to(x.dtype)[pos].unsqueeze(1) * (-sign if inverse else 1.0)
    h = rot // 2
    x1, x2 = x[..., :h], x[..., h:rot]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s, x[..., rot:]], dim=-1)


def rope_abs(e, cos, sin, pos, rot):
    """A rotated-space error bound through the un-rotation: |c| e_d + |s| e_partner."""
    c = cos.to(e.dtype)[pos].unsqueeze(1).abs()
    s = sin.to(e.dtype)[pos].unsqueeze(1).abs()
    h = rot // 2
    e1, e2 = e[..., :h], e[..., h:rot]
    return torch.cat([e1 * c + e2 * s, e2 * c + e1 * s, e[..., rot:]], dim=-1)


# ------------------------------------------------------------------------------------- mask
def visibility(c, inp, mut=None):
    """[B, Tq, Tk] bool, the contract of ops.attention._visibility; `mut` names one deliberate
    off-by-one (test_attention_ref_cpu.py)."""
    dev = inp["q"].device
    B, Tq, Tk = c.B, c.Tq, c.Tk
    qi = torch.arange(Tq, device=dev).view(1, Tq, 1)
    kj = torch.arange(Tk, device=dev).view(1, 1, Tk)
    d = {"causal_lt": ("c", -1), "causal_plus1": ("c", 1), "window_lo_plus1": ("w", 1), "window_lo_minus1": ("w", -1),
         "kv_end_plus1": ("e", 1), "kv_end_minus1": ("e", -1), "kv_start_plus1": ("s", 1),
         "kv_start_minus1": ("s", -1), "seg_start_plus1": ("g", 1), "seg_start_minus1": ("g", -1)}.get(mut, ("", 0))
    dd = lambda k: d[1] if d[0] == k else 0
    ok = torch.ones(B, Tq, Tk, dtype=torch.bool, device=dev)
    if inp["segs"] is not None:
        ok = ok & (kj >= inp["segs"][0].long().view(B, Tq, 1) + dd("g"))
    if inp["kv_start"] is not None:
        ok = ok & (kj >= inp["kv_start"].long().view(B, 1, 1) + dd("s"))
    kend = inp["kv_end"].long().view(B, 1, 1) if inp["kv_end"] is not None else torch.full((B, 1, 1), Tk, device=dev)
    ok = ok & (kj < kend + dd("e"))
    if c.causal:
        ok = ok & (kj <= qi + c.causal_off + dd("c"))
        if c.window > 0:
            ok = ok & (kj > qi + c.causal_off - c.window + dd("w"))
    if mut == "drop_tail_tile":  # the last, partial 64-key tile of the key range never staged
        ok = ok & (kj < kend - kend % FWD_KEYS)
    return ok


def head_map(c, dev, mut=None):
    hq = torch.arange(c.Hq, device=dev)
    return hq % c.Hkv if mut == "gqa_mod" else hq // (c.Hq // c.Hkv)


# -------------------------------------------------------------------------------- reference
def reference(inp, c, dtype=F64):
    """Attention forward and closed-form backward in `dtype` (fp64: the reference; fp32: the E32
    of the bound). Outputs o / dq [B, Tq, Hq, D], dk / dv [B, Tk, Hkv, D], lse / nokey
    [B, Hq, Tq]; the rest are the intermediates `bounds` needs ([B, H, T, .] layout)."""
    q, k, v, do = (inp[x].to(dtype).transpose(1, 2) for x in ("q", "k", "v", "do"))
    dev = q.device
    if c.rot:
        q = rope(q, inp["cos"], inp["sin"], inp["pos"], c.rot)
        k = rope(k, inp["cos"], inp["sin"], inp["pos"], c.rot)
    hm = head_map(c, dev)
    ke, ve = k[:, hm], v[:, hm]
    ok = visibility(c, inp).unsqueeze(1)
    s = (q @ ke.transpose(-1, -2)) * c.scale
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m0)
    l = e.sum(-1, keepdim=True)
    nokey = (~ok.any(-1)).expand(c.B, c.Hq, c.Tq)
    P = e / torch.where(l > 0, l, torch.ones_like(l))
    lse = torch.where(l > 0, m0 + torch.log(torch.where(l > 0, l, torch.ones_like(l))),
                      torch.full_like(l, float("inf"))).squeeze(-1)
    O = P @ ve
    dP = do @ ve.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQr = c.scale * (dS @ ke)
    dKr = torch.zeros(c.B, c.Hkv, c.Tk, c.D, dtype=dtype, device=dev).index_add_(1, hm, c.scale * (dS.transpose(-1, -2) @ q))
    dV = torch.zeros(c.B, c.Hkv, c.Tk, c.D, dtype=dtype, device=dev).index_add_(1, hm, P.transpose(-1, -2) @ do)
    dq, dk = dQr, dKr
    if c.rot:
        dq = rope(dQr, inp["cos"], inp["sin"], inp["pos"], c.rot, inverse=True)
        dk = rope(dKr, inp["cos"], inp["sin"], inp["pos"], c.rot, inverse=True)
    return {"o": O.transpose(1, 2), "lse": lse, "nokey": nokey, "dq": dq.transpose(1, 2), "dk": dk.transpose(1, 2),
            "dv": dV.transpose(1, 2), "P": P, "dS": dS, "dP": dP, "delta": delta, "qr": q, "kr": k, "dQr": dQr,
            "dKr": dKr, "ok": ok}


def bf16_ulp(x):
    """One bf16 ulp (8 significand bits) of each element of x (fp64); 0 at 0."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.where(x == 0, torch.zeros_like(x), torch.pow(torch.tensor(2.0, dtype=F64, device=x.device), e - 7))


def score_error(c, r, num):
    """e_ij of the builder's assertion: max(nf, nb) u a_ij over the visible scores; and a_ij."""
    hm = head_map(c, r["qr"].device)
    a = c.scale * (r["qr"].abs() @ r["kr"][:, hm].abs().transpose(-1, -2))
    e = max(num["nf"], num["nb"]) * U * a
    return torch.where(r["ok"], e, torch.zeros_like(e)).max().item(), a


def bounds(inp, c, r, num, r32=None):
    """The elementwise bounds of the module docstring, one fp64 tensor per output (the layout of
    `reference`'s outputs). r = reference(fp64); r32 = reference(fp32) (computed when None)."""
    if r32 is None:
        r32 = reference(inp, c, torch.float32)
    dev = r["qr"].device
    hm = head_map(c, dev)
    P, dS, dP, delta = r["P"], r["dS"], r["dP"], r["delta"]
    qa, ka = r["qr"].abs(), r["kr"][:, hm].abs()
    va = inp["v"].to(F64).transpose(1, 2)[:, hm].abs()
    doa = inp["do"].to(F64).transpose(1, 2).abs()
    O = r["o"].transpose(1, 2)
    _, a = score_error(c, r, num)
    ef = num["nf"] * U * a
    ebar = (P * ef).sum(-1, keepdim=True)
    EO = (P * (ef + ebar + U)) @ va
    lse = r["lse"].unsqueeze(-1)
    lse_abs = torch.where(torch.isinf(lse), torch.zeros_like(lse), lse.abs())
    g = num["nb"] * U * a + ebar + (U * U * lse_abs if num["w8"] else 0.0)
    ddelta = (doa * (EO + U * O.abs())).sum(-1, keepdim=True) + (U * U * delta.abs() if num["w8"] else 0.0)
    EP = P * (g + U)
    EdS = P * g * (dP - delta).abs() + P * ddelta + U * dS.abs()
    nrnd = (1 if num["rope"] else 0)
    MK = c.scale * (dS.abs().transpose(-1, -2) @ qa)
    MQ = c.scale * (dS.abs() @ ka)
    MV = P.transpose(-1, -2) @ doa
    EdV = EP.transpose(-1, -2) @ doa + (U * MV if num["part16"] else 0.0)
    EdK = c.scale * (EdS.transpose(-1, -2) @ qa) + (nrnd + (1 if num["part16"] else 0)) * U * MK
    EdQ = c.scale * (EdS @ ka) + (nrnd + (1 if num["slab16"] else 0)) * U * MQ
    z = lambda: torch.zeros(c.B, c.Hkv, c.Tk, c.D, dtype=F64, device=dev)
    EdK, EdV = z().index_add_(1, hm, EdK), z().index_add_(1, hm, EdV)
    if num["extra_round"]:
        EdQ = EdQ + U * r["dQr"].abs()
        EdK = EdK + U * r["dKr"].abs()
    if c.rot:
        EdQ = rope_abs(EdQ, inp["cos"], inp["sin"], inp["pos"], c.rot)
        EdK = rope_abs(EdK, inp["cos"], inp["sin"], inp["pos"], c.rot)
    first = {"o": EO.transpose(1, 2), "lse": ebar.squeeze(-1), "dq": EdQ.transpose(1, 2), "dk": EdK.transpose(1, 2),
             "dv": EdV.transpose(1, 2)}
    out, e32s = {}, {}
    for name in OUTPUTS:
        ref = r[name]
        fin = torch.isfinite(ref)
        e32 = (r32[name].to(F64) - ref)[fin].abs().max().item() if fin.any() else 0.0
        top = ref[fin].abs().max().item() if fin.any() else 0.0
        b = 2.0 * first[name] + MARGIN * e32 + FLOOR_ULPS * EPS32 * top
        if name != "lse":
            b = b + bf16_ulp(ref)
        # rows without a visible key, keys no query sees: the contract is exact (0, +inf)
        b = torch.where(first[name] == 0, torch.zeros_like(b), b) if name != "lse" else b
        out[name] = torch.where(fin, b, torch.zeros_like(b))
        e32s[name] = e32
    out["e32"] = e32s
    return out


def ratios(got, r, bnd):
    """max |got - ref| / bound per output over EVERY element (0 / 0 = 0, x / 0 = inf, NaN = inf);
    a non-finite reference entry (the +inf LSE of a row without keys) must be met exactly."""
    res = {}
    for name in OUTPUTS:
        ref, b = r[name], bnd[name]
        x = got[name].to(F64)
        assert x.shape == ref.shape, f"{name}: shape {tuple(x.shape)} vs {tuple(ref.shape)}"
        fin = torch.isfinite(ref)
        inf = torch.full_like(ref, float("inf"))
        zero = torch.zeros_like(ref)
        err = (x - torch.where(fin, ref, zero)).abs()
        ratio = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err == 0, zero, inf))
        ratio = torch.where(torch.isnan(err), inf, ratio)
        ratio = torch.where(fin, ratio, torch.where(x == ref, zero, inf))
        res[name] = float(ratio.max().item()) if ref.numel() else 0.0
    return res


def fmt(res):
    return "  ".join(f"{k} {v:.3f}" for k, v in res.items())


# --------------------------------------------------------------------------------- builders
def _sent_dims(c):
    """(background dim, sentinel dim pool). Under RoPE only dims of the low half whose rotary
    frequency is at most 0.05 rad / position (neighbouring positions stay coherent) and, with a
    partial rotary, the dims past `rot`; without RoPE every dim."""
    if c.rot == 0:
        pool = list(range(c.D))
    else:
        h = c.rot // 2
        pool = [d for d in range(h) if 10000.0 ** (-2.0 * d / c.rot) <= 0.05] + list(range(c.rot, c.D))
    return pool[0], pool[1:]


def _edges(c, kbeg, kend, segb):
    """Mask edges of one batch row as (m, queries): keys m - 1 | m straddle the edge."""
    Tq, Tk, off, W = c.Tq, c.Tk, c.causal_off, c.window

    def near(i):
        qs = [x for x in (i - 1, i, i + 1) if 0 <= x < Tq]
        return qs

    tiles = set(range(FWD_KEYS, Tk, FWD_KEYS))
    ms = {Tk, kbeg, kend}
    if segb:
        ms |= set(segb[1:-1])
    if c.causal:
        ms |= {off + 1, Tq - 1 + off, Tq + off}
    # the mask's own edges first (they get first call on the neighbouring queries), tile ends last
    ms = sorted(m for m in ms if 0 <= m <= Tk)
    ms += sorted(tiles - set(ms))
    E = []
    for m in ms:
        qs = near(m - off) if c.causal else near(m % Tq)
        E.append((m, qs or [m % Tq, (m + 1) % Tq]))
    if c.causal and W > 0:
        for m in ms + [Tq + off - W]:
            qs = near(m - 1 - off + W)
            if qs and 0 <= m <= Tk:
                E.append((m, qs))
    return E


def build(c, seed=0):
    """Inputs of a case on the CPU: q / do [B, Tq, Hq, D], k / v [B, Tk, Hkv, D] bf16; cos, sin,
    pos (RoPE); kv_start, kv_end, segs int32 or None. Asserts max e_ij <= EMAX."""
    g = torch.Generator().manual_seed(1234 + seed + sum(map(ord, c.name)))
    B, Tq, Tk, Hq, Hkv, D = c.B, c.Tq, c.Tk, c.Hq, c.Hkv, c.D
    rn = lambda *s: torch.randn(*s, generator=g)
    inp = {"kv_start": None, "kv_end": None, "segs": None, "cos": None, "sin": None, "pos": None}
    if c.ks is not None:
        inp["kv_start"] = torch.tensor(c.ks, dtype=torch.int32)
    if c.ke is not None:
        inp["kv_end"] = torch.tensor(c.ke, dtype=torch.int32)
    if c.segb is not None:
        st, en = torch.zeros(B, Tq, dtype=torch.int32), torch.zeros(B, Tq, dtype=torch.int32)
        for b, bd in enumerate(c.segb):
            for lo, hi in zip(bd[:-1], bd[1:]):
                st[b, lo:hi], en[b, lo:hi] = lo, hi
        inp["segs"] = torch.stack([st, en]).contiguous()
    if c.rot:
        inp["cos"], inp["sin"] = rope_tables(c.rot)
        pos = torch.arange(Tk).expand(B, Tk).clone()
        if c.pos == "leftpad":
            pos = (pos - torch.tensor(c.ks).view(B, 1)).clamp(min=0)
        inp["pos"] = pos
    q, k, v, do = rn(B, Tq, Hq, D), rn(B, Tk, Hkv, D), rn(B, Tk, Hkv, D), rn(B, Tq, Hq, D)
    if c.fam == "peaked":
        d1, pool = _sent_dims(c)
        sig, A = math.sqrt(3.7 / c.scale), math.sqrt(8.0 / c.scale)
        q, k = 0.1 * q, 0.1 * k
        q[..., d1] = sig * rn(B, Tq, Hq).clamp(-1.6, 1.6)
        k[..., d1] = sig * rn(B, Tk, Hkv).clamp(-1.6, 1.6)
        big = lambda *s: 6.0 * (0.5 + torch.rand(*s, generator=g)) * (2.0 * (torch.rand(*s, generator=g) < 0.5).float() - 1.0)
        for b in range(B):
            kbeg = c.ks[b] if c.ks is not None else 0
            kend = c.ke[b] if c.ke is not None else Tk
            kdim, qdim, nxt = {}, {}, 0
            for m, qs in _edges(c, kbeg, kend, c.segb[b] if c.segb else None):
                keys = [j for j in (m - 1, m) if 0 <= j < Tk]
                dim = next((kdim[j] for j in keys if j in kdim), None)
                if dim is None:
                    dim, nxt = pool[nxt % len(pool)], nxt + 1
                for j in keys:
                    kdim.setdefault(j, dim)
                for i in qs:  # at most two edges per query (the e_ij budget: a_ij ~ 8 per edge)
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
    else:
        assert c.fam == "flat"
    inp.update(q=q, k=k, v=v.bfloat16(), do=do.bfloat16())
    num = c.numerics()
    shrink = 1.0
    for _ in range(2):  # fit the e_ij budget: q, k shrink by one common factor, then round once
        trial = dict(inp, q=(q * shrink).bfloat16(), k=(k * shrink).bfloat16())
        emax, _ = score_error(c, _rotated(trial, c), num)
        if emax <= 0.9 * EMAX:
            break
        shrink *= math.sqrt(0.85 * EMAX / emax)
    assert emax <= EMAX, f"{c.name}: max e_ij {emax:.4f} > {EMAX}"
    trial["emax"], trial["shrink"] = emax, shrink
    return trial


def _rotated(inp, c):
    """The rotated q / k and the mask alone (what score_error needs), without the whole reference."""
    q, k = (inp[x].to(F64).transpose(1, 2) for x in ("q", "k"))
    if c.rot:
        q = rope(q, inp["cos"], inp["sin"], inp["pos"], c.rot)
        k = rope(k, inp["cos"], inp["sin"], inp["pos"], c.rot)
    return {"qr": q, "kr": k, "ok": visibility(c, inp).unsqueeze(1)}


def to_device(inp, dev):
    return {k: (x.to(dev) if torch.is_tensor(x) else x) for k, x in inp.items()}
