"""Plain fp64 references, input builders and derived error terms for the memory-bound block
kernels: csrc/norm.hip, elementwise.hip, rope.hip, embedding.hip, reward_head.hip, transpose.hip
(test_block_refs_cpu.py, test_block_kernels_fp64_gpu.py).

Written from the kernel comments and the op docstrings; nothing here imports the package's ops and
nothing needs a GPU. Every reference takes the exact bf16 / fp32 CPU tensors the kernel sees,
widens them to fp64 and returns a dict of fp64 tensors, one entry per output.

Two roundings are part of a kernel's contract and are applied by the reference:
  * the residual stream s = bf16(x + r) (fp32 add of the two bf16 values, one rounding);
  * mean pooling of the reward head ("the reference pools in bf16"): pooled = bf16(sum / count).

Bound: `_refs64.check`, |out - ref64| <= MARGIN * E32 + FLOOR_ULPS ulp32(max |ref64|) + extra, one
bf16 ulp of the reference element on top for bf16 outputs; `check` below then asks the same with
half a bf16 ulp (one round-to-nearest), the form the figures are reported in. The one output that
keeps the whole ulp is the reward head's mean-pooled row, a rounded value that the fp32 and the
fp64 mean may round to different neighbours. E32 comes from the package's CPU branch
in fp32 (_branch32_block.py); `extra` is derived below, next to each family, from what that branch
does not have (__expf, rsqrtf, tanhf, the kernel's summation order). U32 = 2^-24 is the unit
roundoff of one fp32 operation. A sum whose inputs each pass through at most `depth` additions has
|error| <= depth * U32 * sum |terms| to first order, whatever the order (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2); `depth` is read off each kernel below.

Outputs are checked per row group (`groups`): rows with a planted scale (the all-zero row, whose
rstd is 1 / sqrt(eps); the mean-30 rows) get E32, the floor and `extra` from their own rows, so they
do not loosen the bound of the ordinary rows. Every row is in exactly one group.
"""
import math

import torch

import _refs64 as R
from _refs64 import EPS32, F64, d, gen  # noqa: F401

U32 = 2.0 ** -24
BF = torch.bfloat16


def bfr(x):
    """Round to bf16 (the kernel's input precision)."""
    return x.to(BF)


def check(kernel, name, got, ref, e32, extra=0.0, bf16=False):
    """`_refs64.check` (for bf16 outputs: a whole bf16 ulp on top of the fp32 bound), then for bf16
    outputs the same with HALF a bf16 ulp of the reference element, which is what one
    round-to-nearest of the fp32 value costs: |bf16(v) - ref| <= |v - ref| + ulp(v) / 2, and ulp(v)
    exceeds ulp(ref) only if |v| >= 2^k > |ref|, where v rounds to 2^k itself unless |v - ref| is a
    whole ulp(ref) already. Returns (err, bound) of the tighter form and prints it."""
    err, bound = R.check(kernel, name, got, ref, e32, extra, bf16)
    if not bf16:
        return err, bound
    g, r = d(got.cpu()).reshape(-1), d(ref).reshape(-1)
    fin = torch.isfinite(r)
    diff = ((g[fin] - r[fin]).abs() - 0.5 * R.bf16_ulp(r[fin])).clamp(min=0.0)
    err = diff.max().item() if fin.any() else 0.0
    print(f"FIG {kernel} {name} (half ulp): err {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{kernel}/{name}: max abs err beyond half a bf16 ulp {err:.3e} > bound {bound:.3e}"
    return err, bound


# ========================================================================================= norm
# Launcher edges (csrc/norm.hip): rows < 512 -> norm_fwd_row_kernel (block per row, H / 8 threads
# rounded to a wave, 16 `red` slots at H = 8192); rows >= 512 -> norm_fwd_kernel (wave per row,
# NC = 1, 2, 4, 8, 16 chunks of 64 x 8 columns, four rows per block). Backward: grid min(rows, 768),
# 256 threads x NC chunks, parity double buffer on the second and third trip; wgrad fold = kSplit
# (16) stage-1 splits of ceil(grid / 16) partial rows, then 16 rows in stage 2.
NORM_FWD_ROW_H = [8, 136, 520, 4096, 8192]
NORM_FWD_ROW_ROWS = [1, 5, 300]
NORM_FWD_WAVE_H = [8, 512, 520, 1536, 2560, 4104, 8192]
NORM_FWD_WAVE_ROWS = [512, 513, 515]
NORM_BWD_ROWS = [1, 5, 300, 768, 769, 1537]
NORM_BWD_H = [8, 2048, 2056, 4096, 8192]
NORM_FLAGS = [(True, False, False), (True, True, False), (False, False, False), (False, False, True),
              (False, True, False), (False, True, True)]  # (rms, residual, bias): the six valid ones
NORM_EPS = [1e-5, 1e-6]
K_SPLIT = 16
NORM_BWD_GRID = 768


def norm_fwd_nc(H):
    """NC of the wave-per-row forward kernel (chunks_for(H, 64))."""
    need = (H // 8 + 63) // 64
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else 16


def norm_grid_cases():
    """Covering grid of forward cases: every H x rows of both kernels, the flag combinations, eps
    and the bias cycled over it (every flag set meets both kernels and both eps)."""
    out = []
    i = 0
    for Hs, Rs in ((NORM_FWD_ROW_H, NORM_FWD_ROW_ROWS), (NORM_FWD_WAVE_H, NORM_FWD_WAVE_ROWS)):
        for H in Hs:
            for rows in Rs:
                rms, res, bias = NORM_FLAGS[i % 6]
                out.append((rows, H, rms, res, bias, NORM_EPS[(i // 6) % 2]))
                i += 1
    return out


def norm_bwd_cases():
    """(rows, H, rms, dres, bias, eps): every rows and every H at least once, every flag set, 769 and
    1537 (second / third trip) with both norm types, 5 rows (empty stage-1 splits) with bias."""
    return [(1, 8, True, False, False, 1e-5), (5, 2056, False, True, True, 1e-6), (5, 8192, True, True, False, 1e-5),
            (300, 4096, False, False, False, 1e-5), (300, 2048, False, False, True, 1e-6),
            (768, 2048, True, False, False, 1e-6), (769, 8192, False, True, True, 1e-5),
            (769, 2056, True, True, False, 1e-5), (1537, 2056, False, True, False, 1e-6),
            (1537, 4096, True, False, False, 1e-5), (769, 8, False, False, True, 1e-5)]


def norm_case(rows, H, rms, res, bias, seed=0):
    """bf16 x, res, w, b, dy, dres. With rows >= 3: row 1 is all zero (x and res), and for LayerNorm
    row 2 (and the last row) has mean 30, std 0.5. Returns the tensors and the row groups."""
    g = gen(20000 + 31 * rows + H + seed)
    x = torch.randn(rows, H, generator=g)
    r = torch.randn(rows, H, generator=g) if res else None
    zero, off = [], []
    if rows >= 3:
        zero = [1]
        x[1] = 0.0
        if res:
            r[1] = 0.0
        if not rms:
            off = [2, rows - 1] if rows > 3 else [2]
            for i in off:
                x[i] = 30.0 + 0.5 * torch.randn(H, generator=g)
                if res:
                    r[i] = 0.0
    c = {"x": bfr(x), "res": bfr(r) if res else None, "w": bfr(1 + 0.1 * torch.randn(H, generator=g)),
         "b": bfr(0.1 * torch.randn(H, generator=g)) if bias else None,
         "dy": bfr(torch.randn(rows, H, generator=g)), "dres": bfr(torch.randn(rows, H, generator=g))}
    special = set(zero) | set(off)
    groups = {"bulk": torch.tensor([i for i in range(rows) if i not in special], dtype=torch.long),
              "zero": torch.tensor(zero, dtype=torch.long), "mean30": torch.tensor(off, dtype=torch.long)}
    assert sum(v.numel() for v in groups.values()) == rows
    if zero:
        assert (c["x"][1] == 0).all()
    for i in off:
        assert abs(c["x"][i].float().mean().item() - 30.0) < 1.0 and c["x"][i].float().std().item() < 1.0
    return c, groups


def stream(x, res):
    """The residual stream of the contract: s = bf16(x + r) by one fp32 add; x itself without r."""
    return x if res is None else (x.float() + res.float()).to(BF)


def norm64(x, res, w, b, eps, rms):
    """s = bf16(x + r); y = (s - mean) * rstd * w (+ b), rstd = 1 / sqrt(var + eps) with the two-pass
    variance mean((s - mean)^2); mean = 0 for RMSNorm."""
    s = d(stream(x, res))
    H = s.shape[-1]
    mean = torch.zeros(s.shape[0], dtype=F64) if rms else s.sum(-1) / H
    var = ((s - mean[:, None]) ** 2).sum(-1) / H
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (s - mean[:, None]) * rstd[:, None] * d(w)
    if b is not None:
        y = y + d(b)
    return {"s": s, "y": y, "rstd": rstd, "mean": mean}


def norm_fwd_depth(H, rows):
    """Longest chain of additions an element passes through in a forward row reduction: the wave
    kernel adds a lane's NC * 8 values in sequence, then 6 butterfly steps; the row kernel 8 values,
    6 steps, then up to 16 wave partials in sequence."""
    if rows < 512:
        return 8 + 6 + (H // 8 + 63) // 64
    return min(H, norm_fwd_nc(H) * 8) + 6


def norm_fwd_extra(ref, w, H, rows, groups, eps):
    """What the fp32 CPU branch lacks: the kernel's summation order and rsqrtf.
      mean: |dmean| <= depth U32 mean|s|.
      rstd: var is a sum of squares (all terms positive) -> relative error depth U32 (the two-pass
            form is second order in dmean: sum (d - dm)^2 = sum d^2 + H dm^2 as sum d = 0), so rstd
            moves by half of it relatively; the hardware rsqrt is good to 1 ulp (2 EPS32 taken).
      y:    |y - b| times the relative rstd term, plus rstd |w| dmean."""
    depth = norm_fwd_depth(H, rows)
    out = {"mean": {}, "rstd": {}, "y": {}}
    wmax = d(w).abs().max().item()
    for gname, rows_i in groups.items():
        if rows_i.numel() == 0:
            continue
        s, rstd, mean = ref["s"][rows_i], ref["rstd"][rows_i], ref["mean"][rows_i]
        dmean = depth * U32 * s.abs().mean(-1).max().item()
        rel = 0.5 * depth * U32 + 2 * EPS32
        out["mean"][gname] = dmean
        out["rstd"][gname] = rel * rstd.max().item()
        ycore = ((s - mean[:, None]) * rstd[:, None] * d(w)).abs().max().item()
        out["y"][gname] = ycore * rel + rstd.max().item() * wmax * dmean
    return out


def norm_bwd64(dy, s, w, rstd, mean, dres, eps, rms, has_bias):
    """Autograd on the fp64 forward formula with s as the leaf (ds, dw, db), dres added at the end.
    `rstd` / `mean` (the fp32 tensors handed to the kernel) must be the ones of s: asserted."""
    s64 = d(s).requires_grad_(True)
    w64 = d(w).requires_grad_(True)
    H = s64.shape[-1]
    mu = torch.zeros(s64.shape[0], 1, dtype=F64) if rms else s64.sum(-1, keepdim=True) / H
    rs = 1.0 / torch.sqrt(((s64 - mu) ** 2).sum(-1, keepdim=True) / H + eps)
    b64 = torch.zeros(H, dtype=F64, requires_grad=True)
    y = (s64 - mu) * rs * w64 + b64
    ds, dw, db = torch.autograd.grad(y, (s64, w64, b64), d(dy))
    assert torch.allclose(d(rstd), rs.detach().reshape(-1), rtol=1e-5, atol=0)
    if not rms:
        assert torch.allclose(d(mean), mu.detach().reshape(-1), rtol=1e-5, atol=1e-6)
    if dres is not None:
        ds = ds + d(dres)
    xh = ((s64 - mu) * rs).detach()
    out = {"ds": ds, "dw": dw}
    if has_bias:
        out["db"] = db
    return out, xh


def norm_bwd_depth(H, rows):
    """Row sums of the backward: NC * 8 per thread in sequence, 6 butterfly steps, 4 wave partials.
    Column sums (dw, db): ceil(rows / 768) rows in a block's registers, ceil(grid / 16) partial rows in
    stage 1, 16 in stage 2."""
    need = (H // 8 + 255) // 256
    nc = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else 16
    grid = min(rows, NORM_BWD_GRID)
    return min(H, nc * 8) + 6 + 4, (rows + grid - 1) // grid + (grid + K_SPLIT - 1) // K_SPLIT + K_SPLIT


def norm_bwd_extra(dy, w, xh, rstd64, H, rows, groups, rms):
    """Summation order only (the fp32 CPU branch has the same formula):
      ds = rstd (g - xh mean(g xh) - mean(g)), g = dy w: each mean is off by at most
           depth U32 mean|terms|, scaled by rstd |xh| and rstd;
      dw = sum_rows dy xh, db = sum_rows dy: depth_c U32 sum|terms|, largest column."""
    dr, dc = norm_bwd_depth(H, rows)
    g = d(dy) * d(w)
    out = {"ds": {}}
    for gname, rows_i in groups.items():
        if rows_i.numel() == 0:
            continue
        gi, xi, ri = g[rows_i], xh[rows_i], rstd64[rows_i]
        e = dr * U32 * ((gi * xi).abs().mean(-1) * xi.abs().max(-1).values + (0.0 if rms else 1.0) * gi.abs().mean(-1))
        out["ds"][gname] = (ri * e).max().item()
    out["dw"] = dc * U32 * (d(dy) * xh).abs().sum(0).max().item()
    out["db"] = dc * U32 * d(dy).abs().sum(0).max().item()
    return out


# ================================================================================== activations
# grid_for caps the grid at 2048 blocks of 256 threads x 8 columns: (2049, 2048) is one block past it
ACT_SHAPES = [(1, 8), (257, 24), (13, 192), (2049, 2048)]
GELU_NUMEL = [8, 2056, 2049 * 2048]
PLANTED = [0.0, 1e-3, -1e-3, 8.0, -8.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]  # as bf16 (only 1e-3 rounds)


def swiglu_case(rows, F, seed=0):
    """gu [rows, 2F], dy [rows, F] bf16. Gate column 0 carries the planted values (cycled over the
    rows; with one row they take the row's first columns when they fit)."""
    g = gen(21000 + rows + 7 * F + seed)
    gu = torch.randn(rows, 2 * F, generator=g)
    pl = torch.tensor(PLANTED)
    planted = torch.zeros(rows, F, dtype=torch.bool)
    if rows >= len(PLANTED):
        gu[:, 0] = pl[torch.arange(rows) % len(PLANTED)]
        planted[:, 0] = True
    else:
        n = min(F, len(PLANTED))
        gu[0, :n] = pl[:n]
        planted[0, :n] = True
    gu = bfr(gu)
    assert set(gu[:, :F][planted].float().tolist()) <= set(bfr(pl).float().tolist())
    return {"gu": gu, "dy": bfr(torch.randn(rows, F, generator=g))}, planted


def swiglu64(gu, dy):
    """out = silu(g) u; dg = dy u s (1 + g (1 - s)), du = dy g s, s = sigmoid(g); dgu = [dg | du]."""
    gu64, dy64 = d(gu), d(dy)
    F_ = gu64.shape[-1] // 2
    g, u = gu64[..., :F_], gu64[..., F_:]
    s = torch.sigmoid(g)
    return {"out": g * s * u, "dgu": torch.cat([dy64 * u * s * (1 + g * (1 - s)), dy64 * g * s], -1)}


def swiglu_extra(gu, dy, sel):
    """sigmoidf_ = 1 / (1 + __expf(-g)). __expf(x) = exp2(x log2 e): the product is rounded once
    (|x| U32 relative in the result) and the hardware exp2 is good to 1 ulp, so exp(-g) is off by
    (|g| + 2) EPS32 relatively and s by s (1 - s) (|g| + 2) EPS32 <= 0.6 EPS32 absolutely (the
    maximum of s (1 - s) (|g| + 2) is 0.56, near |g| = 1). Where __expf overflows (g <= -89) s is
    0 against a true value below 2^-126, far under the floor term.
      out: |g u| ds;  du: |dy g| ds;  dg: |d/ds| = |dy u (1 + g - 2 g s)| <= |dy u| (1 + |g|)."""
    gu64, dy64 = d(gu), d(dy)
    F_ = gu64.shape[-1] // 2
    g, u = gu64[..., :F_][sel], gu64[..., F_:][sel]
    dy64 = dy64[sel]
    ds = 0.6 * EPS32
    return {"out": ((g * u).abs().max() * ds).item(),
            "dgu": (torch.maximum((dy64 * u).abs() * (1 + g.abs()), (dy64 * g).abs()).max() * ds).item()}


def gelu_case(numel, seed=0):
    g = gen(22000 + (numel % 9973) + seed)
    x = torch.randn(numel, generator=g)
    n = min(numel, len(PLANTED))
    idx = torch.arange(n) * (numel // n) if numel >= 8 * n else torch.arange(n)
    x[idx] = torch.tensor(PLANTED)[:n]
    planted = torch.zeros(numel, dtype=torch.bool)
    planted[idx] = True
    return {"x": bfr(x), "dy": bfr(torch.randn(numel, generator=g))}, planted


_K0, _K1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu_new64(x, dy):
    """y = 0.5 x (1 + tanh(k0 (x + k1 x^3))); dx = dy dy/dx by autograd."""
    x64 = d(x).requires_grad_(True)
    y = 0.5 * x64 * (1 + torch.tanh(_K0 * (x64 + _K1 * x64 ** 3)))
    (dx,) = torch.autograd.grad(y, x64, d(dy))
    return {"y": y.detach(), "dx": dx}


def gelu_extra(x, dy, sel):
    """tanhf of the device library against the CPU's: 2 ulp taken, dt = 2 EPS32 (t <= 1).
      y:  0.5 |x| dt.
      dx: 0.5 (1 + t) + 0.5 x (1 - t^2) k0 (1 + 3 k1 x^2): 0.5 dt from the first term; 1 - t^2 moves
          by 2 dt, but only where t is not +-1 in fp32 (1 - |t| > 2^-26; beyond, both tanh give
          exactly +-1 and 1 - t^2 is exactly 0)."""
    x64, dy64 = d(x)[sel], d(dy)[sel]
    t = torch.tanh(_K0 * (x64 + _K1 * x64 ** 3))
    dt = 2 * EPS32
    live = ((1 - t.abs()) > 2.0 ** -26).double()
    der = 0.5 * dt + live * 2 * dt * 0.5 * x64.abs() * _K0 * (1 + 3 * _K1 * x64 ** 2)
    return {"y": (0.5 * x64.abs().max() * dt).item(), "dx": (dy64.abs() * der).max().item()}


# ========================================================================================= RoPE
# rope_grid caps at 2048 blocks x 256 items; an item is one rotary pair of 8-column chunks or one
# pass-through chunk: tokens * heads * (D / 8 - rot / 16) items.
ROPE_DROT = [(128, 128), (64, 64), (128, 64), (80, 32)]
ROPE_HEADS = [(4, 2), (0, 2), (3, 1)]
ROPE_BIG = dict(tokens=1032, Hq=48, Hkv=16, D=128, rot=128)  # 1032 * 64 * 8 = 528384 > 2048 * 256
ROPE_MAXPOS = 96


def rope_tables(rot, max_pos=ROPE_MAXPOS, theta=10000.0):
    """fp32 [max_pos, rot / 2] tables of the documented form (angle p * theta^(-2i / rot) in fp64,
    rounded once). The tests hand the SAME tables to the kernel: this pins the kernel, not the table."""
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=F64) / rot))
    fr = torch.outer(torch.arange(max_pos, dtype=F64), inv)
    return fr.cos().float(), fr.sin().float()


def rope_positions(kind, B, T, max_pos=ROPE_MAXPOS):
    """-> (pos tensor for the kernel or None, pos_offset, long [B * T] positions for the reference)."""
    t = torch.arange(T).repeat(B)
    if kind == "off0":
        return None, 0, t
    if kind == "off37":
        assert T + 37 <= max_pos
        return None, 37, t + 37
    g = gen(23000 + B * T)
    p = torch.randint(0, max_pos, (B * T,), generator=g)
    p[0], p[-1] = max_pos - 1, 0  # reaches the table's last row; non-monotone
    assert p.max().item() == max_pos - 1 and (p[1:] < p[:-1]).any() and (p[1:] > p[:-1]).any()
    return p.to(torch.int32), 0, p.long()


def rope_case(tokens, Hq, Hkv, D, slack=8, pad=16, seed=0):
    """A fused qkv buffer wider than (Hq + 2 Hkv) D (`slack` extra columns) inside rows of stride
    width + pad, and rotated-space gradients dq, dk."""
    g = gen(24000 + tokens + Hq * 131 + D + seed)
    W = (Hq + 2 * Hkv) * D + slack
    buf = bfr(torch.randn(tokens, W + pad, generator=g))
    return {"buf": buf, "W": W, "dq": bfr(torch.randn(tokens, Hq * D, generator=g)),
            "dk": bfr(torch.randn(tokens, Hkv * D, generator=g))}


def rope64(src, cos, sin, pos, rot, bwd=False):
    """src [tokens, heads, D]; rotate-half over the first `rot` dims with the fp32 tables' rows
    `pos`: (a, b) -> (a c - b s, b c + a s); the backward is the transpose (a c + b s, b c - a s).
    Columns >= rot pass through."""
    x = d(src)
    half = rot // 2
    c, s = d(cos)[pos][:, None, :], d(sin)[pos][:, None, :]
    if bwd:
        s = -s
    a, b = x[..., :half], x[..., half:rot]
    return {"out": torch.cat([a * c - b * s, b * c + a * s, x[..., rot:]], -1)}


def rope_extra(src):
    """a c - b s may be contracted to one fma in the kernel and not in the CPU branch: the two
    differ by one rounding of a product, <= EPS32 max|x| (|c|, |s| <= 1); 2 taken for both lines."""
    return 2 * EPS32 * d(src).abs().max().item()


# ==================================================================================== embedding
EMB_CHUNK = 16  # kEmbChunk: sorted positions per backward wave
EMB_H = [8, 136, 512, 520, 4096]
EMB_V = 64
# (layout, H, gradient dtype): the edge layouts at every H, the single-run sizes at one H
EMB_CASES = ([(k, H, dt) for k in ("edges", "edges_oob") for H in EMB_H for dt in (torch.float32, torch.bfloat16)]
             + [(k, 136, dt) for k in ("one1", "one15", "one16", "one17", "last_whole")
                for dt in (torch.float32, torch.bfloat16)])


def emb_layout(kind, V=EMB_V):
    """Sorted ids as a list of (id, run length) and the facts the builder asserts about it.
    "edges": out of a run's position relative to the 16-position chunks follows which kernel path
    sums it -- whole in pass 1, pieces to scratch, fold in pass 2."""
    if kind == "edges" or kind == "edges_oob":
        runs = [(1, 3)]  # starts at p = 0
        runs += [(2 + i, 1) for i in range(13)]  # singletons up to p = 16
        runs += [(15, 16)]  # [16, 32): a run of 16 on a chunk boundary, whole in one chunk
        runs += [(16 + i, 1) for i in range(8)]  # up to p = 40
        runs += [(24, 16)]  # [40, 56): a run of 16 at offset 8: crosses one boundary
        runs += [(25 + i, 1) for i in range(8)]  # up to p = 64
        runs += [(33, 33)]  # [64, 97): crosses two boundaries, last piece of length 1
        runs += [(34 + i, 1) for i in range(9)]  # up to p = 106
        runs += [(43, 150)]  # a long run: ten chunk boundaries
        runs += [(44, 20)]  # ends at N, crosses a boundary
        if kind == "edges_oob":
            runs = [(-7, 2), (-1, 19)] + runs + [(V, 18), (V + 300, 1)]  # out-of-range runs, both ends
    elif kind.startswith("one"):  # a single run of N positions: starts at 0 and ends at N
        runs = [(5, int(kind[3:]))]
    elif kind == "last_whole":  # the last run lies inside one chunk and ends at N
        runs = [(3, 16), (9, 5)]
    else:
        raise ValueError(kind)
    sid = torch.tensor([i for i, n in runs for _ in range(n)], dtype=torch.int64)
    assert (sid[1:] >= sid[:-1]).all()
    return sid, runs


def emb_crossings(runs):
    """Per run: (start, end, number of chunk boundaries strictly inside it)."""
    out, p = [], 0
    for _, n in runs:
        out.append((p, p + n, (p + n - 1) // EMB_CHUNK - p // EMB_CHUNK))
        p += n
    return out


def emb_case(kind, H, gdtype, V=EMB_V, seed=0):
    sid, runs = emb_layout(kind, V)
    N = sid.numel()
    g = gen(25000 + N + H + seed)
    perm = torch.randperm(N, generator=g)
    dy = bfr(torch.randn(N, H, generator=g))
    base = torch.randn(V, H, generator=g).to(gdtype)
    return {"sid": sid, "perm": perm, "dy": dy, "base": base, "V": V, "runs": runs}


def embed_bwd64(sid, perm, dy, base, V):
    """grad[sid[j]] += dy[perm[j]] for every j with 0 <= sid[j] < V, onto `base`."""
    ok = (sid >= 0) & (sid < V)
    grad = d(base).clone()
    grad.index_add_(0, sid[ok], d(dy)[perm[ok]])
    return {"grad": grad}


def embed_extra(sid, perm, dy, base, V):
    """fp32 sequential summation over the run (pieces of at most 16, then the pieces): every term
    passes through at most n - 1 additions, n the longest run: (n - 1) U32 sum|dy| of the run, plus
    one rounding of the add into the gradient row, U32 max|grad|. (bf16 gradients: the bf16 ulp of
    the final rounding is `check`'s bf16 term.)"""
    ok = (sid >= 0) & (sid < V)
    if not ok.any():
        return 0.0
    absum = torch.zeros(V, dy.shape[1], dtype=F64)
    absum.index_add_(0, sid[ok], d(dy)[perm[ok]].abs())
    n = torch.bincount(sid[ok], minlength=V).max().item()
    total = (d(base).abs() + absum).max().item()
    return (n - 1) * U32 * absum.max().item() + U32 * total


# ================================================================================== reward head
RH_H = [8, 136, 2048, 2056, 4096]  # > 2048: a second trip of the 256 x 8 column loop
RH_T = [1, 96, 300]  # > 256: a second trip of the mask-count loop
# (H, T, dropout p, bias, strided hidden), each with both poolings
RH_CASES = [(8, 1, 0.0, True, False), (136, 96, 0.5, False, True), (2048, 300, 0.5, True, True),
            (2056, 96, 0.0, False, False), (4096, 300, 0.5, True, True), (2056, 300, 0.5, False, False)]
_M64 = (1 << 64) - 1


def rh_keep64(seed, B, H, p):
    """The keep mask of rh_keep on the CPU, in exact integer arithmetic modulo 2^64:
    z = seed + 0x9E3779B97F4A7C15 (row * 0x100000001B3 + col + 1); two xor-shift-multiply rounds
    (30 / 0xBF58476D1CE4E5B9, 27 / 0x94D049BB133111EB), z ^= z >> 31; u = (z >> 40) / 2^24 >= p.
    p is the fp32 value of the argument, u an exact fp32 value, so the comparison is exact."""
    if p <= 0:
        return torch.ones(B, H, dtype=torch.bool)
    pf = float(torch.tensor(p, dtype=torch.float32))
    keep = torch.empty(B, H, dtype=torch.bool)
    for r in range(B):
        for c in range(H):
            z = (seed + 0x9E3779B97F4A7C15 * ((r * 0x100000001B3 + c + 1) & _M64)) & _M64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
            z ^= z >> 31
            keep[r, c] = (z >> 40) / 16777216.0 >= pf
    return keep


def rh_case(B, T, H, pooling, seed=0, pad=8):
    """hidden as a strided view (stride(1) = H + pad) and contiguous; `last` or `mask`; w, bias,
    dscore. Mean pooling: row 0 right-padded, row 1 all-zero mask (count clamps to 1), row 2
    left-padded, the others full (rows beyond B dropped)."""
    g = gen(26000 + 17 * T + H + seed)
    buf = bfr(torch.randn(B, T, H + pad, generator=g))
    hidden = buf[:, :, :H]
    assert hidden.stride(1) == H + pad or T == 1
    w = bfr(torch.randn(H, generator=g) / math.sqrt(H))
    bias = bfr(torch.randn(1, generator=g))
    ds = torch.randn(B, generator=g)
    mask = torch.ones(B, T)
    k = max(1, (2 * T) // 3)
    mask[0, k:] = 0.0
    if B > 1:
        mask[1] = 0.0
    if B > 2:
        mask[2, :T - k] = 0.0
    last = torch.randint(0, T, (B,), generator=g).to(torch.int32)
    last[0] = T - 1
    if B > 1:
        last[1] = 0
    c = {"hidden": hidden, "w": w, "bias": bias, "ds": ds}
    if pooling == "mean":
        c["mask"], c["last"] = mask, None
        assert B < 2 or mask[1].sum() == 0
    else:
        c["mask"], c["last"] = None, last
    return c


def reward_head64(hidden, last, mask, w, bias, p, seed, ds=None):
    """pooled = hidden[b, last[b]] or bf16(sum_t m h / max(count, 1)), then keep / (1 - p);
    score = <pooled, w> + bias; dhidden = ds w keep / (1 - p) at the pooled position, times
    m / count at every valid position for mean pooling, 0 elsewhere.
    "flip": sum_j |w_j| ulp_bf16(pooled_j) / (1 - p) over the elements whose unrounded mean lies
    within T U32 |v| (the fp32 sum's own error) of a bf16 rounding tie: there the kernel may
    legitimately round to the other neighbour, which moves the score by that much."""
    h, w64 = d(hidden), d(w)
    B, T, H = h.shape
    keep = rh_keep64(seed, B, H, p)
    scale = 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32))) if p > 0 else 1.0
    flip = torch.zeros(B, H, dtype=F64)
    if mask is not None:
        m = d(mask)
        cnt = m.sum(1).clamp(min=1)
        raw = (h * m[:, :, None]).sum(1) / cnt[:, None]
        pooled = raw.to(BF).to(F64)  # fp64 -> fp32 -> bf16: the first rounding moves 2^-24, see `flip`
        ulp = R.bf16_ulp(raw)
        frac = (raw.abs() / ulp) % 1.0  # distance to the tie at .5
        near = (frac - 0.5).abs() * ulp <= (T + 2) * U32 * raw.abs()
        flip = torch.where(near, ulp, torch.zeros_like(ulp))
        route = m / cnt[:, None]
    else:
        idx = last.long()
        pooled = h[torch.arange(B), idx]
        route = torch.zeros(B, T, dtype=F64)
        route[torch.arange(B), idx] = 1.0
    kd = keep.double() * scale
    pooled = pooled * kd
    flip = flip * kd
    score = (pooled * w64).sum(1) + (d(bias)[0] if bias is not None else 0.0)
    out = {"score": score, "pooled": pooled, "keep": keep, "flip": flip, "score_flip": (flip * w64.abs()).sum(1)}
    if ds is not None:
        gcol = d(ds)[:, None] * w64 * kd  # [B, H]
        out["dhidden"] = route[:, :, None] * gcol[:, None, :]
        out["route"] = route
        out["dw"] = (d(ds)[:, None] * pooled).sum(0)
        out["dw_flip"] = (d(ds).abs()[:, None] * flip).sum(0)
    return out


def rh_extra(hidden, mask, w, ref):
    """Summation order of the fp32 dot over H: 8 columns per thread per trip in sequence, ceil(H /
    2048) trips, 6 butterfly steps, 4 wave partials: depth U32 sum|pooled w|."""
    H = hidden.shape[-1]
    depth = 8 * ((H + 2047) // 2048) + 6 + 4
    return depth * U32 * (ref["pooled"] * d(w)).abs().sum(1).max().item()


# ==================================================================================== transpose
# R % 8 or C % 8 nonzero -> transpose_bf16_kernel (LDS tile, partial tiles, scalar tails); both row
# strides multiples of 8 as the binding requires
TRANSPOSE_LDS = [(13, 72), (72, 13), (65, 129), (1, 8), (8, 1)]
