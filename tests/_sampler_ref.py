"""Exact fp64 inverse-CDF oracle of the fused sampler (csrc/sampling.hip), shared by
test_sampler_ref_cpu.py and test_sampler_gpu.py. It imports none of the package's ops and works on
CPU or GPU tensors.

For given (logits, T, top_k, top_p, seed, row, counter) the sampler is a deterministic lookup: the
token whose interval of the kept set's CDF (index order) holds u = Philox4x32-10(key = seed,
ctr = (row, counter)). This module reproduces every piece off the device:

  z      fp32((x - rowmax) * fp32(1 / T)), bit for bit (a subtraction and a multiplication cannot be
         contracted into an FMA), widened to fp64. Only z >= -64 counts.
  kept   HF order, temperature -> top-k -> top-p on the renormalised top-k mass. Top-k keeps
         z >= (k-th largest z), ties kept, inactive for k <= 0 or k >= V, and with fewer than k
         values in the window all of them. Top-p keeps a token iff the mass strictly above it is
         < p * total.
  u      (c0 >> 8) * 2^-24 of Philox4x32-10 with counter words (row_lo, row_hi, ctr_lo, ctr_hi)
         and key (seed_lo, seed_hi) of the int64 seed reinterpreted as uint64.

The kernel pins its thresholds to one fine histogram bin and compares masses in fp32, so two sets
come back per row: K_min, the exact set, and K_max, everything within DELTA in z below either
edge, down to the alternative edge where p * total is met within EPS_M. A row whose two sets
differ (or whose edge could also move up within EPS_M) is AMBIGUOUS and gets only the weak check
`token in K_max`; every other row gets the draw check F[t-1] - EPS_U <= u < F[t] + EPS_U with
F = cumsum(exp(z) over K_min, index order) / sum.

EPS_U = 2^-15 is a worst case, derived: fp32 accumulation chains of at most 128 elements per thread
segment at V = 128256, 10 scan levels and 32 chunk adds stay below 2^-16.6 relative; __expf is
exp2(z * log2e), whose argument rounding is <= 23 * 2^-24 for z >= -16, and tokens below -16
carry <= 1.4 % of the mass; v_exp adds 1 ulp and u * total one rounding; all of it on numerator
and denominator: < 2^-15. The typical error is about 1e-6.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

RANGE = 64.0
BINS = 2048
DELTA = 2 * RANGE / BINS ** 2  # one fine bin + the fp32 rounding of z + 64
EPS_M = 2.0 ** -16             # relative, fp32 mass comparisons
EPS_U = 2.0 ** -15
M32 = 0xFFFFFFFF
NEG_INF = float("-inf")


# The grid test_sampler_gpu.py runs and test_sampler_ref_cpu.py checks the ambiguity cap on. The
# cap is a condition on the inputs, evaluated with this reference alone: about 1 row in 100 has a
# nucleus boundary within EPS_M of p by chance, and the builder seed is one for which no case of
# the grid goes past 2 rows in 64.
ROWS, COUNTERS, GRID_SEED = 64, tuple(range(8)), 1
VOCABS = (4099, 32760, 32768, 32776, 50264, 128256, 50257)
DTYPES = (torch.bfloat16, torch.float32)
TEMPS = (0.7, 1.3)
# (builder, top_k, top_p); never `dense` with top-p alone: at T >= 1 its nucleus holds thousands
# of near-equal tokens and most rows are ambiguous
MODES = (("dense", 0, 1.0), ("dense", 50, 1.0), ("peaked", 0, 0.9), ("peaked", 50, 0.9),
         ("peaked", 0, 0.5), ("peaked", 0, 0.99), ("peaked", 20, 1.0))
AMBIGUOUS_CAP = 0.05


def mode_id(mode) -> str:
    return f"{mode[0]}-k{mode[1]}-p{mode[2]}"


def grid_logits(builder: str, V: int, dtype: torch.dtype, B: int = ROWS) -> torch.Tensor:
    """The grid's logits (CPU), cast to the logits dtype before anything sees them."""
    fn = {"dense": dense, "peaked": peaked}[builder]
    return fn(B, V, GRID_SEED + V).to(dtype)


# ------------------------------------------------------------------------------------ Philox
def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr 4 words, key 2 words -> 4 output words (pure-Python integers)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _u64(x: int) -> int:
    return int(x) & 0xFFFFFFFFFFFFFFFF  # int64 reinterpreted as uint64


def philox_words(seed: int, row: int, counter: int):
    s, r, c = _u64(seed), _u64(row), _u64(counter)
    return philox4x32_10((r & M32, r >> 32, c & M32, c >> 32), (s & M32, s >> 32))


def philox_u01(seed: int, row: int, counter: int) -> float:
    """The sampler's uniform for (seed, row, counter): (c0 >> 8) * 2^-24, exact in a double."""
    return (philox_words(seed, row, counter)[0] >> 8) * 2.0 ** -24


def u_grid(seed: int, rows: int, counters, device="cpu") -> torch.Tensor:
    """[rows, len(counters)] fp64 uniforms."""
    return torch.tensor([[philox_u01(seed, r, c) for c in counters] for r in range(rows)],
                        dtype=torch.float64, device=device)


# ------------------------------------------------------------------------------------ builders
def dense(B: int, V: int, seed: int) -> torch.Tensor:
    """randn * 3: every token inside the window, every segment and chunk boundary carries mass."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, V, generator=g) * 3.0


def peaked(B: int, V: int, seed: int, H: int = 64) -> torch.Tensor:
    """A randn - 20 tail under H well-separated head tokens, 6 - cumsum(U(0.125, 0.5)), at random
    positions: any top-p edge falls between two head tokens."""
    g = torch.Generator().manual_seed(seed)
    H = min(H, V)
    x = torch.randn(B, V, generator=g) - 20.0
    pos = torch.rand(B, V, generator=g).topk(H, dim=-1).indices
    head = 6.0 - (0.125 + 0.375 * torch.rand(B, H, generator=g)).cumsum(-1)
    return x.scatter_(1, pos, head)


# ------------------------------------------------------------------------------------ kept sets
class Kept(NamedTuple):
    z: torch.Tensor          # [B, V] fp64, the kernel's fp32 z widened (NaN where it is NaN)
    kmin: torch.Tensor       # [B, V] bool, the exact kept set
    kmax: torch.Tensor       # [B, V] bool, the widest set the kernel's resolution allows
    ambiguous: torch.Tensor  # [B] bool
    F: torch.Tensor          # [B, V] fp64 inclusive CDF of exp(z) over kmin, index order
    Fex: torch.Tensor        # [B, V] fp64 exclusive CDF


def z_scores(logits: torch.Tensor, T: float) -> torch.Tensor:
    x = logits.float()
    gmax = torch.where(torch.isnan(x), torch.full_like(x, NEG_INF), x).max(-1, keepdim=True).values
    inv_t = torch.tensor(1.0 / float(T), dtype=torch.float64).to(torch.float32).to(x.device)
    d = x - gmax           # one fp32 rounding
    return (d * inv_t).double()  # a second one


def _p_edge(sz, w, run_start, target):
    """Sorted-descending z `sz`, masses `w` (0 outside the candidate set, a prefix) and the
    first index of each run of ties: the smallest kept z per row (+inf when nothing is kept),
    a token being kept iff the mass strictly above it is < target."""
    before = (w.cumsum(-1) - w).gather(1, run_start)
    keep = (before < target) & (w > 0)
    n = keep.sum(-1, keepdim=True)
    edge = sz.gather(1, (n - 1).clamp_(min=0))
    return torch.where(n > 0, edge, torch.full_like(edge, float("inf")))


def kept_sets(logits: torch.Tensor, T: float, top_k: int, top_p: float) -> Kept:
    B, V = logits.shape
    z = z_scores(logits, T)
    window = z >= -RANGE  # NaN compares false
    need_k = 0 < top_k < V
    p32 = float(torch.tensor(float(top_p), dtype=torch.float32))  # the binding's float(top_p)
    need_p = p32 < 1.0
    lo = torch.full((B, 1), -RANGE, dtype=torch.float64, device=z.device)
    f_exact, f_lo, f_hi = lo, lo, lo
    if need_k or need_p:
        sz, _ = torch.where(window, z, torch.full_like(z, NEG_INF)).sort(-1, descending=True)
        kth = sz[:, top_k - 1:top_k] if need_k else lo
        kth = torch.maximum(kth, lo)  # fewer than k values in the window: all of them
        f_exact = kth
        f_lo, f_hi = (kth - DELTA, kth) if need_k else (lo, lo)
    if need_p:
        idx = torch.arange(V, device=z.device).expand(B, V)
        new_run = torch.ones_like(sz, dtype=torch.bool)
        new_run[:, 1:] = sz[:, 1:] != sz[:, :-1]
        run_start = torch.where(new_run, idx, torch.zeros_like(idx)).cummax(-1).values
        edges = []
        for floor, ps in ((kth, (p32, p32 * (1 + EPS_M), p32 * (1 - EPS_M))),
                          (f_lo, (p32 * (1 + EPS_M), p32 * (1 - EPS_M)))):
            w = torch.where((sz >= floor) & (sz > NEG_INF), sz.exp(), torch.zeros_like(sz))
            total = w.sum(-1, keepdim=True)
            edges += [torch.maximum(floor, _p_edge(sz, w, run_start, p * total)) for p in ps]
            if not need_k:
                break
        f_exact = edges[0]
        f_lo = torch.stack(edges).min(0).values - DELTA
        f_hi = torch.stack(edges).max(0).values
    kmin = window & (z >= f_exact)
    kmax = window & (z >= f_lo)
    ambiguous = (kmin != kmax).any(-1) | (f_hi > f_exact).squeeze(-1)
    return Kept(z, kmin, kmax, ambiguous, *cdf(z, kmin))


def cdf(z: torch.Tensor, mask: torch.Tensor):
    """Inclusive and exclusive CDF of exp(z) over `mask`, index order."""
    w = torch.where(mask, z.exp(), torch.zeros_like(z))
    cum = w.cumsum(-1)
    total = cum[:, -1:].clamp(min=1e-300)
    return cum / total, (cum - w) / total


def exact_tokens(kept: Kept, u: torch.Tensor) -> torch.Tensor:
    """Inverse CDF of the exact kept set: [B, C] uniforms -> [B, C] tokens."""
    last = (kept.kmin * torch.arange(1, kept.kmin.shape[1] + 1, device=u.device)).max(-1, keepdim=True).values - 1
    t = torch.searchsorted(kept.F, u.contiguous(), right=True)
    return torch.minimum(t, last.clamp(min=0))


class Check(NamedTuple):
    worst_excess: float   # max(F[t-1] - u, u - F[t], 0) over the unambiguous rows' draws
    needed: int           # draws that needed any of EPS_U
    ambiguous_share: float
    ok: torch.Tensor      # [B, C] bool: the draw passes (weak check on ambiguous rows)


def check_draws(kept: Kept, tokens: torch.Tensor, u: torch.Tensor) -> Check:
    """tokens [B, C] int64 drawn at uniforms u [B, C] (fp64) from the rows of `kept`."""
    V = kept.z.shape[1]
    inside = (tokens >= 0) & (tokens < V)
    t = tokens.clamp(0, V - 1)
    in_min, in_max = kept.kmin.gather(1, t) & inside, kept.kmax.gather(1, t) & inside
    lo, hi = kept.Fex.gather(1, t), kept.F.gather(1, t)
    strong = in_min & (lo - EPS_U <= u) & (u < hi + EPS_U)
    amb = kept.ambiguous[:, None].expand_as(t)
    ok = torch.where(amb, in_max, strong)
    excess = torch.maximum(lo - u, u - hi).clamp(min=0)
    judged = ~amb & in_min
    worst = float(excess[judged].max()) if bool(judged.any()) else 0.0
    needed = int((judged & ((u < lo) | (u >= hi))).sum())
    return Check(worst, needed, float(kept.ambiguous.double().mean()), ok)
