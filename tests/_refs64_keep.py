"""fp64 references for the kept-set ("keep sampling mask") LM-head row kernels, wrappers and sampler
(test_keep_mask_cpu.py, test_keep_mask_gpu.py).

With K the kept set of a row, i = inv_temp and z the bf16 logits:

    lse_K = logsumexp_{v in K} i z_v      logp = i z_t - lse_K   (-inf for t outside K)
    dz_v  = i g (1[v = t] - p_v), p_v = exp(i z_v - lse_K), for v in K;  exactly 0 outside K

which is `_refs64_temp.rows64` / `bwd64` over the kept entries: a dropped entry is a -inf logit there
(p = 0, adds exactly 0, receives exactly 0). Nothing here imports the package's ops; the bit packing
is written out again so that the package's `pack_keep` is tested against it.

`rows32` / `bwd32` are the fp32 CPU formula of record,
log_softmax((logits.float() * i).masked_fill(~kept, -inf)): the E32 of the `_refs64` bound.
"""
import torch

import _refs64 as R
import _refs64_temp as RT

PATTERNS = ["half", "top37", "one", "edges", "ones"]


def masked(x, kept):
    """x with the entries outside `kept` (bool, same shape) at -inf."""
    return x.masked_fill(~kept, R.NINF)


def rows64(x, tgt, it, kept):
    return RT.rows64(masked(x, kept), tgt, it)


def rows32(x, tgt, it, kept):
    return RT.rows32(masked(x, kept), tgt, it)


def bwd64(x, tgt, g, it, kept):
    return RT.bwd64(masked(x, kept), tgt, g, None, it)


def bwd32(x, tgt, g, it, kept):
    return RT.bwd32(masked(x, kept), tgt, g, None, it)


def pack(mask):
    """bool [M, V] -> uint8 [M, V / 8]: bit j (LSB first) of byte i = entry 8 i + j."""
    M, V = mask.shape
    assert V % 8 == 0
    out = torch.zeros(M, V // 8, dtype=torch.int64)
    for j in range(8):
        out |= mask[:, j::8].to(torch.int64) << j
    return out.to(torch.uint8)


def unpack(keep):
    cols = [((keep.to(torch.int64) >> j) & 1).bool() for j in range(8)]
    return torch.stack(cols, -1).reshape(keep.shape[0], keep.shape[1] * 8)


def mask_rows(pattern, x, seed=0):
    """One mask row per logits row of x [N, V] (bool [N, V]); every row keeps at least one entry."""
    N, V = x.shape
    g = R.gen(777 + seed)
    m = torch.zeros(N, V, dtype=torch.bool)
    if pattern == "half":
        m = torch.rand(N, V, generator=g) < 0.5
    elif pattern == "top37":
        m.scatter_(1, x.float().topk(min(37, V), dim=-1).indices, True)
    elif pattern == "one":
        m[torch.arange(N), torch.randint(0, V, (N,), generator=g)] = True
    elif pattern == "edges":  # bit 7 of byte 0 and bit 0 of the last byte
        m[:, 7] = True
        m[:, V - 8] = True
    elif pattern == "ones":
        m[:] = True
    else:
        raise ValueError(pattern)
    return m


def keep_rows_for(N):
    """int64 [N]: mask row of every logits row. N - 2 mask rows in a scrambled order, one logits row
    without a mask (-1) and two logits rows on one mask row, so indexing the mask by the logits row
    shows. Returns (keep_rows, M)."""
    assert N >= 5
    M = N - 2
    perm = torch.randperm(M, generator=R.gen(4242)).tolist()
    kr = perm + [perm[0], -1]  # row N - 2 shares row 0's mask row, row N - 1 has none
    if kr[:M] == list(range(M)):  # never the identity
        kr[0], kr[1] = kr[1], kr[0]
        kr[N - 2] = kr[0]
    return torch.tensor(kr, dtype=torch.int64), M


def case(pattern, x, seed=0):
    """For logits x [N, V]: (mask bool [M, V], keep_rows int64 [N], kept bool [N, V] = the set of
    every logits row (all True on the -1 row), tgt int64 [N]). Targets lie inside the kept set (the
    kept entry with the largest logit), except row 3 (ignored, -100) and, where the set leaves room,
    row 5, whose target is a dropped entry (logp = -inf, its gradient row is -g p)."""
    N, V = x.shape
    kr, M = keep_rows_for(N)
    own = mask_rows(pattern, x, seed)  # built per logits row, then filed under that row's mask row
    mask = torch.zeros(M, V, dtype=torch.bool)
    for r in range(N):
        if kr[r] >= 0 and r != N - 2:
            mask[kr[r]] = own[r]
    kept = torch.where((kr >= 0).unsqueeze(-1), mask[kr.clamp(min=0)], torch.ones(N, V, dtype=torch.bool))
    tgt = masked(x.float(), kept).argmax(-1)
    tgt[3] = -100
    if not bool(kept[5].all()):
        tgt[5] = int((~kept[5]).nonzero()[0])
    return mask, kr, kept, tgt
