"""The memory-bound block kernels (csrc/norm.hip, elementwise.hip, rope.hip, embedding.hip,
reward_head.hip, transpose.hip) against the fp64 references and derived bounds of
_refs64_block.py, at the shapes that sit on each launcher's dispatch edges.

Every case
  * launches twice and requires bitwise equal outputs (none of these files uses float atomics);
  * first makes the scratch a launcher takes with at::empty visibly stale (the norm dw / db partial
    rows with their kSplit stage-1 rows, the embedding scratch slab): tensors of those sizes are
    NaN-filled and freed, best effort as in test_attention_fp64_gpu.py;
  * checks EVERY element of every output with `_refs64.check` (the share left out is zero) and
    prints the figures; exact contracts (the residual stream s, the embedding gather, the keep
    mask, zeros off the pooled positions, untouched guard columns, the transposes) are bit-equal.
  bf16 outputs pass `_refs64.check` with its whole bf16 ulp and then the half-ulp form of
  `_refs64_block.check`; the figures below are of the half-ulp form.
test_block_refs_cpu.py shows on the CPU that the same check and bounds reject thirteen planted
defects of the kinds these kernels can have.

Measured on an MI355X, worst error / bound over all cases and row groups (the bounds are worst-case
summation bounds, so a correct kernel sits far inside them; the planted defects sit 10x to 1e6x
outside):
    norm_fwd_row    y 0.015  rstd 0.057  mean 0.017
    norm_fwd_wave   y 0.016  rstd 0.171  mean 0.014
    norm_bwd        ds 0.013  dw 0.009  db 0.000
    add_norm        y 0.007  dx 0.014  dw 0.004  db 0.000
    swiglu          out 0.007  dgu 0.005
    gelu_new        y 0.012  dx 0.030
    rope_fwd        qk 0.011        rope_bwd  dqk 0.010
    embed_bwd       grad 0.035      embedding grad: dense 0.000, main-grad fp32 0.001, bf16 0.000
    reward_head     score 0.010  pooled 0.000 (whole ulp)  dhidden 0.000  dw 0.000
(0.000: every element within half a bf16 ulp of the reference, nothing left for the fp32 bound.)
The exact contracts held bit for bit, and two launches always agreed.
Cross-check on the GPU: a build whose wgrad stage 2 folded 15 of the 16 splits failed 13 of the 18
norm backward and add_norm cases; the 5 that passed (1, 5 and 37 rows) have no partial row in split 15.

Found: RMSNorm with a bias was silently wrong on the GPU (the launchers pick HAS_BIAS = false for
rms, so the forward dropped the bias and norm_bwd returned uninitialised db partials as db) and is
now rejected by ops.add_norm, norm_fwd and norm_bwd; rope_fwd / rope_bwd did not check
T + pos_offset against the table with pos = None and now do. No further kernel bug found.
"""
import pytest
import torch

import _branch32_block as B32
import _refs64 as R
import _refs64_block as RB
from _refs64 import d

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WORST = {}


def _C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def dev(x):
    return None if x is None else x.to(DEV)


def bits(x):
    x = x.contiguous()
    return x.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def twice(fn):
    """Run fn twice -> the first result, after requiring bitwise equal outputs."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y)), "outputs differ between two launches"
    return a


def poison(*specs):
    """NaN-filled tensors of the launcher's at::empty scratch sizes, freed at once."""
    junk = [torch.full(shape, NAN, dtype=dt, device=DEV) for shape, dt in specs]
    del junk


def note(kernel, name, err, bound):
    r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    key = f"{kernel} {name}"
    WORST[key] = max(WORST.get(key, 0.0), r)


def check(kernel, name, got, ref, b32, extra=0.0, bf16=False, sel=None, tag=""):
    """`_refs64.check` on the elements `sel` (all by default), E32 from the fp32 branch's same elements."""
    g, r, b = got.detach().cpu(), ref, b32
    if sel is not None:
        g, r, b = g[sel], r[sel], b[sel]
        if r.numel() == 0:
            return
    err, bound = RB.check(kernel, name + tag, g, r, R.e32_of(b, r), extra, bf16)
    note(kernel, name, err, bound)


# ========================================================================================== norm
@pytest.mark.parametrize("rows,H,rms,res,bias,eps", RB.norm_grid_cases())
def test_norm_fwd(rows, H, rms, res, bias, eps):
    C = _C()
    c, groups = RB.norm_case(rows, H, rms, res, bias)
    x, r, w, b = dev(c["x"]), dev(c["res"]), dev(c["w"]), dev(c["b"])
    y, so, rstd, mean = twice(lambda: C.norm_fwd(x, r, w, b, eps, rms))
    ref = RB.norm64(c["x"], c["res"], c["w"], c["b"], eps, rms)
    b32 = B32.norm(c["x"], c["res"], c["w"], c["b"], eps, rms)
    ex = RB.norm_fwd_extra(ref, c["w"], H, rows, groups, eps)
    if res:  # the residual stream is exact: one fp32 add, one rounding
        assert torch.equal(bits(so.cpu()), bits(RB.stream(c["x"], c["res"])))
    else:
        assert so.numel() == 0
    kern = "norm_fwd_row" if rows < 512 else "norm_fwd_wave"
    for gname, idx in groups.items():
        if idx.numel() == 0:
            continue
        check(kern, "y", y, ref["y"], b32["y"], ex["y"][gname], True, idx, f"[{gname}]")
        check(kern, "rstd", rstd, ref["rstd"], b32["rstd"], ex["rstd"][gname], False, idx, f"[{gname}]")
        if not rms:
            check(kern, "mean", mean, ref["mean"], b32["mean"], ex["mean"][gname], False, idx, f"[{gname}]")


def _norm_bwd_direct(rows, H, rms, dres, bias, eps):
    C = _C()
    c, groups = RB.norm_case(rows, H, rms, False, bias)
    f = RB.norm64(c["x"], None, c["w"], c["b"], eps, rms)
    rstd32, mean32 = f["rstd"].float(), f["mean"].float()
    dr = c["dres"] if dres else None
    ref, xh = RB.norm_bwd64(c["dy"], c["x"], c["w"], rstd32, mean32, dr, eps, rms, bias)
    b32 = B32.norm_bwd(c["dy"], c["x"], c["w"], dr, eps, rms, bias)
    ex = RB.norm_bwd_extra(c["dy"], c["w"], xh, f["rstd"], H, rows, groups, rms)
    args = (dev(c["dy"]), dev(c["x"]), dev(c["w"]), dev(rstd32), None if rms else dev(mean32), dev(dr))
    srows = min(rows, RB.NORM_BWD_GRID) + RB.K_SPLIT

    def run():
        poison(((srows, H), torch.float32), ((srows, H), torch.float32), ((rows, H), torch.bfloat16),
               ((H,), torch.bfloat16), ((H,), torch.bfloat16))
        return C.norm_bwd(*args, bias, rms)

    ds, dw, db = twice(run)
    for gname, idx in groups.items():
        if idx.numel():
            check("norm_bwd", "ds", ds, ref["ds"], b32["ds"], ex["ds"][gname], True, idx, f"[{gname}]")
    check("norm_bwd", "dw", dw, ref["dw"], b32["dw"], ex["dw"], True)
    if bias:
        check("norm_bwd", "db", db, ref["db"], b32["db"], ex["db"], True)
    else:
        assert db.numel() == 0


@pytest.mark.parametrize("rows,H,rms,dres,bias,eps", RB.norm_bwd_cases())
def test_norm_bwd(rows, H, rms, dres, bias, eps):
    _norm_bwd_direct(rows, H, rms, dres, bias, eps)


def test_norm_bwd_h16384():
    """NC = 8 of the backward (H above the forward's 8192): rstd and mean built by the reference.
    37 rows: stage-1 splits of 3 partial rows, the last ones empty."""
    _norm_bwd_direct(37, 16384, False, True, True, 1e-5)


@pytest.mark.parametrize("rows,H,rms,res,bias,keep,eps", [
    (515, 520, True, True, False, False, 1e-6), (300, 136, False, True, True, False, 1e-5),
    (513, 1536, False, False, True, True, 1e-5), (5, 8, True, False, False, True, 1e-5),
    (769, 2056, False, False, False, False, 1e-6), (1537, 2048, True, True, False, False, 1e-5)])
def test_add_norm_autograd(rows, H, rms, res, bias, keep, eps):
    """ops.add_norm with autograd: the gradient of the stream output (a residual, or keep_stream)
    comes back as `dres` of the one backward kernel; x and the residual get the same gradient."""
    from distributed_llm_alignment_amd import ops

    c, groups = RB.norm_case(rows, H, rms, res, bias)
    has_dres = res or keep
    leaves = {k: dev(c[k]).requires_grad_() for k in ("x", "res", "w", "b") if c[k] is not None}
    srows = min(rows, RB.NORM_BWD_GRID) + RB.K_SPLIT

    def run():
        y, s = ops.add_norm(leaves["x"], leaves.get("res"), leaves["w"], leaves.get("b"), eps, rms, keep_stream=keep)
        poison(((srows, H), torch.float32), ((srows, H), torch.float32), ((rows, H), torch.bfloat16))
        outs, gouts = [y], [dev(c["dy"])]
        if has_dres:
            outs.append(s)
            gouts.append(dev(c["dres"]))
        gr = torch.autograd.grad(outs, list(leaves.values()), gouts)
        return (y.detach(), s.detach()) + tuple(gr)

    out = twice(run)
    y, s, grads = out[0], out[1], dict(zip(leaves, out[2:]))
    sref = RB.stream(c["x"], c["res"])
    assert torch.equal(bits(s.cpu()), bits(sref))
    f = RB.norm64(c["x"], c["res"], c["w"], c["b"], eps, rms)
    b32f = B32.norm(c["x"], c["res"], c["w"], c["b"], eps, rms)
    exf = RB.norm_fwd_extra(f, c["w"], H, rows, groups, eps)
    dr = c["dres"] if has_dres else None
    ref, xh = RB.norm_bwd64(c["dy"], sref, c["w"], f["rstd"].float(), f["mean"].float(), dr, eps, rms, bias)
    b32 = B32.norm_bwd(c["dy"], sref, c["w"], dr, eps, rms, bias)
    ex = RB.norm_bwd_extra(c["dy"], c["w"], xh, f["rstd"], H, rows, groups, rms)
    for gname, idx in groups.items():
        if idx.numel():
            check("add_norm", "y", y, f["y"], b32f["y"], exf["y"][gname], True, idx, f"[{gname}]")
            check("add_norm", "dx", grads["x"], ref["ds"], b32["ds"], ex["ds"][gname], True, idx, f"[{gname}]")
    if res:
        assert torch.equal(bits(grads["res"]), bits(grads["x"]))
    check("add_norm", "dw", grads["w"], ref["dw"], b32["dw"], ex["dw"], True)
    if bias:
        check("add_norm", "db", grads["b"], ref["db"], b32["db"], ex["db"], True)


def test_rms_norm_with_bias_is_rejected():
    """The RMS kernels have no bias: the forward dropped it and the backward returned uninitialised
    memory as db. Rejected by the bindings and by ops.add_norm."""
    from distributed_llm_alignment_amd import ops

    C = _C()
    x = torch.randn(4, 16, device=DEV).bfloat16()
    w, b = torch.ones(16, device=DEV).bfloat16(), torch.zeros(16, device=DEV).bfloat16()
    rstd = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="no bias"):
        C.norm_fwd(x, None, w, b, 1e-5, True)
    with pytest.raises(RuntimeError, match="no bias"):
        C.norm_bwd(x, x, w, rstd, None, None, True, True)
    with pytest.raises(ValueError):
        ops.add_norm(x, None, w, b, 1e-5, True)
    with pytest.raises(ValueError):
        ops.add_norm(x, x, w, b, 1e-5, True)
    ops.add_norm(x, None, w, b, 1e-5, False)


# =================================================================================== activations
@pytest.mark.parametrize("rows,F", RB.ACT_SHAPES)
def test_swiglu(rows, F):
    C = _C()
    c, planted = RB.swiglu_case(rows, F)
    gu, dy = dev(c["gu"]), dev(c["dy"])
    out, dgu = twice(lambda: (C.swiglu_fwd(gu), C.swiglu_bwd(gu, dy)))
    ref, b32 = RB.swiglu64(**c), B32.swiglu(**c)
    for tag, sel in (("[bulk]", ~planted), ("[planted]", planted)):
        if not sel.any():
            continue
        ex = RB.swiglu_extra(c["gu"], c["dy"], sel)
        check("swiglu", "out", out, ref["out"], b32["out"], ex["out"], True, sel, tag)
        check("swiglu", "dgu", dgu, ref["dgu"], b32["dgu"], ex["dgu"], True, torch.cat([sel, sel], -1), tag)


@pytest.mark.parametrize("numel", RB.GELU_NUMEL)
def test_gelu_new(numel):
    C = _C()
    c, planted = RB.gelu_case(numel)
    x, dy = dev(c["x"]), dev(c["dy"])
    y, dx = twice(lambda: (C.gelu_fwd(x), C.gelu_bwd(x, dy)))
    ref, b32 = RB.gelu_new64(**c), B32.gelu_new(**c)
    for tag, sel in (("[bulk]", ~planted), ("[planted]", planted)):
        if not sel.any():
            continue
        ex = RB.gelu_extra(c["x"], c["dy"], sel)
        check("gelu_new", "y", y, ref["y"], b32["y"], ex["y"], True, sel, tag)
        check("gelu_new", "dx", dx, ref["dx"], b32["dx"], ex["dx"], True, sel, tag)


# ========================================================================================== RoPE
SENT = 777.0  # exact in bf16


def _rope_run(B, T, Hq, Hkv, D, rot, kind, max_pos=RB.ROPE_MAXPOS):
    C = _C()
    cos, sin = RB.rope_tables(rot, max_pos)
    tokens = B * T
    c = RB.rope_case(tokens, Hq, Hkv, D)
    kpos, off, pos = RB.rope_positions(kind, B, T, max_pos)
    nqk = (Hq + Hkv) * D
    buf = dev(c["buf"])
    view = buf[:, :c["W"]]
    assert view.stride(0) > view.shape[1] > (Hq + 2 * Hkv) * D
    cd, sd, pd = dev(cos), dev(sin), dev(kpos)
    q, k = twice(lambda: C.rope_fwd(view, cd, sd, pd, Hq, Hkv, D, rot, T, off))
    assert torch.equal(bits(buf.cpu()), bits(c["buf"]))  # the source is read only
    src = c["buf"][:, :nqk].reshape(tokens, Hq + Hkv, D)
    got = torch.cat([q.view(tokens, Hq, D), k.view(tokens, Hkv, D)], 1)
    ref, b32 = RB.rope64(src, cos, sin, pos, rot)["out"], B32.rope(src, cos, sin, pos, rot)["out"]
    check("rope_fwd", "qk", got, ref, b32, RB.rope_extra(src), True)
    # backward: un-rotated gradients into the q / k column slices of a sentinel-filled dqkv
    dq, dk = dev(c["dq"]), dev(c["dk"])

    def bwd():
        dqkv = torch.full(tuple(c["buf"].shape), SENT, dtype=torch.bfloat16, device=DEV)
        C.rope_bwd(dq, dk, dqkv[:, :c["W"]], cd, sd, pd, Hq, Hkv, D, rot, T, off)
        return (dqkv,)

    (dqkv,) = twice(bwd)
    rest = dqkv[:, nqk:].cpu()
    assert torch.equal(bits(rest), bits(torch.full_like(rest, SENT))), "rope_bwd wrote outside the q / k columns"
    gsrc = torch.cat([c["dq"].view(tokens, Hq, D), c["dk"].view(tokens, Hkv, D)], 1)
    ref, b32 = RB.rope64(gsrc, cos, sin, pos, rot, True)["out"], B32.rope(gsrc, cos, sin, pos, rot, True)["out"]
    check("rope_bwd", "dqk", dqkv[:, :nqk].reshape(tokens, Hq + Hkv, D), ref, b32, RB.rope_extra(gsrc), True)


@pytest.mark.parametrize("kind", ["off0", "off37", "explicit"])
@pytest.mark.parametrize("Hq,Hkv", RB.ROPE_HEADS)
@pytest.mark.parametrize("D,rot", RB.ROPE_DROT)
def test_rope(D, rot, Hq, Hkv, kind):
    _rope_run(2, 24, Hq, Hkv, D, rot, kind)


def test_rope_grid_stride():
    """More work items than the 2048-block cap covers in one trip."""
    b = RB.ROPE_BIG
    _rope_run(1, b["tokens"], b["Hq"], b["Hkv"], b["D"], b["rot"], "off0", max_pos=b["tokens"])


def test_rope_table_range_is_checked():
    """pos = None: T + pos_offset beyond the table is refused before any launch."""
    C = _C()
    cos, sin = (dev(t) for t in RB.rope_tables(64, 32))
    qkv = torch.zeros(48, 4 * 64, dtype=torch.bfloat16, device=DEV)
    dq, dk = torch.zeros(48, 2 * 64, dtype=torch.bfloat16, device=DEV), torch.zeros(48, 64, dtype=torch.bfloat16, device=DEV)
    for T, off in ((48, 0), (24, 9), (16, 17)):
        with pytest.raises(RuntimeError, match="table"):
            C.rope_fwd(qkv, cos, sin, None, 2, 1, 64, 64, T, off)
        with pytest.raises(RuntimeError, match="table"):
            C.rope_bwd(dq, dk, qkv, cos, sin, None, 2, 1, 64, 64, T, off)
    C.rope_fwd(qkv, cos, sin, None, 2, 1, 64, 64, 24, 8)  # T + offset == table length is in range


# ===================================================================================== embedding
@pytest.mark.parametrize("H", RB.EMB_H)
def test_embedding_forward_exact(H):
    C = _C()
    g = R.gen(H)
    V = 50
    buf = dev(torch.randn(V, H + 8, generator=g).bfloat16())
    ids = dev(torch.randint(0, V, (37,), generator=g))
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for w in (buf[:, :H], buf[:, :H].contiguous()):  # ldw > H and ldw == H
        (out,) = twice(lambda: (C.embed_fwd(w, ids, bad),))
        assert torch.equal(bits(out), bits(w[ids]))
    assert bad.item() == 0


@pytest.mark.parametrize("kind,H,gdtype", RB.EMB_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_embed_bwd(kind, H, gdtype):
    """The binding with constructed sorted ids and permutation, onto a nonzero base. Cases with H
    not a multiple of 16 use a gradient view with ldg > H inside a sentinel-filled buffer."""
    C = _C()
    c = RB.emb_case(kind, H, gdtype)
    V, N = c["V"], c["sid"].numel()
    strided = (H // 8) % 2 == 1 or kind == "edges_oob"
    sid, perm, dy = dev(c["sid"]), dev(c["perm"]), dev(c["dy"])

    def run():
        buf = torch.full((V + 2, H + 8), SENT, dtype=gdtype, device=DEV)
        grad = buf[1:V + 1, :H] if strided else torch.empty(V, H, dtype=gdtype, device=DEV)
        grad.copy_(dev(c["base"]))
        poison(((N, H), torch.float32))
        C.embed_bwd(sid, perm, dy, grad)
        return grad, buf

    grad, buf = twice(run)
    args = (c["sid"], c["perm"], c["dy"], c["base"], V)
    ref, b32 = RB.embed_bwd64(*args)["grad"], B32.embed_bwd(*args)["grad"]
    check("embed_bwd", "grad", grad, ref, b32, RB.embed_extra(*args), gdtype == torch.bfloat16)
    ok = (c["sid"] >= 0) & (c["sid"] < V)
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[c["sid"][ok]] = False
    assert torch.equal(bits(grad.cpu()[untouched]), bits(c["base"][untouched])), "an untouched row changed"
    if strided:
        b = buf.cpu()
        for part in (b[0], b[V + 1], b[:, H:]):
            assert torch.equal(bits(part), bits(torch.full_like(part, SENT))), "embed_bwd wrote outside the gradient view"


@pytest.mark.parametrize("path", ["dense", "main_grad_f32", "main_grad_bf16"])
def test_embedding_autograd(path):
    """ops.embedding + backward: the device sort feeds the same kernels."""
    from distributed_llm_alignment_amd import ops

    H = 520
    c = RB.emb_case("edges", H, torch.bfloat16 if path == "main_grad_bf16" else torch.float32)
    V, N = c["V"], c["sid"].numel()
    ids = torch.empty(N, dtype=torch.int64)
    ids[c["perm"]] = c["sid"]  # position perm[j] holds token sid[j]
    base = torch.zeros_like(c["base"]) if path == "dense" else c["base"]
    w = dev(torch.randn(V, H, generator=R.gen(9)).bfloat16()).requires_grad_()

    def run():
        w.grad = None
        if path != "dense":
            w.main_grad = dev(base).clone()
        out = ops.embedding(dev(ids).view(2, N // 2), w)
        assert torch.equal(bits(out.detach().view(N, H)), bits(w.detach()[dev(ids)]))
        poison(((N, H), torch.float32))
        out.backward(dev(c["dy"]).view(2, N // 2, H))
        return (w.grad if path == "dense" else w.main_grad,)

    (grad,) = twice(run)
    # a stable sort orders equal ids by position; the sum over a run is checked whatever its order
    args = (c["sid"], c["perm"], c["dy"], base, V)
    ref, b32 = RB.embed_bwd64(*args)["grad"], B32.embed_bwd(*args)["grad"]
    check("embedding", "grad " + path, grad, ref, b32, RB.embed_extra(*args), grad.dtype == torch.bfloat16)


# =================================================================================== reward head
@pytest.mark.parametrize("pooling", ["last_token", "mean"])
@pytest.mark.parametrize("H,T,p,has_bias,strided", RB.RH_CASES)
def test_reward_head(H, T, p, has_bias, strided, pooling):
    from distributed_llm_alignment_amd.models.reward import _RewardHeadFn

    C = _C()
    B, seed = 4, 1234 + H
    c = RB.rh_case(B, T, H, pooling)
    bias = c["bias"] if has_bias else None
    hidden = dev(c["hidden"]._base)[:, :, :H] if strided else dev(c["hidden"].contiguous())
    assert (hidden.stride(1) > H) == strided
    last, mask, w, bd, ds = dev(c["last"]), dev(c["mask"]), dev(c["w"]), dev(bias), dev(c["ds"])

    def run():
        score, pooled = C.reward_head_fwd(hidden, last, mask, w, bd, p, seed)
        return score, pooled, C.reward_head_bwd(ds, hidden, last, mask, w, p, seed)

    score, pooled, dh = twice(run)
    ref = RB.reward_head64(c["hidden"], c["last"], c["mask"], c["w"], bias, p, seed, c["ds"])
    scale = 1.0 / (1.0 - p)
    b32 = B32.reward_head(c["hidden"], c["last"], c["mask"], c["w"], bias, ref["keep"], scale, c["ds"])
    # the keep mask, exactly: wherever the undropped pooled value is nonzero the output is nonzero
    # iff the CPU hash keeps the column; in the backward likewise wherever ds * w is nonzero
    full = RB.reward_head64(c["hidden"], c["last"], c["mask"], c["w"], bias, 0.0, 0)["pooled"]
    live = full != 0
    assert torch.equal((pooled.cpu() != 0)[live], ref["keep"][live]), "forward keep mask differs from the hash"
    on = ref["route"] != 0  # [B, T]
    gl = (d(c["ds"])[:, None] * d(c["w"]) != 0)[:, None, :] & on[:, :, None]
    assert torch.equal((dh.cpu() != 0)[gl], ref["keep"][:, None, :].expand(B, T, H)[gl]), "backward keep mask differs"
    assert (dh.cpu()[~on] == 0).all(), "dhidden is not zero off the pooled positions"
    if pooling == "last_token":  # a gather times a power of two: exact
        assert torch.equal(d(pooled.cpu()), ref["pooled"])
    else:  # bf16(mean): one bf16 ulp where the fp32 and the fp64 mean round to different neighbours
        # (a whole ulp: `_refs64.check` itself, not the half-ulp form of `_refs64_block.check`)
        note("reward_head", "pooled", *R.check("reward_head", "pooled", pooled, ref["pooled"], 0.0, 0.0, True))
        assert ((d(pooled.cpu()) - ref["pooled"]).abs() <= ref["flip"] + 4 * R.EPS32 * ref["pooled"].abs().max()).all(), \
            "pooled differs from the reference away from a rounding tie"
    ex = RB.rh_extra(c["hidden"], c["mask"], c["w"], ref) + ref["score_flip"].max().item()
    check("reward_head", "score", score, ref["score"], b32["score"], ex)
    check("reward_head", "dhidden", dh, ref["dhidden"], b32["dhidden"], 0.0, True)
    # the weight gradient of the autograd node (sum_b ds_b pooled_b in fp32, rounded to bf16)
    w2 = w.view(1, H).clone().requires_grad_()
    sc = _RewardHeadFn.apply(hidden, w2, bd, last, mask, p, seed)
    assert torch.equal(bits(sc.detach()), bits(score))
    (dw,) = torch.autograd.grad(sc, w2, ds)
    exw = ref["dw_flip"].max().item() + B * RB.U32 * (d(c["ds"]).abs()[:, None] * ref["pooled"].abs()).sum(0).max().item()
    check("reward_head", "dw", dw.view(-1), ref["dw"], b32["dw"], exw, True)


# ===================================================================================== transpose
@pytest.mark.parametrize("R_,C_", RB.TRANSPOSE_LDS)
def test_transpose_lds_kernel(R_, C_):
    """R or C not a multiple of 8: the LDS kernel with partial tiles and scalar tails, on strided
    views (row strides multiples of 8); the slack columns of `out` stay untouched."""
    C = _C()
    assert R_ % 8 or C_ % 8
    ldi, ldo = (C_ + 7) // 8 * 8 + 8, (R_ + 7) // 8 * 8 + 16
    src = torch.randn(R_, ldi, generator=R.gen(R_ * 131 + C_)).bfloat16().to(DEV)
    x = src[:, :C_]

    def run():
        buf = torch.full((C_, ldo), SENT, dtype=torch.bfloat16, device=DEV)
        C.transpose_bf16(x, buf[:, :R_])
        return (buf,)

    (buf,) = twice(run)
    assert torch.equal(bits(buf[:, :R_]), bits(x.t()))
    slack = buf[:, R_:]
    assert torch.equal(bits(slack), bits(torch.full_like(slack, SENT))), "transpose wrote into the slack columns"


def test_block_kernels_report():
    """Prints the worst error / bound per kernel and output over the cases that ran before it."""
    for key in sorted(WORST):
        print(f"FIG block worst {key}: {WORST[key]:.3f}")
