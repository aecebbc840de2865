"""Argument contract of the decode projection torch ops (csrc/bindings_decode.cpp): what
`skinny_gemm`, `skinny_glu_ks`, `skinny_fused`, `skinny_fused_f8`, `skinny_glu_il`,
`skinny_glu_il_f8`, `skinny64`, `skinny64_f8`, `tile_weight` and `quant_tile_f8` accept and what
they refuse on the host, before any launch. The accepted calls use one tiny shape per op and are
checked against the references and tolerances of tests/test_decode_gpu.py; every refused call
raises before a kernel runs.

Two combinations one might expect to be refused are accepted, and recorded here as such:
`skinny_fused` / `skinny_fused_f8` with `res` AND `ssq_in` (the kernel has that form: normalised
input, residual output), and `skinny_gemm` at 17 rows on the narrow split-K shape."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 1e-5
# (N, K): K = 1024, N = 32 on the split-K ops, N = 128 on the GLU forms, K = 512, N = 128 at 17..64 rows
SHAPES = {"skinny_gemm": (32, 1024), "skinny_glu_ks": (128, 1024), "skinny_fused": (32, 1024),
          "skinny_fused_f8": (32, 1024), "skinny_glu_il": (128, 1024), "skinny_glu_il_f8": (128, 1024),
          "skinny64": (128, 512), "skinny64_f8": (128, 512)}
OPS = list(SHAPES)
F8 = [op for op in OPS if op.endswith("_f8")]
GLU_IL = ["skinny_glu_il", "skinny_glu_il_f8"]
M64 = ["skinny64", "skinny64_f8"]
FUSED = ["skinny_fused", "skinny_fused_f8"]
ROW_MAJOR = ["skinny_gemm", "skinny_glu_ks", "skinny_fused", "skinny64"]  # ops taking a row-major bf16 w
MAX_ROWS = {op: 16 if op in FUSED + GLU_IL else 64 for op in OPS}


@pytest.fixture(scope="module")
def C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def _bf(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(torch.bfloat16)


def _tile(C, w, nw=None, il=False):
    out = torch.empty(w.shape[0] // 16, w.shape[1] // 32, 4, 16, 8, device=DEV, dtype=torch.bfloat16)
    C.tile_weight(w, nw, out, il)
    return out


def _quant(C, w, nw=None, il=False):
    out = torch.empty(w.shape[0] // 16, w.shape[1] // 64, 64, 16, device=DEV, dtype=torch.uint8)
    sc = torch.empty(w.shape[0], device=DEV, dtype=torch.float32)
    C.quant_tile_f8(w, nw, out, sc, il)
    return out, sc


def _dequant(w8, wscale, il=False):
    """fp32 [N, K] weight that the e4m3 tiled copy (tile_f8's layout, `il`: gate / up rows interleaved
    8 + 8 per tile) and its scales stand for: with it as the reference only accumulation order and
    bf16 output rounding differ, as in test_decode_gpu.py. (The quantiser itself is checked against
    torch below; at K = 512 one e4m3 step on a rounding tie is worth more than the tolerance.)"""
    T, KT = w8.shape[:2]
    q = w8.view(T, KT, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(16 * T, 64 * KT)
    w = q.view(torch.float8_e4m3fn).float() * wscale[:, None]
    if il:
        w = w.view(T, 2, 8, -1)
        w = torch.cat([w[:, 0].reshape(8 * T, -1), w[:, 1].reshape(8 * T, -1)])
    return w


def _partials(s, rows, per):
    """fp32 [rows, K / per] partial sums of squares of s's rows (rows past M zero)."""
    sq = torch.zeros(max(rows, s.shape[0]), s.shape[1] // per, device=DEV)
    sq[:s.shape[0]] = (s.float() ** 2).view(s.shape[0], -1, per).sum(-1)
    return sq


def _args(C, op, M=5, N=None, K=None):
    """Valid arguments of `op` at its tiny shape: plain for the projections, the GLU forms with
    their row-norm partials."""
    N, K = N or SHAPES[op][0], K or SHAPES[op][1]
    g = torch.Generator(device=DEV).manual_seed(M + N)
    a = dict(x=_bf(g, M, K), w=_bf(g, N, K, scale=K ** -0.5), res=None, ssq_in=None, eps=EPS, glu=False,
             counters=torch.zeros(8, device=DEV, dtype=torch.int32), swiglu=False, glu_out=False)
    a["nw"] = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(torch.bfloat16)
    a["res_in"] = _bf(g, M, N)
    il = op in GLU_IL
    if il:
        a["ssq_in"] = _partials(a["x"], 16, 16)
    if op == "skinny_glu_il":
        a["wt"] = _tile(C, a["w"], a["nw"], True)
    if op in F8:
        a["w8"], a["wscale"] = _quant(C, a["w"], a["nw"] if il else None, il)
    return a


def _call(C, op, a):
    if op == "skinny_gemm":
        return C.skinny_gemm(a["x"], a["w"], a["counters"], a["swiglu"], a["glu_out"])
    if op == "skinny_glu_ks":
        return C.skinny_glu_ks(a["x"], a["w"])
    if op == "skinny_fused":
        return C.skinny_fused(a["x"], a["w"], a["res"], a["ssq_in"], a["eps"], a["glu"])
    if op == "skinny_fused_f8":
        return C.skinny_fused_f8(a["x"], a["w8"], a["wscale"], a["res"], a["ssq_in"], a["eps"])
    if op == "skinny_glu_il":
        return C.skinny_glu_il(a["x"], a["wt"], a["ssq_in"], a["eps"])
    if op == "skinny_glu_il_f8":
        return C.skinny_glu_il_f8(a["x"], a["w8"], a["wscale"], a["ssq_in"], a["eps"])
    if op == "skinny64":
        return C.skinny64(a["x"], a["w"], a["res"], a["ssq_in"], a["eps"], a["glu"])
    return C.skinny64_f8(a["x"], a["w8"], a["wscale"], a["res"], a["ssq_in"], a["eps"], a["glu"])


def _glu_ref(gu):
    g, u = gu.float().chunk(2, dim=-1)
    return torch.nn.functional.silu(g) * u


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


# ------------------------------------------------------------------------------ accepted calls
@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
def test_skinny_gemm_accepts(C, M):
    from distributed_llm_alignment_amd.ops import decode

    a = _args(C, "skinny_gemm", M)
    y = _call(C, "skinny_gemm", a)
    r = decode.ref_skinny_linear(a["x"], a["w"])
    assert y.shape == (M, 32) and y.dtype == torch.bfloat16
    err = (y.float() - r.float()).abs().max().item()
    assert err <= 2e-2 * max(1.0, r.float().abs().max().item()), err
    if M > 16:
        return
    g = torch.Generator(device=DEV).manual_seed(M)
    a["x"], a["swiglu"] = _bf(g, M, 2048), True  # the LDS-staged kernel: x = gu [M, 2K]
    y = _call(C, "skinny_gemm", a)
    r = decode.ref_skinny_linear(a["x"], a["w"], True)
    err = (y.float() - r.float()).abs().max().item()
    assert err <= 2e-2 * max(1.0, r.float().abs().max().item()), err
    a = _args(C, "skinny_gemm", M, N=128)
    a["glu_out"] = True
    m = _call(C, "skinny_gemm", a)
    r = _glu_ref((a["x"].float() @ a["w"].float().t()).to(torch.bfloat16))
    assert m.shape == (M, 64)
    err = (m.float() - r).abs().max().item()
    assert err <= 3e-2 * max(1.0, r.abs().max().item()), err


@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
def test_skinny_glu_ks_accepts(C, M):
    a = _args(C, "skinny_glu_ks", M)
    m = _call(C, "skinny_glu_ks", a)
    r = _glu_ref((a["x"].float() @ a["w"].float().t()).to(torch.bfloat16))
    assert m.shape == (M, 64) and m.dtype == torch.bfloat16
    err = (m.float() - r).abs().max().item()
    assert err <= 3e-2 * max(1.0, r.abs().max().item()), err


def _check_residual_form(a, s, ssq, wf, M):
    s_ref = (a["x"].float() @ wf.t()).to(torch.bfloat16).float() + a["res"].float()
    assert float((s.float() - s_ref).abs().max()) < 0.05
    assert torch.allclose(ssq[:M].sum(1), (s.float() ** 2).sum(1), rtol=1e-4)


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("op", FUSED)
def test_fused_ops_accept(C, op, M):
    """Plain, residual producer, norm-on-input consumer; and both at once, which the ops accept."""
    from distributed_llm_alignment_amd.ops import decode
    from distributed_llm_alignment_amd.ops.norm import _ref_norm

    a = _args(C, op, M)
    wf = _dequant(a["w8"], a["wscale"]) if op in F8 else a["w"].float()
    y, _ = _call(C, op, a)
    assert y.shape == (M, 32)
    r = (a["x"].float() @ wf.t()).to(torch.bfloat16)
    err = (y.float() - r.float()).abs().max().item()
    assert err <= 2e-2 * max(1.0, r.float().abs().max().item()), err
    if op == "skinny_fused":
        assert torch.equal(r, decode.ref_skinny_linear(a["x"], a["w"]))
    a["res"] = a["res_in"]
    s, ssq = _call(C, op, a)
    assert ssq.shape == (16, 2) and ssq.dtype == torch.float32
    _check_residual_form(a, s, ssq, wf, M)
    # consumer: x a residual stream with its partials, the norm weight folded into w
    b = _args(C, op, M)
    s, b["ssq_in"] = b["x"], _partials(b["x"], 16, 16)
    if op in F8:
        b["w8"], b["wscale"] = _quant(C, b["w"], b["nw"])
        wn = _dequant(b["w8"], b["wscale"])
    else:
        b["w"] = b["w"] * b["nw"].view(1, -1)
        wn = b["w"].float()
    y, _ = _call(C, op, b)
    rstd = torch.rsqrt((s.float() ** 2).mean(1, keepdim=True) + EPS)
    assert _rel(y, (s.float() * rstd) @ wn.t()) < 1e-2
    if op == "skinny_fused":
        h_ref = _ref_norm(s.float(), b["nw"].float(), None, EPS, True)
        assert _rel(y, h_ref @ a["w"].float().t()) < 1e-2
    b["res"] = b["res_in"]  # normalised input AND residual output: accepted
    s2, ssq2 = _call(C, op, b)
    assert ssq2.shape == (16, 2)
    s2_ref = ((s.float() * rstd) @ wn.t()).to(torch.bfloat16).float() + b["res"].float()
    assert float((s2.float() - s2_ref).abs().max()) < 0.05
    assert torch.allclose(ssq2[:M].sum(1), (s2.float() ** 2).sum(1), rtol=1e-4)


@pytest.mark.parametrize("M", [1, 5, 16])
def test_skinny_fused_glu_accepts(C, M):
    from distributed_llm_alignment_amd.ops.norm import _ref_norm

    a = _args(C, "skinny_fused", M, N=128)
    h_ref = _ref_norm(a["x"].float(), a["nw"].float(), None, EPS, True)
    m_ref = _glu_ref(h_ref @ a["w"].float().t())
    a.update(ssq_in=_partials(a["x"], 16, 16), glu=True)
    folded = a["w"] * a["nw"].view(1, -1)
    outs = []
    for w in (folded, _tile(C, a["w"], a["nw"])):  # row-major and tiled: the same bits
        a["w"] = w
        m, _ = _call(C, "skinny_fused", a)
        assert m.shape == (M, 64) and _rel(m, m_ref) < 1e-2
        outs.append(m)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("op", GLU_IL)
def test_glu_il_ops_accept(C, op, M):
    from distributed_llm_alignment_amd.ops.norm import _ref_norm

    a = _args(C, op, M)
    m = _call(C, op, a)
    assert m.shape == (M, 64) and m.dtype == torch.bfloat16
    if op in F8:
        rstd = torch.rsqrt((a["x"].float() ** 2).mean(1, keepdim=True) + EPS)
        gu = (a["x"].float() * rstd) @ _dequant(a["w8"], a["wscale"], True).t()
    else:
        gu = _ref_norm(a["x"].float(), a["nw"].float(), None, EPS, True) @ a["w"].float().t()
    assert _rel(m, _glu_ref(gu)) < 1e-2


@pytest.mark.parametrize("M", [17, 64])
@pytest.mark.parametrize("op", M64)
def test_skinny64_ops_accept(C, op, M):
    from distributed_llm_alignment_amd.ops import decode

    a = _args(C, op, M)
    wf = _dequant(a["w8"], a["wscale"]) if op in F8 else a["w"].float()
    y, _ = _call(C, op, a)
    assert y.shape == (M, 128)
    assert _rel(y, a["x"].float() @ wf.t()) < 5e-3
    if op == "skinny64":
        r = decode.ref_skinny_linear(a["x"], a["w"])
        assert (y.float() - r.float()).abs().max().item() <= 2e-2 * max(1.0, r.float().abs().max().item())
        assert torch.equal(C.skinny64(a["x"], _tile(C, a["w"]), None, None, 0.0, False)[0], y)
    a["res"] = a["res_in"]
    s, ssq = _call(C, op, a)
    assert ssq.shape == (M, 1) and ssq.dtype == torch.float32
    _check_residual_form(a, s, ssq, wf, M)
    b = _args(C, op, M)
    s, b["ssq_in"] = b["x"], _partials(b["x"], M, 512)  # [M, 1]: one partial per 1024 columns of a producer
    if op in F8:
        b["w8"], b["wscale"] = _quant(C, b["w"], b["nw"])
        wn = _dequant(b["w8"], b["wscale"])
    else:
        b["w"] = b["w"] * b["nw"].view(1, -1)
        wn = b["w"].float()
    rstd = torch.rsqrt((s.float() ** 2).mean(1, keepdim=True) + EPS)
    y, _ = _call(C, op, b)
    assert _rel(y, (s.float() * rstd) @ wn.t()) < 1e-2
    for ssq_in in (b["ssq_in"], None):  # gate|up with and without the row factor
        b.update(glu=True, ssq_in=ssq_in)
        m, _ = _call(C, op, b)
        gu = (s.float() * (rstd if ssq_in is not None else 1.0)) @ wn.t()
        assert m.shape == (M, 64) and _rel(m, _glu_ref(gu)) < 1e-2


def test_tile_weight_and_quant_tile_f8_accept(C):
    from distributed_llm_alignment_amd.ops import decode

    g = torch.Generator(device=DEV).manual_seed(3)
    w = _bf(g, 64, 128)
    nw = (1 + 0.1 * torch.randn(128, device=DEV, generator=g)).to(torch.bfloat16)
    for norm in (None, nw):
        for il in (False, True):
            src = w if norm is None else w * norm.view(1, -1)
            src = decode._glu_interleave(src) if il else src
            assert torch.equal(_tile(C, w, norm, il), src.reshape(4, 16, 4, 4, 8).permute(0, 2, 3, 1, 4))
            t, sc = _quant(C, w, norm, il)
            q_ref, sc_ref = decode.quantize_rows_f8(src)
            assert torch.allclose(sc, sc_ref, rtol=1e-6, atol=0)
            t_ref = decode.tile_f8(q_ref)
            assert (t != t_ref).float().mean().item() < 1e-2
            assert int((t.int() - t_ref.int()).abs().max()) <= 1


# ------------------------------------------------------------------------------- refused calls
def _offset4(t):
    """The same values behind a view that starts 4 elements (8 bytes) into its storage."""
    buf = torch.zeros(t.numel() + 8, device=DEV, dtype=t.dtype)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _inner_stride2(t):
    buf = torch.zeros(t.shape[0], 2 * t.shape[1], device=DEV, dtype=t.dtype)
    return buf[:, ::2]


def _row_stride_plus4(t):
    buf = torch.zeros(t.shape[0], t.shape[1] + 4, device=DEV, dtype=t.dtype)
    return buf[:, :t.shape[1]]


TENSOR_BAD = {"f16": lambda t: t.half(), "inner_stride": _inner_stride2, "row_stride": _row_stride_plus4,
              "offset8": _offset4}


def _refused(C, op, a):
    with pytest.raises(RuntimeError):
        _call(C, op, a)


@pytest.mark.parametrize("bad", TENSOR_BAD)
@pytest.mark.parametrize("op", OPS)
def test_every_op_refuses_bad_x(C, op, bad):
    a = _args(C, op)
    a["x"] = TENSOR_BAD[bad](a["x"])
    _refused(C, op, a)


@pytest.mark.parametrize("bad", TENSOR_BAD)
@pytest.mark.parametrize("op", ROW_MAJOR)
def test_row_major_ops_refuse_bad_w(C, op, bad):
    a = _args(C, op)
    a["w"] = TENSOR_BAD[bad](a["w"])
    _refused(C, op, a)


@pytest.mark.parametrize("op", OPS)
def test_every_op_refuses_row_counts(C, op):
    a = _args(C, op)
    a["x"] = a["x"][:0]
    _refused(C, op, a)
    b = _args(C, op, MAX_ROWS[op] + 1)  # 17 or 65 rows
    if op in GLU_IL:
        b["ssq_in"] = b["ssq_in"][:16].contiguous()
    _refused(C, op, b)


def test_skinny_gemm_refuses_17_rows_off_the_split_k_path(C):
    for form in (dict(swiglu=True), dict(glu_out=True)):
        a = _args(C, "skinny_gemm", 17, N=128)
        if "swiglu" in form:
            a["x"] = torch.cat([a["x"], a["x"]], 1)
        a.update(form)
        _refused(C, "skinny_gemm", a)
    _refused(C, "skinny_gemm", _args(C, "skinny_gemm", 17, K=512))  # K % 1024: not a split-K shape


@pytest.mark.parametrize("op,N,K", [
    ("skinny_gemm", 32, 384), ("skinny_gemm", 24, 1024), ("skinny_glu_ks", 128, 768), ("skinny_glu_ks", 48, 1024),
    ("skinny_fused", 32, 512), ("skinny_fused", 24, 1024), ("skinny_fused", 16384, 1024),
    ("skinny64", 128, 384), ("skinny64", 64, 512)])
def test_row_major_ops_refuse_shape_multiples(C, op, N, K):
    _refused(C, op, _args(C, op, 5 if op not in M64 else 17, N=N, K=K))


def _raw_w8(a, tiles, ktiles):
    a["w8"] = torch.zeros(tiles, ktiles, 64, 16, device=DEV, dtype=torch.uint8)
    a["wscale"] = torch.ones(16 * tiles, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    a["x"] = _bf(g, a["x"].shape[0], 64 * ktiles)
    a["res_in"] = _bf(g, a["x"].shape[0], 16 * tiles)


@pytest.mark.parametrize("op,tiles,ktiles,res", [
    ("skinny_fused_f8", 2, 8, False),      # K = 512: K % 1024
    ("skinny_fused_f8", 1024, 16, True),   # N = 16384 on a fused form
    ("skinny_glu_il_f8", 8, 4, False),     # K = 256: K % 512
    ("skinny_glu_il_f8", 1, 16, False),    # N = 16: 2F % 32
    ("skinny64_f8", 8, 7, False),          # K = 448: K % 256
    ("skinny64_f8", 4, 8, False)])         # N = 64: N % 128
def test_f8_ops_refuse_shape_multiples(C, op, tiles, ktiles, res):
    a = _args(C, op, 17 if op in M64 else 5)
    _raw_w8(a, tiles, ktiles)
    if res:
        a["res"] = a["res_in"]
    if op in GLU_IL:
        a["ssq_in"] = torch.ones(16, 4, device=DEV)
    _refused(C, op, a)


def test_skinny_glu_il_refuses_weight_layouts(C):
    a = _args(C, "skinny_glu_il")
    a["wt"] = a["w"]  # row-major
    _refused(C, "skinny_glu_il", a)
    a["wt"] = torch.zeros(16, 32, 4, 16, 8, device=DEV, dtype=torch.bfloat16)[::2]  # not contiguous
    _refused(C, "skinny_glu_il", a)
    a = _args(C, "skinny_glu_il")
    g = torch.Generator(device=DEV).manual_seed(2)
    a["x"], a["wt"] = _bf(g, 5, 256), torch.zeros(8, 8, 4, 16, 8, device=DEV, dtype=torch.bfloat16)  # K = 256
    a["ssq_in"] = torch.ones(16, 4, device=DEV)
    _refused(C, "skinny_glu_il", a)


@pytest.mark.parametrize("op", F8)
def test_f8_ops_refuse_weight_arguments(C, op):
    M = 17 if op in M64 else 5
    a = _args(C, op, M)
    a["wscale"] = a["wscale"][:-1].contiguous()
    _refused(C, op, a)
    a = _args(C, op, M)
    a["wscale"] = a["wscale"].double()
    _refused(C, op, a)
    a = _args(C, op, M)
    a["w8"] = torch.zeros(2 * a["w8"].shape[0], *a["w8"].shape[1:], device=DEV, dtype=torch.uint8)[::2]
    assert not a["w8"].is_contiguous()
    _refused(C, op, a)
    a = _args(C, op, M)
    a["w8"] = a["w8"].view(torch.int8)
    _refused(C, op, a)


@pytest.mark.parametrize("op", FUSED + GLU_IL + M64)
def test_ssq_in_ops_refuse_partials(C, op):
    M = 17 if op in M64 else 5
    rows, limit = (M, 64) if op in M64 else (16, 512)
    for shape in [(rows + 1, 4), (rows, 0), (rows, limit + 1)]:
        a = _args(C, op, M)
        a["ssq_in"] = torch.ones(*shape, device=DEV)
        _refused(C, op, a)
    a = _args(C, op, M)
    a["ssq_in"] = torch.ones(rows, 4, device=DEV, dtype=torch.float64)
    _refused(C, op, a)
    a["ssq_in"] = torch.ones(rows, 8, device=DEV)[:, ::2]
    _refused(C, op, a)


@pytest.mark.parametrize("op", FUSED + M64)
def test_res_ops_refuse_residual_arguments(C, op):
    M = 17 if op in M64 else 5
    N = SHAPES[op][0]
    a = _args(C, op, M)
    a["res"] = torch.zeros(M, N + 16, device=DEV, dtype=torch.bfloat16)
    _refused(C, op, a)
    a["res"] = torch.zeros(M + 1, N, device=DEV, dtype=torch.bfloat16)
    _refused(C, op, a)
    a["res"] = torch.zeros(M, N, device=DEV, dtype=torch.float16)
    _refused(C, op, a)
    if op in M64:  # a residual output takes a plain input
        a = _args(C, op, M)
        a.update(res=a["res_in"], ssq_in=torch.ones(M, 1, device=DEV))
        _refused(C, op, a)
    if op != "skinny_fused_f8":  # (it has no glu argument)
        a = _args(C, op, M, N=128)
        a.update(res=a["res_in"], ssq_in=torch.ones(M if op in M64 else 16, 4, device=DEV), glu=True)
        _refused(C, op, a)
        a["ssq_in"] = None
        _refused(C, op, a)


def test_skinny_fused_glu_refusals(C):
    a = _args(C, "skinny_fused", N=128)
    a["glu"] = True  # no ssq_in
    _refused(C, "skinny_fused", a)
    a = _args(C, "skinny_fused", N=64)  # 2F % 128
    a.update(glu=True, ssq_in=torch.ones(16, 4, device=DEV))
    _refused(C, "skinny_fused", a)


def test_staged_kernels_refuse_x_past_lds(C):
    """16 rows x 8192: 262 KB of x, past every LDS limit of the kernels that stage all of x."""
    a = _args(C, "skinny_gemm", 16, N=128, K=8192)
    a["glu_out"] = True
    _refused(C, "skinny_gemm", a)
    a = _args(C, "skinny_fused", 16, N=128, K=8192)
    a.update(glu=True, ssq_in=torch.ones(16, 512, device=DEV))
    _refused(C, "skinny_fused", a)
    for op in GLU_IL:
        _refused(C, op, _args(C, op, 16, N=32, K=8192))


def test_skinny_gemm_refuses_counters(C):
    a = _args(C, "skinny_gemm", N=256)
    a["counters"] = torch.zeros(1, device=DEV, dtype=torch.int32)  # two column blocks
    _refused(C, "skinny_gemm", a)
    a["counters"] = torch.zeros(8, device=DEV, dtype=torch.int64)
    _refused(C, "skinny_gemm", a)
    a["counters"] = torch.zeros(16, device=DEV, dtype=torch.int32)[::2]
    _refused(C, "skinny_gemm", a)
    a["counters"] = torch.zeros(8, device=DEV, dtype=torch.int32)
    a["swiglu"] = True  # x is [M, K], not [M, 2K]
    _refused(C, "skinny_gemm", a)


def test_tile_weight_and_quant_tile_f8_refuse(C):
    g = torch.Generator(device=DEV).manual_seed(4)

    def tile(w, nw=None, il=False, out=None):
        out = out if out is not None else torch.empty(w.shape[0] // 16, w.shape[1] // 32, 4, 16, 8, device=DEV,
                                                      dtype=torch.bfloat16)
        C.tile_weight(w, nw, out, il)

    def quant(w, nw=None, il=False, out=None, sc=None):
        out = out if out is not None else torch.empty(w.shape[0] // 16, w.shape[1] // 64, 64, 16, device=DEV,
                                                      dtype=torch.uint8)
        C.quant_tile_f8(w, nw, out, sc if sc is not None else torch.empty(w.shape[0], device=DEV), il)

    w = _bf(g, 64, 128)
    for f in (tile, quant):
        for bad in TENSOR_BAD.values():
            with pytest.raises(RuntimeError):
                f(bad(w))
        with pytest.raises(RuntimeError):
            f(w, _bf(g, 64))  # nw [K]
        with pytest.raises(RuntimeError):
            f(_bf(g, 64, 144))  # K % 32 / K % 64
    for N, il in ((24, False), (48, True)):  # N % 16; glu_il: N % 32
        with pytest.raises(RuntimeError):
            tile(_bf(g, N, 128), il=il)
    with pytest.raises(RuntimeError):
        quant(_bf(g, 48, 128))  # N % 32
    with pytest.raises(RuntimeError):
        tile(w, out=torch.empty(4, 4, 4, 16, 8, device=DEV, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        tile(w, out=torch.empty(4, 2, 4, 16, 8, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        quant(w, out=torch.empty(4, 1, 64, 16, device=DEV, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        quant(w, sc=torch.empty(63, device=DEV))
    with pytest.raises(RuntimeError):
        quant(w, sc=torch.empty(64, device=DEV, dtype=torch.float64))
