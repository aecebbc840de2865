"""Argument contract of the training attention torch ops (csrc/bindings_attention.cpp): what
`attn_fwd`, `attn_bwd` and `attn_fwd_switch` accept and what they refuse on the host. The accepted
calls use one tiny shape (each optional operand on and off, strided views of a fused buffer) and
must match `ops.attention.ref_attention` at the tolerance of test_kernels_gpu.py (relative L2 error
2e-2 forward, 3e-2 backward, every head dim). Every refused call must raise before anything is
written: a sentinel in q_rot (forward) and in dq / dk / dv (backward) stays as it was.

Not tested: the refusals of B, Hq, Hkv, Tq, Tk or a planned grid of 2^31 and more, whose operands
are too large to allocate here."""
import pytest
import torch

from distributed_llm_alignment_amd.ops.attention import _qkv_views, _ref_rope, ref_attention

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B, T, HQ, HKV, ROWS = 2, 40, 4, 2, 64
BTHD_FWD = ["q", "k", "v", "q_rot"]
BTHD_BWD = ["dout", "q", "k", "v", "o", "dq", "dk", "dv"]
OTHER = ["kv_start", "kv_end", "segs", "cos", "sin", "pos"]


@pytest.fixture(scope="module")
def C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def rel_err(a, b):  # as test_kernels_gpu.py
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _tables(half, rows=ROWS):
    inv = 10000.0 ** (-torch.arange(0, half, device=DEV, dtype=torch.float32) / half)
    ang = torch.arange(rows, device=DEV, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _args(D=64, half=None, Tq=T, Hkv=HKV, fused=False):
    """Every operand of both ops, all optional ones present; a call passes the names it wants."""
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()  # noqa: E731
    i32 = lambda x: torch.tensor(x, device=DEV, dtype=torch.int32)  # noqa: E731
    if fused:  # q / k / v column slices of one [B, T, C] buffer, dq / dk / dv of one dqkv
        q, k, v = _qkv_views(rn(B, T, (HQ + 2 * Hkv) * D), HQ, Hkv, D)
        dq, dk, dv = _qkv_views(torch.empty(B, T, (HQ + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16), HQ, Hkv, D)
    else:
        q, k, v = rn(B, Tq, HQ, D), rn(B, T, Hkv, D), rn(B, T, Hkv, D)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    st = torch.zeros(B, Tq, dtype=torch.int32, device=DEV)
    st[:, 17:] = 17  # two packed sequences per row: [0, 17) and [17, T)
    en = torch.where(st == 0, 17, Tq).int()
    a = dict(q=q, k=k, v=v, dout=rn(B, Tq, HQ, D), o=torch.zeros(B, Tq, HQ, D, device=DEV, dtype=torch.bfloat16),
             lse2=torch.zeros(B, HQ, Tq, device=DEV), dq=dq, dk=dk, dv=dv, q_rot=torch.empty_like(q),
             kv_start=i32([0, 3]), kv_end=i32([T, 33]), segs=torch.stack([st, en]).contiguous(),
             prefix=i32([[0, 17, Tq]] * B), pos=(torch.arange(B * Tq, device=DEV) % Tq).int(), D=D, causal=True,
             causal_off=T - Tq, window=0, rope_k=True, rope_inputs=False)
    a["cos"], a["sin"] = _tables(D // 2 if half is None else half)
    return a


def _fwd(C, a, use=()):
    t = lambda n: a[n] if n in use else None  # noqa: E731
    return C.attn_fwd(a["q"], a["k"], a["v"], a["D"] ** -0.5, a["causal"], a["causal_off"], a["window"],
                      t("kv_start"), t("kv_end"), t("segs"), t("cos"), t("sin"), t("pos"), t("q_rot"), a["rope_k"],
                      t("prefix"))


def _bwd(C, a, use=()):
    t = lambda n: a[n] if n in use else None  # noqa: E731
    return C.attn_bwd(a["dout"], a["q"], a["k"], a["v"], a["o"], a["lse2"], a["dq"], a["dk"], a["dv"], a["D"] ** -0.5,
                      a["causal"], a["causal_off"], a["window"], t("kv_start"), t("kv_end"), t("segs"), t("cos"),
                      t("sin"), t("pos"), a["rope_inputs"])


# ------------------------------------------------------------------------------------ accepted
def _reference(a, use, rot):
    """fp32 o and the gradients with respect to the un-rotated q, k, v, on the bf16 operands."""
    t = lambda n: a[n] if n in use else None  # noqa: E731
    q, k, v = (a[n].detach().float().requires_grad_() for n in ("q", "k", "v"))
    qr, kr = q, k
    if rot:
        pos = (a["pos"] if "pos" in use else torch.arange(T, device=DEV).repeat(B)).view(B, T).long()
        qr, kr = (_ref_rope(x, a["cos"], a["sin"], pos, rot) for x in (q, k))
    o = ref_attention(qr, kr, v, a["D"] ** -0.5, a["causal"], a["causal_off"], a["window"], t("kv_start"),
                      t("kv_end"), t("segs"), t("prefix"))
    return (o, qr, kr) + torch.autograd.grad(o, [q, k, v], a["dout"].float())


ACCEPTED = {  # name: (optional operands passed, D, table half width, changes to the scalars)
    "plain": ((), 64, None, {}),
    "noncausal": ((), 64, None, {"causal": False}),
    "window": ((), 64, None, {"window": 9}),
    "kv_start": (("kv_start",), 64, None, {}),
    "kv_end": (("kv_end",), 64, None, {}),
    "segs": (("segs",), 64, None, {}),
    "prefix": (("segs", "prefix"), 64, None, {}),
    "rope": (("cos", "sin"), 64, None, {}),
    "rope_pos_q_rot": (("cos", "sin", "pos", "q_rot"), 64, None, {}),
    "rope_q_only": (("cos", "sin", "q_rot"), 64, None, {"rope_k": False}),
    "fused_views": ((), 64, None, {"fused": True}),
    "all_D128": (("kv_start", "kv_end", "segs", "cos", "sin", "pos", "q_rot"), 128, None, {}),
    "partial_rotary_D80": (("cos", "sin"), 80, 16, {}),
}


@pytest.mark.parametrize("name", ACCEPTED)
def test_accepted_calls_match_the_reference(C, name):
    """Forward, then the backward on its o / lse2 with the same optional operands: with tables the
    backward reads the rotated q (q_rot, or rotated here) and returns un-rotated dq / dk; with
    rope_k the forward's k is un-rotated and the backward rotates it again (rope_inputs). D = 80
    has no RoPE on load: the forward gets rotated q / k, the backward the [64, 16] tables."""
    use, D, half, ch = ACCEPTED[name]
    a = _args(D=D, half=half, fused=ch.get("fused", False))
    a.update({k: v for k, v in ch.items() if k != "fused"})
    rope = "cos" in use
    rot = 2 * a["cos"].shape[1] if rope else 0
    ro, qr, kr, rq, rk, rv = _reference(a, use, rot)
    k_in = a["k"]
    on_load = rope and D != 80
    if rope and not (on_load and a["rope_k"]):
        a["k"] = kr.detach().bfloat16()
    if rope and not on_load:
        a["q"] = qr.detach().bfloat16()
    o, lse2 = _fwd(C, a, [n for n in use if on_load or n not in ("cos", "sin", "pos")])
    valid = torch.ones(B, T, 1, 1, dtype=torch.bool, device=DEV)
    if "kv_start" in use:
        valid[1, :3] = False  # queries in front of their row's first key see nothing
    assert rel_err(o * valid, ro * valid) < 2e-2, "forward"
    if "q_rot" in use:
        assert rel_err(a["q_rot"], qr) < 1e-2, "q_rot"
    a["o"], a["lse2"] = o, lse2
    if rope:  # the backward reads the rotated q; k rotated here, or un-rotated with rope_inputs
        a["q"] = a["q_rot"] if "q_rot" in use else qr.detach().bfloat16()
        a["rope_inputs"] = bool(on_load and a["rope_k"])
        a["k"] = k_in if a["rope_inputs"] else kr.detach().bfloat16()
    for n in ("dq", "dk", "dv"):
        a[n].fill_(float("nan"))
    if "prefix" in use:  # the backward form of the mask: the prefix keys [0, 17) are seen up to qe = T
        a["segs"] = torch.stack([a["segs"][0], torch.full_like(a["segs"][1], T)]).contiguous()
    _bwd(C, a, [n for n in use if n not in ("q_rot", "prefix")])
    torch.cuda.synchronize()
    assert rel_err(a["dq"] * valid, rq * valid) < 3e-2, "dq"
    assert rel_err(a["dk"], rk) < 3e-2, "dk"
    assert rel_err(a["dv"], rv) < 3e-2, "dv"


# ------------------------------------------------------------------------------------- refused
def _dtype(x):
    return x.double() if x.dtype == torch.float32 else x.half() if x.dtype == torch.bfloat16 else x.long()


def _cpu(x):
    return x.cpu()


def _d_stride(x):  # every other element of a twice as wide last dim
    return torch.zeros(*x.shape[:-1], 2 * x.shape[-1], device=DEV, dtype=x.dtype)[..., ::2]


def _stride_not_8(x):  # token rows 4 elements further apart than H * D
    b, t, h, d = x.shape
    row = h * d + 4
    return torch.zeros(b * t * row, device=DEV, dtype=x.dtype).as_strided((b, t, h, d), (t * row, row, d, 1))


def _offset_8_bytes(x):
    buf = torch.zeros(x.numel() + 8, device=DEV, dtype=x.dtype)
    return buf[4:4 + x.numel()].view(x.shape)


def _other_gpu(x):
    return x.to("cuda:1")


def _set(name, f):
    def bad(a):
        a[name] = f(a[name])
    bad.__name__ = f"{name}-{f.__name__.strip('_')}"
    return bad


def _put(**kw):
    def bad(a):
        a.update({k: (v(a) if callable(v) else v) for k, v in kw.items()})
    return bad


ALL = ("kv_start", "kv_end", "segs", "cos", "sin", "pos")
ROPE = ("cos", "sin")
BTHD_RULES = [_dtype, _cpu, _d_stride, _stride_not_8, _offset_8_bytes]
# name: (args of _args, optional operands passed, the change that must be refused)
SHARED = {
    "D96": (dict(D=96), (), _put()),
    "Hq_not_multiple_of_Hkv": (dict(Hkv=3), (), _put()),
    "v_shorter_than_k": ({}, (), _put(v=lambda a: a["v"][:, :32].contiguous(), dv=lambda a: a["dv"][:, :32].contiguous())),
    "kv_start_int64": ({}, ("kv_start",), _set("kv_start", _dtype)),
    "kv_start_B_plus_1": ({}, ("kv_start",), _put(kv_start=lambda a: torch.zeros(B + 1, dtype=torch.int32, device=DEV))),
    "segs_wrong_shape": ({}, ("segs",), _put(segs=lambda a: a["segs"][:, :, :T - 1].contiguous())),
    "segs_noncausal": ({}, ("segs",), _put(causal=False)),
    "segs_Tq_not_Tk": (dict(Tq=32), ("segs",), _put(causal_off=0)),
    "rope_sin_missing": ({}, ("cos",), _put()),
    "rope_table_width": (dict(half=16), ROPE, _put()),
    "rope_Tq_not_Tk": (dict(Tq=32), ROPE, _put(causal_off=0)),
    "T_beyond_table": ({}, ROPE, _put(cos=lambda a: a["cos"][:32].contiguous(), sin=lambda a: a["sin"][:32].contiguous())),
    "rope_pos_numel": ({}, ROPE + ("pos",), _put(pos=lambda a: a["pos"][:-1].contiguous())),
}
FWD_ONLY = {
    "prefix_without_segs": ({}, ("prefix",), _put()),
    "prefix_with_window": ({}, ("segs", "prefix"), _put(window=8)),
    "prefix_wrong_shape": ({}, ("segs", "prefix"), _put(prefix=lambda a: a["prefix"][:, :2].contiguous())),
    "rope_at_D80": (dict(D=80), ROPE, _put()),
    "q_rot_without_tables": ({}, ("q_rot",), _put()),
    "q_rot_wrong_shape": ({}, ROPE + ("q_rot",), _put(q_rot=lambda a: torch.empty_like(a["q"][:, :, :2]))),
}
BWD_ONLY = {
    "lse2_numel": ({}, (), _put(lse2=lambda a: a["lse2"][:, :, :-1].contiguous())),
    "k_batch_differs": ({}, (), _put(k=lambda a: a["k"][:1], v=lambda a: a["v"][:1], dk=lambda a: a["dk"][:1],
                                     dv=lambda a: a["dv"][:1])),
    "rope_inputs_without_tables": ({}, (), _put(rope_inputs=True)),
    "rope_inputs_partial_rotary": (dict(D=80, half=16), ROPE, _put(rope_inputs=True)),
    **{f"{n}_shape": ({}, (), _put(**{n: (lambda n: lambda a: a[n][:, :, :1].contiguous())(n)}))
       for n in ("dout", "o", "dq", "dk", "dv")},
}


def _refused(C, call, a, use, outs):
    for n in outs:
        a[n].fill_(7.0)
    with pytest.raises(RuntimeError):
        call(C, a, use)
    torch.cuda.synchronize()
    for n in outs:
        assert bool((a[n] == 7.0).all()), f"{n} was written by a refused call"


@pytest.mark.parametrize("rule", BTHD_RULES, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("name", BTHD_FWD)
def test_attn_fwd_refuses_a_bad_bthd_operand(C, name, rule):
    a = _args()
    a[name] = rule(a[name])
    _refused(C, _fwd, a, ROPE + ("q_rot",), ["q_rot"])


@pytest.mark.parametrize("rule", BTHD_RULES, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("name", BTHD_BWD)
def test_attn_bwd_refuses_a_bad_bthd_operand(C, name, rule):
    a = _args()
    a[name] = rule(a[name])
    _refused(C, _bwd, a, (), ["dq", "dk", "dv"])


@pytest.mark.parametrize("rule", [_dtype, _cpu], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("name", OTHER + ["prefix", "lse2"])
def test_both_ops_refuse_a_bad_index_or_table_operand(C, name, rule):
    a = _args()
    a[name] = rule(a[name])
    if name != "lse2":
        _refused(C, _fwd, a, ALL + ("q_rot",) + (("prefix",) if name == "prefix" else ()), ["q_rot"])
    if name != "prefix":
        _refused(C, _bwd, a, ALL, ["dq", "dk", "dv"])


@pytest.mark.parametrize("name", list(SHARED) + list(FWD_ONLY))
def test_attn_fwd_refuses(C, name):
    kw, use, bad = {**SHARED, **FWD_ONLY}[name]
    a = _args(**kw)
    bad(a)
    _refused(C, _fwd, a, use, ["q_rot"])


@pytest.mark.parametrize("name", list(SHARED) + list(BWD_ONLY))
def test_attn_bwd_refuses(C, name):
    kw, use, bad = {**SHARED, **BWD_ONLY}[name]
    a = _args(**kw)
    bad(a)
    _refused(C, _bwd, a, use, ["dq", "dk", "dv"])


def test_attn_fwd_switch_refuses_an_unknown_name(C):
    with pytest.raises(RuntimeError, match="unknown switch"):
        C.attn_fwd_switch("nosuch", 1)
    prev = C.attn_fwd_switch("msub", 1)
    assert C.attn_fwd_switch("msub", prev) == 1


@pytest.mark.parametrize("name", BTHD_FWD + OTHER + ["prefix"])
def test_attn_fwd_refuses_an_operand_on_another_gpu(C, name):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    a = _args()
    a[name] = _other_gpu(a[name])
    use = ALL + ("q_rot",)
    _refused(C, _fwd, a, (("segs", "prefix") if name == "prefix" else use), ["q_rot"])


@pytest.mark.parametrize("name", BTHD_BWD + OTHER + ["lse2"])
def test_attn_bwd_refuses_an_operand_on_another_gpu(C, name):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    a = _args()
    a[name] = _other_gpu(a[name])
    _refused(C, _bwd, a, ALL, ["dq", "dk", "dv"])
