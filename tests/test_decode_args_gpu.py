"""Argument contract of the decode attention torch ops (csrc/bindings_decode.cpp): what
`decode_attn`, `decode_attn_group`, `decode_attn_rope`, `decode_attn_rope_group` and
`rope_cache_write` accept and what they refuse on the host, before any launch. Every refused call
raises before a kernel runs; the accepted ones use one tiny shape."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B, HQ, HKV, D, TMAX, ROT, G, TP, L = 4, 4, 2, 64, 128, 32, 2, 64, 100
OPS = ["decode_attn", "decode_attn_group", "decode_attn_rope", "decode_attn_rope_group"]
PLAIN, ROPE, GROUP = OPS[:2], OPS[2:], OPS[1::2]


@pytest.fixture(scope="module")
def C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def _tables(rot, rows=TMAX):
    """fp32 rope tables [rows, rot / 2] (empty at rot = 0)."""
    inv = 10000.0 ** (-torch.arange(0, rot, 2, device=DEV, dtype=torch.float32) / max(rot, 1))
    ang = torch.arange(rows, device=DEV, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _args(Hq=HQ, Hkv=HKV, d=D, rot=ROT):
    g = torch.Generator(device=DEV).manual_seed(0)
    bf = lambda *s: torch.randn(*s, device=DEV, generator=g).to(torch.bfloat16)  # noqa: E731
    a = dict(q=bf(B, Hq, d), qkv=bf(B, 1, (Hq + 2 * Hkv) * d), kc=bf(B, TMAX, Hkv, d), vc=bf(B, TMAX, Hkv, d),
             kv_len=torch.tensor([L], device=DEV, dtype=torch.int32),
             kv_start=torch.tensor([0, 0, 3, 3], device=DEV, dtype=torch.int32),
             pos=torch.full((B,), L - 1, device=DEV, dtype=torch.int32),
             slot=torch.tensor([L - 1], device=DEV, dtype=torch.long),
             Hq=Hq, Hkv=Hkv, D=d, rot=rot, G=G, Tp=TP)
    a["kc"][:, :TP] = a["kc"][[0, 0, 2, 2], :TP]  # the rows of a group share the prefix
    a["vc"][:, :TP] = a["vc"][[0, 0, 2, 2], :TP]
    a["cos"], a["sin"] = _tables(rot)
    return a


def _call(C, op, a):
    group = (a["G"], a["Tp"]) if op in GROUP else ()
    if op in PLAIN:
        return getattr(C, op)(a["q"], a["kc"], a["vc"], a["kv_len"], a["kv_start"], 0, a["D"] ** -0.5, *group)
    return getattr(C, op)(a["qkv"], a["cos"], a["sin"], a["pos"], a["kc"], a["vc"], a["slot"], a["kv_len"],
                          a["kv_start"], 0, a["D"] ** -0.5, a["Hq"], a["Hkv"], a["D"], a["rot"], *group)


def _offset4(t):
    """The same values behind a view that starts 4 elements (8 bytes) into its storage."""
    buf = torch.zeros(t.numel() + 8, device=DEV, dtype=t.dtype)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _f16_caches(a):
    a["kc"], a["vc"] = a["kc"].half(), a["vc"].half()


def _kv_len_i64(a):
    a["kv_len"] = a["kv_len"].long()


def _kv_start_b_plus_1(a):
    a["kv_start"] = torch.zeros(B + 1, device=DEV, dtype=torch.int32)


def _kv_start_i64(a):
    a["kv_start"] = a["kv_start"].long()


def _kv_strides_differ(a):  # head-major storage behind the same [B, Tmax, Hkv, D] view, v only
    a["vc"] = a["vc"].transpose(1, 2).contiguous().transpose(1, 2)


def _misaligned(a):
    a["kc"], a["vc"] = _offset4(a["kc"]), _offset4(a["vc"])


def _pos_short(a):
    a["pos"] = a["pos"][:B - 1].contiguous()


def _slot_i32(a):
    a["slot"] = a["slot"].int()


def _qkv_wide(a):
    a["qkv"] = torch.zeros(B, 1, (HQ + 2 * HKV) * D + D, device=DEV, dtype=torch.bfloat16)


ANY = [_f16_caches, _kv_len_i64, _kv_start_b_plus_1, _kv_start_i64, _kv_strides_differ, _misaligned]


@pytest.mark.parametrize("op", OPS)
def test_valid_call_returns_finite_output(C, op):
    o = _call(C, op, _args())
    torch.cuda.synchronize()
    assert o.shape == (B, HQ, D) and o.dtype == torch.bfloat16
    assert torch.isfinite(o.float()).all()


@pytest.mark.parametrize("bad", ANY, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("op", OPS)
def test_every_op_refuses(C, op, bad):
    a = _args()
    bad(a)
    with pytest.raises(RuntimeError):
        _call(C, op, a)


@pytest.mark.parametrize("shape", [dict(d=32), dict(Hq=6, Hkv=2), dict(Hq=3, Hkv=2)],
                         ids=["D32", "ratio3", "Hq3Hkv2"])
@pytest.mark.parametrize("op", PLAIN)
def test_prerotated_ops_refuse_head_geometry(C, op, shape):
    with pytest.raises(RuntimeError):
        _call(C, op, _args(rot=min(ROT, shape.get("d", D)), **shape))


@pytest.mark.parametrize("rot", [0, 8, D + 16])
@pytest.mark.parametrize("op", ROPE)
def test_rope_ops_refuse_rot(C, op, rot):
    with pytest.raises(RuntimeError):
        _call(C, op, _args(rot=rot))  # tables sized for this rot: it is rot itself that is refused


@pytest.mark.parametrize("bad", [_pos_short, _slot_i32, _qkv_wide], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("op", ROPE)
def test_rope_ops_refuse_rope_step_arguments(C, op, bad):
    a = _args()
    bad(a)
    with pytest.raises(RuntimeError):
        _call(C, op, a)


@pytest.mark.parametrize("op", GROUP)
def test_group_ops_refuse_group_arguments(C, op):
    a = _args()
    a["G"] = 3
    with pytest.raises(RuntimeError, match="group_size"):
        _call(C, op, a)
    for tp in (0, TMAX + 1):
        a = _args()
        a["Tp"] = tp
        with pytest.raises(RuntimeError, match="prefix_len"):
            _call(C, op, a)


def _rope_write(C, a):
    return C.rope_cache_write(a["qkv"], a["cos"], a["sin"], a["pos"], a["kc"], a["vc"], a["slot"], a["Hq"],
                              a["Hkv"], a["D"], a["rot"])


@pytest.mark.parametrize("d,rot", [(80, 32), (80, 0), (D, 0)])
def test_rope_cache_write_accepts_partial_and_no_rotary(C, d, rot):
    a = _args(d=d, rot=rot)
    q = _rope_write(C, a)
    torch.cuda.synchronize()
    assert q.shape == (B, HQ, d) and torch.isfinite(q.float()).all()
    rows = a["qkv"].view(B, HQ + 2 * HKV, d)
    assert torch.equal(q[..., rot:], rows[:, :HQ, rot:])  # dims past `rot` pass through
    assert torch.equal(a["kc"][:, L - 1, :, rot:], rows[:, HQ:HQ + HKV, rot:])
    assert torch.equal(a["vc"][:, L - 1], rows[:, HQ + HKV:])


def test_rope_cache_write_refuses_rot_8(C):
    with pytest.raises(RuntimeError):
        _rope_write(C, _args(rot=8))
