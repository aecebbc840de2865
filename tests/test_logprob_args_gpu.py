"""Argument contract of the 15 LM-head log-prob torch ops (csrc/bindings_logprob.cpp): what they
refuse on the host, before any launch. Every refused call raises before a kernel runs, so an in-place
op leaves `logits` bit for bit untouched; the accepted calls use one tiny shape (N = 8, V = 64)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N, V, IT = 8, 64, 0.7

# op -> (kind, variant, entropy)
OPS = {
    "logprob_fwd": ("fwd", "plain", False),
    "logprob_bwd": ("bwd", "plain", False),
    "logprob_bwd_t": ("bwd_t", "plain", False),
    "logprob_entropy_fwd": ("fwd", "plain", True),
    "logprob_entropy_bwd": ("bwd", "plain", True),
    "logprob_entropy_bwd_t": ("bwd_t", "plain", True),
    "logprob_fwd_temp": ("fwd", "temp", False),
    "logprob_bwd_temp": ("bwd", "temp", False),
    "logprob_bwd_t_temp": ("bwd_t", "temp", False),
    "logprob_fwd_keep": ("fwd", "keep", False),
    "logprob_bwd_keep": ("bwd", "keep", False),
    "logprob_bwd_t_keep": ("bwd_t", "keep", False),
    "logprob_entropy_fwd_temp": ("fwd", "temp", True),
    "logprob_entropy_bwd_temp": ("bwd", "temp", True),
    "logprob_entropy_bwd_t_temp": ("bwd_t", "temp", True),
}
ALL = list(OPS)
BACKWARD = [o for o in ALL if OPS[o][0] != "fwd"]
BWD_T = [o for o in ALL if OPS[o][0] == "bwd_t"]
WITH_INV_TEMP = [o for o in ALL if OPS[o][1] != "plain"]
KEEP = [o for o in ALL if OPS[o][1] == "keep"]


@pytest.fixture(scope="module")
def C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def _args(n=N, v=V):
    g = torch.Generator(device=DEV).manual_seed(0)
    logits = (3 * torch.randn(n, v, device=DEV, generator=g)).to(torch.bfloat16)
    f32 = lambda: torch.randn(n, device=DEV, generator=g)  # noqa: E731
    return dict(logits=logits, targets=torch.arange(n, device=DEV) % v,
                lse=torch.logsumexp(logits.float() * IT, -1), ent=f32().abs(), grad=f32(), grad_ent=f32(),
                keep=torch.full((n, v // 8), 0xFF, device=DEV, dtype=torch.uint8),
                keep_rows=torch.arange(n, device=DEV), inv_temp=IT)


def _rows(op):
    """The per-row fp32 vectors `op` takes, in argument order."""
    kind, _, entropy = OPS[op]
    if kind == "fwd":
        return []
    return ["lse", "ent", "grad", "grad_ent"] if entropy else ["lse", "grad"]


def _call(C, op, a):
    variant = OPS[op][1]
    tail = {"plain": [], "temp": ["inv_temp"], "keep": ["keep", "keep_rows", "inv_temp"]}[variant]
    return getattr(C, op)(*[a[k] for k in ["logits", "targets"] + _rows(op) + tail])


def _refused(C, op, a):
    before = a["logits"].clone()
    with pytest.raises(RuntimeError):
        _call(C, op, a)
    assert torch.equal(a["logits"], before)  # nothing launched


@pytest.mark.parametrize("op", ALL)
def test_accepted(C, op):
    """The calls the cases below spoil, unspoiled: they run, and the backwards rewrite the logits."""
    a = _args()
    before = a["logits"].clone()
    kind, variant, entropy = OPS[op]
    if variant == "plain":
        a["lse"] = torch.logsumexp(before.float(), -1)
    out = _call(C, op, a)
    if kind == "fwd":
        assert len(out) == (3 if entropy else 2) and all(o.shape == (N,) and o.dtype == torch.float32 for o in out)
        assert torch.equal(a["logits"], before)
    else:
        assert not torch.equal(a["logits"], before)
        if kind == "bwd_t":
            assert out.shape == (V, N) and torch.equal(out, a["logits"].t())


@pytest.mark.parametrize("op", BACKWARD)
def test_strided_row_vector(C, op):
    for name in _rows(op):
        a = _args()
        wide = torch.zeros(2 * N, device=DEV)
        wide[::2] = a[name]
        a[name] = wide[::2]
        assert a[name].numel() == N and not a[name].is_contiguous()
        _refused(C, op, a)


@pytest.mark.parametrize("op", BACKWARD)
def test_row_vector_dtype_and_length(C, op):
    for name in _rows(op):
        for spoil in (lambda t: t.double(), lambda t: t.half(), lambda t: t[:N - 1].contiguous(),
                      lambda t: torch.cat([t, t[:1]])):
            a = _args()
            a[name] = spoil(a[name])
            _refused(C, op, a)


@pytest.mark.parametrize("op", ALL)
def test_cpu_targets(C, op):
    a = _args()
    a["targets"] = a["targets"].cpu()
    _refused(C, op, a)


@pytest.mark.parametrize("op", WITH_INV_TEMP)
def test_inv_temp_range(C, op):
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        a = _args()
        a["inv_temp"] = bad
        _refused(C, op, a)


@pytest.mark.parametrize("op", KEEP)
def test_keep_width(C, op):
    for width in (V // 8 - 1, V // 8 + 1, V):
        a = _args()
        a["keep"] = torch.full((N, width), 0xFF, device=DEV, dtype=torch.uint8)
        _refused(C, op, a)


@pytest.mark.parametrize("op", BWD_T)
def test_bwd_t_outside_its_shapes_returns_empty(C, op):
    """N = 12 (not a multiple of 8) and V = 60 (neither V nor the row stride is): an empty tensor, and
    nothing written. The keep ops refuse V = 60 outright: their mask is a byte per 8 entries."""
    for n, v in ((12, V), (N, 60)):
        a = _args(n, v)
        if v % 8:
            a["keep"] = torch.full((n, 8), 0xFF, device=DEV, dtype=torch.uint8)
            if op in KEEP:
                _refused(C, op, a)
                continue
        before = a["logits"].clone()
        out = _call(C, op, a)
        assert out.numel() == 0
        assert torch.equal(a["logits"], before)
