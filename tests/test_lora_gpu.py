"""GPU tier: the LoRA kernels of csrc/lora.hip (lora_shrink, lora_expand_add_) and the
`ops.lora.lora_linear` autograd function. Every launch runs twice and the bits must be equal.

Exact-integer cases (see _refs64_lora): the kernel output equals the fp64 result bitwise, for both
ops, both small-operand layouts and every rank.

Random cases against fp64 with `_refs64.check(..., bf16=True)`:
  E32   = error of the un-rounded fp32 CPU composition on the same bf16 inputs,
  extra = gamma_K sum_k |x_k| |a_k| (K terms summed in another order; `_refs64_lora.dot_extra`,
          derived there, never measured), times the scale the kernel applies to the sum.

Gradients: t and dts = bf16(s dy B) enter the fp64 gradient formulas as the bf16 values the op
produced (each is checked against fp64 on its own), and dx0 = dy W as the bf16 tensor the base
input-gradient GEMM returned, exactly as y0 enters the forward: the check is on what the adapter
adds, and a last-bit flip in an intermediate cannot fail it.
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext
from distributed_llm_alignment_amd.ops import lora as L
from distributed_llm_alignment_amd.ops.linear import input_grad

import _refs64 as R
import _refs64_lora as RL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
RANKS = [8, 16, 32, 64]
MS = [1, 15, 16, 17, 33, 250]
KS = [8, 40, 64, 264]
NS = [8, 24, 136]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _shrink2(x, a, scale, transposed=False):
    n0 = L.CALLS["shrink_kernel"]
    t1 = L.lora_shrink(x, a, scale, transposed=transposed, force_kernel=True)
    t2 = L.lora_shrink(x, a, scale, transposed=transposed, force_kernel=True)
    assert L.CALLS["shrink_kernel"] == n0 + 2, "the HIP kernel did not serve this call"
    assert _same_bits(t1, t2), "two launches differ"
    return t1


def _expand2(y0, t, b, scale=1.0, transposed=False):
    assert L.expand_ok(y0, t, b, transposed)
    y1, y2 = y0.clone(), y0.clone()
    n0 = L.CALLS["expand_kernel"]
    L.lora_expand_add_(y1, t, b, scale, transposed=transposed, force_kernel=True)
    L.lora_expand_add_(y2, t, b, scale, transposed=transposed, force_kernel=True)
    assert L.CALLS["expand_kernel"] == n0 + 2, "the HIP kernel did not serve this call"
    assert _same_bits(y1, y2), "two launches differ"
    return y1


# ------------------------------------------------------------------------------ exact integers
@pytest.mark.parametrize("R_", RANKS)
def test_shrink_exact_integers(R_):
    _ext.require()
    for M in (1, 17, 250):
        for K in (8, 40, 64):
            for scale in (1.0, 0.5):
                x, a = RL.exact_shrink_case(M, K, R_, seed=M + K)
                ref = RL.shrink64(x, a, scale)
                assert ref.abs().max() <= 128
                got = _shrink2(x.to(DEV), a.to(DEV), scale)
                assert torch.equal(got.cpu().to(RL.F64), ref), f"shrink M={M} K={K} R={R_} scale={scale}"
                # the other layout: the small operand handed over as [K, R]
                got_t = _shrink2(x.to(DEV), a.t().contiguous().to(DEV), scale, transposed=True)
                assert torch.equal(got_t.cpu().to(RL.F64), ref), f"shrink^T M={M} K={K} R={R_}"


@pytest.mark.parametrize("R_", RANKS)
def test_expand_exact_integers(R_):
    _ext.require()
    for M in (1, 17, 250):
        for N in NS:
            y0, t, b = RL.exact_expand_case(M, N, R_, seed=M + N)
            ref = RL.expand64(y0, t, b)
            assert ref.abs().max() <= 192
            got = _expand2(y0.to(DEV), t.to(DEV), b.to(DEV))
            assert torch.equal(got.cpu().to(RL.F64), ref), f"expand M={M} N={N} R={R_}"
            got_t = _expand2(y0.to(DEV), t.to(DEV), b.t().contiguous().to(DEV), transposed=True)
            assert torch.equal(got_t.cpu().to(RL.F64), ref), f"expand [R, N] M={M} N={N} R={R_}"


# ------------------------------------------------------------------------------ random vs fp64
def _check_shrink(x, a, scale, got, name):
    ref = RL.shrink64(x, a, scale)
    e32 = R.e32_of(float(scale) * (x.float() @ a.float().t()), ref)
    extra = abs(scale) * RL.dot_extra(x.shape[1], RL.abs_dot_max(x, a))
    R.check("lora_shrink", name, got, ref, e32, extra, bf16=True)


def _check_expand(y0, t, b, got, name, scale=1.0):
    ref = RL.expand64(y0, t, b, scale)
    e32 = R.e32_of(y0.float() + float(scale) * (t.float() @ b.float().t()), ref)
    extra = abs(scale) * RL.dot_extra(t.shape[1], RL.abs_dot_max(t, b))
    R.check("lora_expand_add_", name, got, ref, e32, extra, bf16=True)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("R_", RANKS)
def test_shrink_random(M, R_):
    for K in KS:
        x, a = RL.shrink_case(M, K, R_, seed=M * 1000 + K)
        got = _shrink2(x.to(DEV), a.to(DEV), 2.0)
        _check_shrink(x, a, 2.0, got, f"M{M} K{K} R{R_}")


@pytest.mark.parametrize("R_", RANKS)
def test_shrink_split_k(R_):
    """K = 4096: every wave of the block owns k-steps and the LDS reduction sums all eight."""
    x, a = RL.shrink_case(64, 4096, R_, seed=5)
    got = _shrink2(x.to(DEV), a.to(DEV), 0.25)
    _check_shrink(x, a, 0.25, got, f"M64 K4096 R{R_}")
    at = a.t().contiguous().to(DEV)  # [K, R]: through the cached transposed copy
    got_t = _shrink2(x.to(DEV), at, 0.25, transposed=True)
    assert _same_bits(got, got_t)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("R_", RANKS)
def test_expand_random(M, R_):
    for N in NS:
        y0, t, b = RL.expand_case(M, N, R_, seed=M * 1000 + N)
        got = _expand2(y0.to(DEV), t.to(DEV), b.to(DEV))
        _check_expand(y0, t, b, got, f"M{M} N{N} R{R_}")
        got_t = _expand2(y0.to(DEV), t.to(DEV), b.t().contiguous().to(DEV), transposed=True)
        assert _same_bits(got, got_t), "the [R, N] layout gives other bits"
    y0, t, b = RL.expand_case(M, 136, R_, seed=M + 3)
    got = _expand2(y0.to(DEV), t.to(DEV), b.to(DEV), scale=0.5)
    _check_expand(y0, t, b, got, f"M{M} N136 R{R_} scale0.5", scale=0.5)


def test_expand_many_blocks():
    """More than one block along both grid axes (256 tokens and 64 columns per block)."""
    y0, t, b = RL.expand_case(530, 200, 16, seed=9)
    got = _expand2(y0.to(DEV), t.to(DEV), b.to(DEV))
    _check_expand(y0, t, b, got, "M530 N200 R16")


# ------------------------------------------------------------------------------ views, fallbacks
def test_strided_x():
    x, a = RL.shrink_case(33, 40, 16, seed=21)
    wide = torch.zeros(33, 96, dtype=BF16)
    wide[:, 16:56] = x
    xv = wide.to(DEV)[:, 16:56]
    assert xv.stride(0) == 96 and not xv.is_contiguous()
    got = _shrink2(xv, a.to(DEV), 2.0)
    assert _same_bits(got, _shrink2(x.to(DEV), a.to(DEV), 2.0))
    _check_shrink(x, a, 2.0, got, "strided x")


def _nan_buf(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=BF16, device=DEV)


def test_views_in_nan_buffers():
    """x, a, t, b and y as views inside NaN-filled buffers: finite outputs, and every sentinel
    outside the views keeps its bits (the tails are zero-filled in registers, never loaded)."""
    M, K, N, R_ = 17, 40, 24, 8
    x, a = RL.shrink_case(M, K, R_, seed=31)
    y0, _, b = RL.expand_case(M, N, R_, seed=32)
    xb, ab = _nan_buf(M + 4, K + 24), _nan_buf(R_ + 3, K + 16)
    xb[2:2 + M, 8:8 + K] = x.to(DEV)
    ab[1:1 + R_, 8:8 + K] = a.to(DEV)
    t = _shrink2(xb[2:2 + M, 8:8 + K], ab[1:1 + R_, 8:8 + K], 2.0)
    assert torch.isfinite(t.float()).all()
    _check_shrink(x, a, 2.0, t, "nan-buffer views")
    tb, bb, yb = _nan_buf(M + 2, R_ + 16), _nan_buf(N + 2, R_ + 8), _nan_buf(M + 3, N + 16)
    tb[1:1 + M, 8:8 + R_] = t
    bb[1:1 + N, 0:R_] = b.to(DEV)
    yb[2:2 + M, 8:8 + N] = y0.to(DEV)
    before = _bits(yb).clone()
    yv = yb[2:2 + M, 8:8 + N]
    assert L.expand_ok(yv, tb[1:1 + M, 8:8 + R_], bb[1:1 + N, 0:R_])
    L.lora_expand_add_(yv, tb[1:1 + M, 8:8 + R_], bb[1:1 + N, 0:R_], force_kernel=True)
    torch.cuda.synchronize()
    assert torch.isfinite(yv.float()).all()
    _check_expand(y0, t.cpu(), b, yv, "nan-buffer views")
    outside = torch.ones_like(before, dtype=torch.bool)
    outside[2:2 + M, 8:8 + N] = False
    assert torch.equal(_bits(yb)[outside], before[outside]), "a sentinel outside the y view changed"
    # the [R, N] layout as a view (2-byte loads: any row stride)
    bt = _nan_buf(R_ + 2, N + 3)
    bt[1:1 + R_, 1:1 + N] = b.t().to(DEV)
    y2 = y0.to(DEV)
    L.lora_expand_add_(y2, t, bt[1:1 + R_, 1:1 + N], transposed=True, force_kernel=True)
    assert L.expand_ok(y2, t, bt[1:1 + R_, 1:1 + N], True)
    assert _same_bits(y2, yv.contiguous())


def test_ineligible_takes_composition():
    # K % 8 != 0
    x, a = RL.shrink_case(17, 44, 16, seed=41)
    assert not L.shrink_ok(x.to(DEV), a.to(DEV))
    got = L.lora_shrink(x.to(DEV), a.to(DEV), 2.0)
    assert _same_bits(got, L.shrink_composition(x.to(DEV), a.to(DEV), 2.0))
    # a misaligned base (4 elements = 8 bytes into a row)
    x, a = RL.shrink_case(17, 40, 16, seed=42)
    wide = torch.zeros(17, 48, dtype=BF16, device=DEV)
    xv = wide[:, 4:44]
    xv.copy_(x.to(DEV))
    assert xv.data_ptr() % 16 == 8 and not L.shrink_ok(xv, a.to(DEV))
    got = L.lora_shrink(xv, a.to(DEV), 2.0)
    assert _same_bits(got, L.shrink_composition(xv, a.to(DEV), 2.0))
    _check_shrink(x, a, 2.0, got, "misaligned x (composition)")
    # a rank outside the kernel set, and N % 8 != 0
    y0, t, b = RL.expand_case(9, 20, 24, seed=43)
    assert not L.expand_ok(y0.to(DEV), t.to(DEV), b.to(DEV))
    y = y0.to(DEV)
    L.lora_expand_add_(y, t.to(DEV), b.to(DEV))
    assert _same_bits(y, L.expand_add_composition(y0.to(DEV), t.to(DEV), b.to(DEV)))


# ------------------------------------------------------------------------------ lora_linear
def _dev_case(c, mg_dtype=None):
    out = {k: (v.to(DEV) if v is not None else None) for k, v in c.items()}
    out["w"].requires_grad_(False)
    for k in ("a", "b"):
        out[k] = torch.nn.Parameter(out[k])
        if mg_dtype is not None:
            out[k].main_grad = torch.zeros(out[k].shape, dtype=mg_dtype, device=DEV)
    return out


def _by_hand(g, scale):
    x, w = g["x"], g["w"]
    if g["resid"] is not None:
        y = ops.linear_add(x, w, g["resid"])
    else:
        y = ops.linear(x, w, g["bias"])
    t = L.lora_shrink(x, g["a"].detach(), scale)
    L.lora_expand_add_(y, t, g["b"].detach())
    return y, t


@pytest.mark.parametrize("mode", ["plain", "bias", "resid"])
def test_lora_linear_forward(mode):
    scale = 2.0
    c = RL.full_case(250, 264, 136, 16, seed=3, with_bias=mode == "bias", with_resid=mode == "resid")
    g = _dev_case(c)
    with torch.no_grad():
        want, t = _by_hand(g, scale)
    y1 = L.lora_linear(g["x"], g["w"], g["a"], g["b"], scale, bias=g["bias"], resid=g["resid"])
    y2 = L.lora_linear(g["x"], g["w"], g["a"], g["b"], scale, bias=g["bias"], resid=g["resid"])
    assert _same_bits(y1, y2) and _same_bits(y1, want), "forward differs from the three pieces by hand"
    # B == 0: the base projection bit for bit
    with torch.no_grad():
        zero_b = torch.zeros_like(g["b"])
        base = ops.linear_add(g["x"], g["w"], g["resid"]) if mode == "resid" else ops.linear(g["x"], g["w"], g["bias"])
    y0 = L.lora_linear(g["x"], g["w"], g["a"], zero_b, scale, bias=g["bias"], resid=g["resid"])
    assert _same_bits(y0, base), "B == 0 does not give the base projection's bits"
    # and the whole forward against fp64, y0 given (the base GEMM's own bf16 output)
    with torch.no_grad():
        _check_expand(base.cpu(), t.cpu(), c["b"], y1.detach(), f"lora_linear fwd {mode}")


def _grads_given64(c, t, dts, dx0):
    d = RL.d
    return {"dx": d(dx0) + d(dts) @ d(c["a"]), "dA": d(dts).t() @ d(c["x"]), "dB": d(c["dy"]).t() @ d(t)}


def _check_grads(c, g, scale, dx, dA, dB, calls, bf16_wgrad, tag):
    """dx / dA / dB (dA, dB accumulated over `calls` identical backward passes) against fp64."""
    with torch.no_grad():
        t = L.lora_shrink(g["x"], g["a"].detach(), scale).cpu()
        dts = L.lora_shrink(g["dy"], g["b"].detach(), scale, transposed=True).cpu()
        dx0 = input_grad(g["dy"], g["w"]).cpu()
    _check_shrink(c["dy"], c["b"].t(), scale, dts, f"{tag} dts")
    ref = _grads_given64(c, t, dts, dx0)
    M = c["x"].shape[0]
    e32 = R.e32_of(dx0.float() + dts.float() @ c["a"].float(), ref["dx"])
    extra = RL.dot_extra(dts.shape[1], RL.abs_dot_max(dts, c["a"].t()))
    R.check("lora_linear", f"{tag} dx", dx, ref["dx"], e32, extra, bf16=True)
    for name, got, p, q in (("dA", dA, dts, c["x"]), ("dB", dB, c["dy"], t)):
        r64 = calls * ref[name]
        e32 = R.e32_of(calls * (p.float().t() @ q.float()), r64)
        extra = calls * RL.dot_extra(M, RL.abs_dot_max(p.t(), q.t()))
        R.check("lora_linear", f"{tag} {name}", got, r64, e32, extra, bf16=bf16_wgrad)


@pytest.mark.parametrize("mode", ["plain", "bias", "resid"])
@pytest.mark.parametrize("mg_dtype", [None, torch.bfloat16, torch.float32])
def test_lora_linear_backward(mode, mg_dtype):
    scale = 2.0
    c = RL.full_case(250, 264, 136, 16, seed=4, with_bias=mode == "bias", with_resid=mode == "resid")
    g = _dev_case(c, mg_dtype)
    x = g["x"].clone().requires_grad_(True)
    resid = g["resid"].clone().requires_grad_(True) if g["resid"] is not None else None
    calls = 1 if mg_dtype is None else 2
    before = dict(L.CALLS)
    for _ in range(calls):
        x.grad = None
        y = L.lora_linear(x, g["w"], g["a"], g["b"], scale, bias=g["bias"], resid=resid)
        y.backward(g["dy"])
    # forward and backward each ran one shrink and one expand, all four on the HIP kernels
    for k, v in L.CALLS.items():
        assert v - before[k] == (2 * calls if k.endswith("_kernel") else 0), (k, v - before[k])
    dx = x.grad
    if mg_dtype is None:
        dA, dB = g["a"].grad, g["b"].grad
    else:
        assert g["a"].grad is None and g["b"].grad is None
        dA, dB = g["a"].main_grad, g["b"].main_grad
    assert g["w"].grad is None
    if resid is not None:
        assert _same_bits(resid.grad, (calls * g["dy"].float()).to(BF16))
    _check_grads(c, g, scale, dx, dA, dB, calls, mg_dtype != torch.float32, f"{mode} mg={mg_dtype}")
    # equal bits from a second, identical pass
    x2 = g["x"].clone().requires_grad_(True)
    h = _dev_case(c, mg_dtype)
    for _ in range(calls):
        x2.grad = None
        L.lora_linear(x2, h["w"], h["a"], h["b"], scale, bias=h["bias"],
                      resid=(h["resid"].clone().requires_grad_(True) if h["resid"] is not None else None)
                      ).backward(h["dy"])
    assert _same_bits(dx, x2.grad)
    dA2, dB2 = (h["a"].grad, h["b"].grad) if mg_dtype is None else (h["a"].main_grad, h["b"].main_grad)
    assert torch.equal(dA, dA2) and torch.equal(dB, dB2)


def test_lora_linear_frozen_input_skips_dx():
    c = RL.full_case(33, 64, 24, 8, seed=6)
    g = _dev_case(c)
    y = L.lora_linear(g["x"], g["w"], g["a"], g["b"], 2.0)  # x does not require grad
    y.backward(g["dy"])
    assert g["a"].grad is not None and g["b"].grad is not None and g["x"].grad is None


def test_lora_linear_under_checkpoint():
    from torch.utils.checkpoint import checkpoint

    scale = 2.0
    c = RL.full_case(64, 264, 136, 16, seed=7, with_resid=True)
    outs = []
    for use_ckpt in (False, True):
        g = _dev_case(c, torch.float32)
        x = g["x"].clone().requires_grad_(True)
        r = g["resid"].clone().requires_grad_(True)

        def f(x_, r_):
            return L.lora_linear(x_, g["w"], g["a"], g["b"], scale, resid=r_)

        y = checkpoint(f, x, r, use_reentrant=False) if use_ckpt else f(x, r)
        y.backward(g["dy"])
        assert g["a"].grad is None and g["b"].grad is None
        outs.append((x.grad.clone(), g["a"].main_grad.clone(), g["b"].main_grad.clone()))
    for p, q in zip(*outs):
        assert torch.equal(p, q), "activation recompute changes the gradient bits"
    assert outs[1][1].abs().sum() > 0 and outs[1][2].abs().sum() > 0


def test_lora_linear_graph_capture():
    scale = 2.0
    c0 = RL.full_case(250, 264, 136, 16, seed=8, with_resid=True)
    c1 = RL.full_case(250, 264, 136, 16, seed=9, with_resid=True)
    g = _dev_case(c0)
    xs, rs = g["x"].clone(), g["resid"].clone()
    with torch.no_grad():
        L.lora_linear(xs, g["w"], g["a"], g["b"], scale, resid=rs)  # warm: nothing lazy left for the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = L.lora_linear(xs, g["w"], g["a"], g["b"], scale, resid=rs)
        xs.copy_(c1["x"].to(DEV))
        rs.copy_(c1["resid"].to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = L.lora_linear(c1["x"].to(DEV), g["w"], g["a"], g["b"], scale, resid=c1["resid"].to(DEV))
    assert _same_bits(yg, want)


# ------------------------------------------------------------------------------ end to end
def _cpu_and_gpu_models(seed):
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.models import lora as ML

    cfg = get_config("tiny-llama")
    cpu = build_model(cfg, device="cpu", seed=seed)
    gpu = build_model(cfg, device=DEV, dtype=BF16, init=False)
    with torch.no_grad():
        for (n, p), (_, q) in zip(gpu.named_parameters(), cpu.named_parameters()):
            p.copy_(q.to(BF16))
    base = {n: p.detach().clone() for n, p in gpu.named_parameters()}
    for m in (cpu, gpu):
        ML.apply_lora(m, r=16, alpha=32, seed=seed)
        m.train()
    return cfg, cpu, gpu, base


@pytest.mark.parametrize("stage", ["sft", "dpo"])
def test_two_steps_on_tiny_llama(stage):
    """Two SFT steps / two shared-reference DPO steps in bf16 on the GPU next to the same steps in
    fp32 on the CPU, from the same weights and batches: the base stays bitwise, every target's
    adapter gets a gradient, and the losses agree within 0.02 (the bound test_trainers_gpu.py uses
    for its loss comparison)."""
    from distributed_llm_alignment_amd.data.synthetic import synthetic_lm_batch, synthetic_preference_batch
    from distributed_llm_alignment_amd.models import lora as ML
    from distributed_llm_alignment_amd.objectives import dpo_step_loss, sft_loss
    from distributed_llm_alignment_amd.parallel.data_parallel import DataParallelEngine

    _ext.require()
    cfg, cpu, gpu, base = _cpu_and_gpu_models(seed=3)
    for ad in ML.lora_adapters(gpu):
        assert L.lora_ok(torch.zeros(96, ad.A.shape[1], dtype=BF16, device=DEV), ad.A, ad.B), ad.qualified_name
    before = dict(L.CALLS)
    losses = {}
    for tag, m, dev in (("cpu", cpu, "cpu"), ("gpu", gpu, DEV)):
        eng = DataParallelEngine(m, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0)
        ref = ML.LoRAReference(m)
        g = torch.Generator().manual_seed(11)
        out = []
        for step in range(2):
            if stage == "sft":
                loss = sft_loss(m, synthetic_lm_batch(3, 40, cfg.vocab_size, device=dev, generator=g))
            else:
                batch = synthetic_preference_batch(2, 48, cfg.vocab_size, device=dev, generator=g, min_len=30)
                loss, metrics = dpo_step_loss(m, ref, batch, beta=0.1)
                assert torch.isfinite(metrics["rewards/accuracy"]).all()
            loss.backward()
            if step == 1:  # B left zero in step 0, so from here every A and B has a gradient
                for a in ML.lora_adapters(m):
                    assert a.A.main_grad.abs().sum() > 0 and a.B.main_grad.abs().sum() > 0, a.qualified_name
            eng.step()
            out.append(float(loss.detach()))
        losses[tag] = out
    print(f"FIG lora e2e {stage}: cpu {losses['cpu']} gpu {losses['gpu']}")
    ran = {k: v - before[k] for k, v in L.CALLS.items()}
    # r = 16, K <= 4096: every GPU adapter product ran a HIP kernel (the compositions are the CPU run's)
    assert ran["shrink_library"] == 0 and ran["expand_library"] == 0, ran
    assert ran["shrink_kernel"] > 0 and ran["shrink_kernel"] == ran["shrink_composition"], ran
    assert ran["expand_kernel"] > 0 and ran["expand_kernel"] == ran["expand_composition"], ran
    for n, p in gpu.named_parameters():
        if ".lora_" not in n:
            assert _same_bits(p, base[n]) and not p.requires_grad, f"base weight {n} changed"
        else:
            assert p.requires_grad
    for c, g_ in zip(losses["cpu"], losses["gpu"]):
        assert abs(c - g_) <= 0.02, losses
    if stage == "dpo":
        import math

        # B == 0: policy and reference log-probs are the same bits, the loss is -logsigmoid(0)
        assert abs(losses["gpu"][0] - math.log(2.0)) <= 1e-6, losses["gpu"]


@pytest.mark.parametrize("R_", [32, 64])
def test_library_path_outside_the_default_gates(R_):
    """Eligible calls outside the kernels' default gates (shrink: r > 32 or K > 4096; expand: r > 16) run the
    library GEMMs with the rounding of the formula of record: same bound as the kernels."""
    x, a = RL.shrink_case(33, 264, R_, seed=51)
    n0 = dict(L.CALLS)
    t = L.lora_shrink(x.to(DEV), a.to(DEV), 2.0)
    _check_shrink(x, a, 2.0, t, f"gated shrink R{R_}")
    y0, _, b = RL.expand_case(33, 136, R_, seed=52)
    y = y0.to(DEV)
    L.lora_expand_add_(y, t, b.to(DEV))
    _check_expand(y0, t.cpu(), b, y, f"library expand R{R_}")
    if L._MODE == "auto":  # the shrink kernel is the default up to r = 32 (K <= 4096), the expand up to r = 16
        assert L.CALLS["shrink_library"] - n0["shrink_library"] == (1 if R_ > 32 else 0)
        assert L.CALLS["shrink_kernel"] - n0["shrink_kernel"] == (0 if R_ > 32 else 1)
        assert L.CALLS["expand_library"] == n0["expand_library"] + 1
    zero = L.lora_expand_add_(y0.to(DEV), t, torch.zeros_like(b).to(DEV))
    assert _same_bits(zero, y0.to(DEV)), "B == 0 changes y on the library path"
    x, a = RL.shrink_case(16, 4104, 16, seed=53)  # r = 16 but K > 4096
    t = L.lora_shrink(x.to(DEV), a.to(DEV), 0.25)
    _check_shrink(x, a, 0.25, t, "library shrink K4104 R16")
