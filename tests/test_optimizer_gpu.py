"""GPU tier: csrc/adamw.hip (adamw_step, grad_sumsq, clip_coef) against fp64.

Sizes sit on the 8-element vectors and the grid cap: n = 8 (one vector), 2040 / 2048 / 2056
(255 / 256 / 257 vectors around one 256-thread block) and 2 097 160 (262 145 vectors, one past the
1024 x 256 grid, so the grid-stride loop runs a second time for exactly one lane). Weights,
both moments and, where present, the bf16 parameters are checked elementwise after every step.

Bound (see _refs64): 8 * E32 + 4 ulp32(max |ref|); E32 from the fp32 CPU branch run on a master
copy next to an independent fp64 chain. bf16 parameters without a master: one bf16 ulp of the
fp64 step taken from the parameters the kernel read, plus the fp32 bound.
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd.ops import _ext

import _branch32 as B32
import _refs64 as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16, F32 = torch.bfloat16, torch.float32
LAYOUTS = ["param+master", "param", "master"]


def _step_gpu(k, p, w, g, m, v, step, wd, clip, gs):
    hp = R.ADAMW_HP
    k.adamw_step(p, w, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, step, clip, gs)


def _chain(k, c, grads, n, layout, wd, clip, gs):
    """ADAMW_STEPS from zero moments in one layout; w, m, v (and the bf16 param) after every step."""
    clip_t = None if clip is None else torch.tensor(clip, dtype=F32, device=DEV)
    clip32 = None if clip is None else clip_t.item()  # the fp32 value the kernel reads
    p = c["w0"].to(DEV, BF16) if "param" in layout else None
    w = c["w0"].to(DEV) if "master" in layout else None
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    w64, m64, v64 = R.d(c["w0"]), torch.zeros(n, dtype=R.F64), torch.zeros(n, dtype=R.F64)
    w32, m32, v32 = c["w0"].clone(), torch.zeros(n), torch.zeros(n)
    for step, g_cpu, g in zip(R.ADAMW_STEPS, c["grads"], grads):
        if w is None:  # the bf16 parameters are the state: step from what the kernel reads
            w64 = R.d(p.cpu())
            w32 = p.cpu().float()
        _step_gpu(k, p, w, g, m, v, step, wd, clip_t, gs)
        w64, m64, v64 = R.adamw64(w64, g_cpu, m64, v64, step, wd, clip32, gs)
        w32, m32, v32 = B32.adamw(w32, g_cpu, m32, v32, step, wd, clip32, gs)
        tag = f"n={n} {layout} step={step} clip={clip} gs={gs}"
        R.check("adamw_step", f"m [{tag}]", m, m64, R.e32_of(m32, m64))
        R.check("adamw_step", f"v [{tag}]", v, v64, R.e32_of(v32, v64))
        if w is not None:
            R.check("adamw_step", f"w [{tag}]", w, w64, R.e32_of(w32, w64))
            if p is not None:
                assert torch.equal(p, w.to(BF16)), "bf16 param != master.to(bf16)"
        else:
            R.check("adamw_step_bf16", f"p [{tag}]", p, w64, R.e32_of(w32, w64), bf16=True)
    assert (w64 - R.d(c["w0"])).abs().max() > 1e-3  # the steps moved the weights


@pytest.mark.parametrize("wd", R.ADAMW_WD)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("gdt", [BF16, F32], ids=["gbf16", "gfp32"])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_step(n, gdt, layout, wd):
    k = _ext.require()
    c = R.adamw_case(n, gdt)
    grads = [g.to(DEV) for g in c["grads"]]
    # every (clip, grad_scale) pair; at the 2 M size the two pairs that hold every value (run time)
    pairs = [(cl, gs) for cl in R.ADAMW_CLIP for gs in R.ADAMW_GS]
    for clip, gs in (pairs if n < 1_000_000 else [pairs[0], pairs[3]]):
        _chain(k, c, grads, n, layout, wd, clip, gs)


@pytest.mark.parametrize("gdt", [BF16, F32], ids=["gbf16", "gfp32"])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_grad_sumsq(n, gdt):
    k = _ext.require()
    g_cpu = R.sumsq_case(n, gdt)
    g = g_cpu.to(DEV)
    ref = R.d(g_cpu).pow(2).sum().reshape(1)
    cpu = torch.zeros(1)
    out = torch.full((1,), 7.0, device=DEV)  # accumulate=False overwrites
    k.grad_sumsq(g, out, False)
    B32.grad_sumsq(g_cpu, cpu, False)
    R.check("grad_sumsq", f"n={n}", out, ref, R.e32_of(cpu, ref))
    again = torch.zeros(1, device=DEV)
    k.grad_sumsq(g, again, False)
    assert torch.equal(out, again)  # fixed grid, fixed order
    for i in (2, 3):  # accumulate twice into the same out
        k.grad_sumsq(g, out, True)
        B32.grad_sumsq(g_cpu, cpu, True)
        R.check("grad_sumsq", f"n={n} accumulate x{i}", out, i * ref, R.e32_of(cpu, i * ref))


@pytest.mark.parametrize("gdt", [BF16, F32], ids=["gbf16", "gfp32"])
@pytest.mark.parametrize("n,o", [(2056, 8), (2040, 4104), (2_097_160, 64)])
def test_grad_sumsq_slice(n, o, gdt):
    """A slice g[o:o+n] of a larger shard, o a multiple of 8 elements (the expert-norm path of
    parallel/data_parallel.py), accumulated onto a previous value."""
    k = _ext.require()
    big_cpu = R.sumsq_case(n, gdt, seed=3, total=n + o + 24)
    big = big_cpu.to(DEV)
    ref = R.d(big_cpu[o:o + n]).pow(2).sum().reshape(1) + 2.5
    out = torch.full((1,), 2.5, device=DEV)
    cpu = torch.full((1,), 2.5)
    k.grad_sumsq(big[o:o + n], out, True)
    B32.grad_sumsq(big_cpu[o:o + n], cpu, True)
    R.check("grad_sumsq", f"slice n={n} o={o}", out, ref, R.e32_of(cpu, ref))


@pytest.mark.parametrize("sumsq,max_norm,exact", [(9.0, 1.0, None), (9.0, 4.0, 1.0), (9.0, 0.0, 1.0),
                                                  (9.0, -1.0, 1.0), (0.0, 1.0, 1.0), (0.0, 0.0, 1.0),
                                                  (1234.5, 0.37, None)])
def test_clip_coef(sumsq, max_norm, exact):
    k = _ext.require()
    s_cpu = torch.tensor([sumsq], dtype=F32)
    norm, coef = k.clip_coef(s_cpu.to(DEV), max_norm)
    n64, c64 = R.clip_coef64(s_cpu.item(), max_norm)
    ncpu, ccpu = B32.clip_coef(s_cpu, max_norm)
    R.check("clip_coef", "norm", norm, torch.tensor(n64, dtype=R.F64), R.e32_of(ncpu, torch.tensor(n64, dtype=R.F64)))
    R.check("clip_coef", "coef", coef, torch.tensor(c64, dtype=R.F64), R.e32_of(ccpu, torch.tensor(c64, dtype=R.F64)))
    if exact is not None:  # a norm below max_norm, max_norm <= 0: exactly 1 (sumsq = 0 included)
        assert coef.item() == exact
    assert torch.isfinite(norm).all() and torch.isfinite(coef).all()
