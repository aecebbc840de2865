"""GPU tier: `grpo_loss_seq` (csrc/losses.hip, the GRPO loss with the sequence-level ratio, GSPO)
against the fp64 reference of tests/_refs64_gspo.py, elementwise on loss, gradient and metrics;
every call is launched twice and the two results must be bitwise equal. Shapes sit around the
256-thread row stride of the row reduction and include S > 256 for the finalising loops.

Bound (see _refs64): 8 * E32 + 4 ulp32(max |ref|), E32 being the error of the package's fp32 CPU
branch on the same inputs. No extra term: the kernel's row sum (256 strided partial sums, a wave
shuffle tree, four wave totals) is another summation order than the CPU branch's, and stays inside
the plain bound (worst err / bound measured 0.54, on a loss; the FIG lines are in profiles/gspo.md).
"""
import pytest
import torch

import distributed_llm_alignment_amd as dla  # noqa: F401
from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.ops import _ext
from distributed_llm_alignment_amd.ops.losses import _ref_grpo_loss

import _branch32_gspo as BG
import _refs64 as R
import _refs64_gspo as RG
import _refs64_is as RI

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("loss", "dlp", "metrics")


def dev(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def twice(fn):
    """Launch twice; the outputs must be bitwise equal. Returns the first result."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two launches differ bitwise"
    return a


def compare(kernel, got, ref, cpu):
    assert set(got) == set(ref)
    for k in ref:
        R.check(kernel, k, got[k], ref[k], R.e32_of(cpu[k], ref[k]))


def _seq_gpu(c, beta, mode, max_len, denom=None, w=None, alias_old=False):
    k = _ext.require()
    g = dev(c)
    dn = None if denom is None else torch.tensor([denom], dtype=torch.float32, device=DEV)
    wd = None if w is None else w.to(DEV)
    old = g["lp"] if alias_old else g["old"]
    out = twice(lambda: k.grpo_loss_seq(g["lp"], old, g["ref"], g["adv"], g["m"], wd, dn, R.GRPO_CLIP[0],
                                        R.GRPO_CLIP[1], beta, R.GRPO_MODES.index(mode), float(max_len)))
    return dict(zip(KEYS, out))


def _check_case(c, kw, w=None):
    S, T = c["m"].shape
    got = _seq_gpu(c, **kw, w=w)
    ref = RG.gspo64(**c, **kw, w=w)
    compare("grpo_loss_seq_w" if w is not None else "grpo_loss_seq", got, ref, BG.gspo(**c, **kw, w=w))
    n = c["m"].sum().item()
    assert got["metrics"][3].item() == n  # the count is exact
    # every row is at least SEP from the clip range: the decisions, so the clipped-token count, are the reference's
    assert round(got["metrics"][0].item() * n) == RG.clipped_tokens64(c["lp"], c["old"], c["m"])
    assert (got["dlp"].cpu()[c["m"] == 0] == 0).all()  # fully masked rows included
    return got


@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
@pytest.mark.parametrize("S,T", RG.GSPO_SHAPES)
def test_grpo_loss_seq(S, T, mode, beta):
    c = RG.gspo_case(S, T)
    kw = dict(beta=beta, mode=mode, max_len=T)
    plain = _check_case(c, kw)
    _check_case(c, kw, w=RI.weight_case((S, T)))
    # w = 1 is the unweighted instantiation, bit for bit (1.0f * x and c_s / c_s are exact)
    ones = _seq_gpu(c, **kw, w=torch.ones(S, T))
    for key in KEYS:
        assert torch.equal(ones[key], plain[key]), key


def test_grpo_loss_seq_denom():
    c = RG.gspo_case(257, 5)
    kw = dict(beta=0.04, mode="token", max_len=5, denom=R.GRPO_DENOM)
    plain = _check_case(c, kw)
    _check_case(c, kw, w=RI.weight_case((257, 5)))
    ones = _seq_gpu(c, **kw, w=torch.ones(257, 5))
    for key in KEYS:
        assert torch.equal(ones[key], plain[key]), key


@pytest.mark.parametrize("mode", R.GRPO_MODES)
def test_on_policy_is_the_token_op_within_the_bound(mode):
    """`old` aliasing `lp`: l_s = 0 and sr_s = 1 exactly, nothing is clipped, and loss / gradient are
    the token op's up to the rounding of either (checked against fp64 with the token op's E32)."""
    k = _ext.require()
    c = RG.gspo_case(300, 257)
    kw = dict(beta=0.04, mode=mode, max_len=257)
    got = _seq_gpu(c, **kw, alias_old=True)
    assert got["metrics"][0].item() == 0 and got["metrics"][1].item() == 0
    g = dev(c)
    tok = dict(zip(KEYS, k.grpo_loss(g["lp"], g["lp"], g["ref"], g["adv"], g["m"], None, R.GRPO_CLIP[0],
                                     R.GRPO_CLIP[1], 0.04, R.GRPO_MODES.index(mode), 257.0)))
    same = {**c, "old": c["lp"]}
    ref = RG.gspo64(**same, **kw)
    cpu = BG.gspo(**same, **kw, level="token")
    for key in ("loss", "dlp"):
        e32 = R.e32_of(cpu[key], ref[key])
        R.check("grpo_loss_seq_on_policy", key, got[key], ref[key], e32)
        R.check("grpo_loss_on_policy", key, tok[key], ref[key], e32)
    assert torch.equal(tok["metrics"][3], got["metrics"][3])


@pytest.mark.parametrize("weighted", [False, True])
def test_junk_outside_the_mask_is_never_read(weighted):
    c = RG.gspo_case(300, 257)
    w = RI.weight_case((300, 257)) if weighted else None
    kw = dict(beta=0.04, mode="sequence", max_len=257)
    got = _seq_gpu(c, **kw, w=w)
    off = c["m"] == 0
    assert (c["lp"][off] == RG.JUNK).all() and (c["old"][off] == -RG.JUNK).all() and (c["m"].sum(1) == 0).sum() >= 2
    assert (got["dlp"].cpu()[off] == 0).all()
    for junk in (0.0, float("nan")):
        z = {k: (torch.where(off, torch.full_like(v, junk), v) if v.dim() == 2 and k != "m" else v) for k, v in c.items()}
        zw = None if w is None else torch.where(off, torch.full_like(w, junk), w)
        zero = _seq_gpu(z, **kw, w=zw)
        for key in KEYS:
            assert torch.equal(zero[key], got[key]), (junk, key)


def test_wrapper_runs_the_op_and_token_is_the_old_path():
    k = _ext.require()
    c = RG.gspo_case(257, 5)
    w = RI.weight_case((257, 5))
    g = dev(c)
    for iw in (None, w):
        x = g["lp"].clone().requires_grad_(True)
        loss, met = ops.grpo_loss(x, g["old"], g["ref"], g["adv"], g["m"], 0.2, 0.28, 0.04, "token", is_weight=
                                  None if iw is None else iw.to(DEV), importance_level="sequence")
        loss.backward()
        raw = _seq_gpu(c, beta=0.04, mode="token", max_len=0, w=iw)
        assert torch.equal(loss.detach(), raw["loss"]) and torch.equal(x.grad, raw["dlp"] * 1)
        assert torch.equal(torch.stack([met[n] for n in ("clipfrac", "approx_kl", "kl_ref", "tokens")]), raw["metrics"])
    g = dev(R.grpo_case(257, 5))  # (the token kernel reads outside the mask: no junk there)
    x = g["lp"].clone().requires_grad_(True)
    loss, _ = ops.grpo_loss(x, g["old"], g["ref"], g["adv"], g["m"], 0.2, 0.28, 0.04, "token", importance_level="token")
    loss.backward()
    raw = k.grpo_loss(g["lp"], g["old"], g["ref"], g["adv"], g["m"], None, 0.2, 0.28, 0.04, 1, 0.0)
    assert torch.equal(loss.detach(), raw[0]) and torch.equal(x.grad, raw[1])


def test_argument_checks():
    k = _ext.require()
    g = dev(RG.gspo_case(3, 255))
    lp, old, ref, adv, m = (g[n] for n in ("lp", "old", "ref", "adv", "m"))
    tail = (None, 0.2, 0.28, 0.04, 0, 255.0)
    k.grpo_loss_seq(lp, old, ref, adv, m, None, *tail)
    for bad in ((lp, old[:, :-1].contiguous(), ref, adv, m), (lp, old, ref, adv[:-1], m), (lp, old, ref, adv, m[:-1]),
                (lp.double(), old, ref, adv, m), (lp, old, ref, adv.double(), m), (lp, old.cpu(), ref, adv, m),
                (lp.cpu(), old.cpu(), ref.cpu(), adv.cpu(), m.cpu()), (lp[0], old[0], ref[0], adv, m[0])):
        with pytest.raises(RuntimeError):
            k.grpo_loss_seq(*bad, None, *tail)
    for mode in (3, -1):
        with pytest.raises(RuntimeError):
            k.grpo_loss_seq(lp, old, ref, adv, m, None, None, 0.2, 0.28, 0.04, mode, 255.0)
    with pytest.raises(RuntimeError):  # constant mode without max_len or denom
        k.grpo_loss_seq(lp, old, ref, adv, m, None, None, 0.2, 0.28, 0.04, 2, 0.0)
    for w in (m[:, :-1].contiguous(), m[:-1], m.double(), m.cpu()):
        with pytest.raises(RuntimeError):
            k.grpo_loss_seq(lp, old, ref, adv, m, w, *tail)


def test_graph_capture():
    """The raw op (two launches on one stream: a linear graph), weighted, captured in a hipGraph and
    replayed on inputs overwritten in place equals an eager call on the new inputs bitwise: no host
    read of a device value anywhere."""
    k = _ext.require()

    def inputs(seed):
        c = RG.gspo_case(6, 37, seed=seed)
        return [t.to(DEV).contiguous() for t in (c["lp"], c["old"], c["ref"], c["adv"], c["m"],
                                                 RI.weight_case((6, 37), seed=seed))]

    args = (0.2, 0.28, 0.04, 1, 37.0)
    first, new = inputs(2), inputs(3)
    denom = torch.full((1,), 5.0, device=DEV)
    k.grpo_loss_seq(*first, denom, *args)  # warm: nothing lazy left for the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = k.grpo_loss_seq(*first, denom, *args)
    for dst, src in zip(first, new):
        dst.copy_(src)
    denom.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    want = k.grpo_loss_seq(*new, torch.full((1,), 7.0, device=DEV), *args)
    for got, w in zip(out, want):
        assert torch.equal(got, w)


def test_gspo_step_two_layer_model():
    """One end-to-end step on the tiny model of test_grpo_gpu.py: `objectives.grpo_loss` at the
    sequence level. The [S, T] gradient the op hands to the model equals the CPU formula's at the
    same log-probs within R.check's bound, the loss is finite and the policy gradient non-zero."""
    from distributed_llm_alignment_amd.models import build_model, get_config
    from distributed_llm_alignment_amd.objectives import grpo_loss, grpo_rollout_stats
    from distributed_llm_alignment_amd.parallel.data_parallel import DataParallelEngine

    _ext.require()
    cfg = get_config("tiny-llama-d128", num_layers=2)
    pol = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    ref = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=0).requires_grad_(False).eval()
    eng = DataParallelEngine(pol, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(0)
    Tp, n, G, P = 16, 16, 4, 2
    seqs = torch.randint(3, cfg.vocab_size, (P * G, Tp + n), generator=g).to(DEV)
    mask = torch.ones_like(seqs)
    mask[1, Tp + 10:] = 0  # one rollout ended early
    scores = torch.randn(P * G, generator=g).to(DEV)
    stats = grpo_rollout_stats(pol, ref, seqs, mask, Tp, scores, G, beta=0.04, need_old=True)
    # an old policy whose rows sit on both sides of the clip range (row means of d = +-0.3, +-0.1 ...)
    shift = torch.tensor([0.3, -0.3, 0.1, -0.1, 0.35, -0.4, 0.05, 0.0])[:, None].to(DEV)
    noise = 0.05 * torch.randn(P * G, Tp + n, generator=g).to(DEV)
    stats["old_logp"] = (stats["old_logp"] - shift + noise) * stats["act"]
    loss, m = grpo_loss(pol, seqs, mask, stats, 0.2, 0.28, 0.04, "sequence", n, importance_level="sequence")
    loss.backward()
    assert torch.isfinite(loss).item() and 0 < m["clipfrac"].item() < 1 and m["approx_kl"].item() > 0
    assert eng.grad_buf.float().abs().sum().item() > 0
    # the op once more on the same log-probs, for its [S, T] gradient
    with torch.no_grad():
        lp_dev = pol.token_logprobs(seqs, mask)
    x = lp_dev.clone().requires_grad_(True)
    again, _ = ops.grpo_loss(x, stats["old_logp"], stats["ref_logp"], stats["advantages"], stats["act"], 0.2, 0.28,
                             0.04, "sequence", n, importance_level="sequence")
    again.backward()
    assert abs(again.item() - loss.item()) < 1e-6
    lp = lp_dev.float().cpu()
    c = {"lp": lp, "old": stats["old_logp"].float().cpu(), "ref": stats["ref_logp"].float().cpu(),
         "adv": stats["advantages"].float().cpu(), "m": stats["act"].float().cpu()}
    kw = dict(beta=0.04, mode="sequence", max_len=n)
    sr = RG._rows(c["lp"], c["old"], c["m"])[1]
    lo, hi = 1 - R.GRPO_CLIP[0], 1 + R.GRPO_CLIP[1]
    assert ((sr - lo).abs() >= R.SEP).all() and ((sr - hi).abs() >= R.SEP).all()  # same decisions in fp32 and fp64
    ref64, cpu = RG.gspo64(**c, **kw), BG.gspo(**c, **kw)
    R.check("gspo_step", "dlp", x.grad, ref64["dlp"], R.e32_of(cpu["dlp"], ref64["dlp"]))
    R.check("gspo_step", "loss", again.detach(), ref64["loss"], R.e32_of(cpu["loss"], ref64["loss"]))
    want, _ = _ref_grpo_loss(lp, c["old"], c["ref"], c["adv"], c["m"], 0.2, 0.28, 0.04, "sequence", n,
                             importance_level="sequence")
    assert abs(loss.item() - want.item()) < 1e-4
    p0 = eng.param_buf.detach().float().clone()
    norm = float(eng.step())
    assert 0 < norm < float("inf") and ((eng.param_buf.detach().float() - p0).abs() > 0).any()
