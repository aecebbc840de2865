"""CPU tier: the package's fp32 CPU branch agrees with the fp64 references of tests/_refs64.py on
every builder and shape that the GPU modules use, and the builders' own boundary assertions hold
(they run inside each builder). This ties the references to the formulas of record without a GPU
and prints E32, the fp32 branch's max abs error against fp64, per output.

Bound: an fp32 formula of <= ~20 operations on well-scaled inputs is good to ~1e-6 relative; the
branch must agree to 1e-4 of the output's largest magnitude, plus, for reductions (which may
cancel to near 0), 1e-6 of the inputs' magnitude. A wrong formula is off by percents."""
import pytest
import torch

import _branch32 as B32
import _refs64 as R


def agree(name, cpu, ref, inscale=8.0):
    assert set(cpu) == set(ref), name
    for k in ref:
        a, b = R.d(cpu[k]).reshape(-1), R.d(ref[k]).reshape(-1)
        assert a.shape == b.shape, f"{name}/{k}"
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin], b[~fin]), f"{name}/{k}: non-finite entries"
        e32 = R.e32_of(cpu[k], ref[k])
        scale = b[fin].abs().max().item() if fin.any() else 0.0
        bound = 1e-4 * scale + (1e-6 * inscale if b.numel() <= 8 else 0.0)
        print(f"E32 {name} {k}: {e32:.3e} (bound {bound:.3e})")
        assert e32 <= bound, f"{name}/{k}: {e32:.3e} > {bound:.3e}"


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("S,T", R.SEQ_SHAPES + [R.SEQ_BIG])
def test_seq_reduce(S, T, mean):
    c = R.seq_case(S, T)
    agree("seq_reduce", B32.seq_reduce(**c, mean=mean), R.seq_reduce64(**c, mean=mean))


@pytest.mark.parametrize("ls", R.DPO_LS)
@pytest.mark.parametrize("beta", R.DPO_BETAS)
@pytest.mark.parametrize("B", R.PAIR_B)
def test_dpo(B, beta, ls):
    c = R.dpo_case(B)
    agree("dpo_loss", B32.dpo(**c, beta=beta, ls=ls), R.dpo64(**c, beta=beta, ls=ls))


@pytest.mark.parametrize("ls", R.DPO_LS)
@pytest.mark.parametrize("beta", R.DPO_BETAS)
def test_dpo_saturated(beta, ls):
    c = R.dpo_sat_case(beta)
    agree("dpo_loss_sat", B32.dpo(**c, beta=beta, ls=ls), R.dpo64(**c, beta=beta, ls=ls), inscale=1e4)


@pytest.mark.parametrize("B", R.PAIR_B)
def test_pairwise(B):
    c = R.pairwise_case(B)
    agree("pairwise_loss", B32.pairwise(**c), R.pairwise64(**c))


def test_pairwise_saturated():
    c = R.pairwise_sat_case()
    agree("pairwise_loss_sat", B32.pairwise(**c), R.pairwise64(**c), inscale=1e4)


@pytest.mark.parametrize("n", R.KLPG_N)
def test_klpg(n):
    c = R.klpg_case(n)
    agree("kl_penalty_pg", B32.klpg(**c), R.klpg64(**c))


@pytest.mark.parametrize("T,mask,gl", R.GAE_CASES)
def test_gae(T, mask, gl):
    c = R.gae_case(T, mask)
    agree("gae", B32.gae(**c, gamma=gl[0], lam=gl[1]), R.gae64(**c, gamma=gl[0], lam=gl[1]))


@pytest.mark.parametrize("n,masked", [(n, False) for n in R.PPO_N] + [(1025, True)])
def test_ppo(n, masked):
    c = R.ppo_policy_case(n, masked)
    agree("ppo_policy_loss", B32.ppo_policy(**c), R.ppo_policy64(**c))
    c = R.ppo_value_case(n, masked)
    agree("ppo_value_loss", B32.ppo_value(**c), R.ppo_value64(**c))


@pytest.mark.parametrize("scale_std", [True, False])
@pytest.mark.parametrize("G", R.GROUP_G)
def test_group_advantages(G, scale_std):
    c = R.group_case(G)
    ref = R.group_advantages64(**c, scale_std=scale_std)
    agree("group_advantages", B32.group_advantages(**c, scale_std=scale_std), ref)
    if G == 1:
        assert (ref["adv"] == 0).all() and (ref["sd"] == 0).all()


@pytest.mark.parametrize("beta", R.GRPO_BETAS)
@pytest.mark.parametrize("mode", R.GRPO_MODES)
@pytest.mark.parametrize("S,T", R.GRPO_SHAPES)
def test_grpo(S, T, mode, beta):
    c = R.grpo_case(S, T)
    kw = dict(beta=beta, mode=mode, max_len=T)
    agree("grpo_loss", B32.grpo(**c, **kw), R.grpo64(**c, **kw))


def test_grpo_denom():
    c = R.grpo_case(257, 5)
    kw = dict(beta=0.04, mode="token", max_len=5, denom=R.GRPO_DENOM)
    agree("grpo_loss_denom", B32.grpo(**c, **kw), R.grpo64(**c, **kw))


@pytest.mark.parametrize("gdt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw(n, gdt):
    c = R.adamw_case(n, gdt)
    for wd, clip, gs in [(0.0, None, 1.0), (0.1, 0.37, 0.5)]:
        w32, m32, v32 = c["w0"].clone(), torch.zeros(n), torch.zeros(n)
        w64, m64, v64 = R.d(c["w0"]), torch.zeros(n, dtype=R.F64), torch.zeros(n, dtype=R.F64)
        clip32 = None if clip is None else torch.tensor(clip, dtype=torch.float32).item()
        for step, g in zip(R.ADAMW_STEPS, c["grads"]):
            w32, m32, v32 = B32.adamw(w32, g, m32, v32, step, wd, clip, gs)
            w64, m64, v64 = R.adamw64(w64, g, m64, v64, step, wd, clip32, gs)
            agree(f"adamw step {step}", {"w": w32, "m": m32, "v": v32}, {"w": w64, "m": m64, "v": v64})
    for k, x in R.ADAMW_HP.items():  # the stated hyper-parameters are fp32 values
        assert float(torch.tensor(x, dtype=torch.float32)) == x, k


@pytest.mark.parametrize("gdt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_grad_sumsq_and_clip(n, gdt):
    g = R.sumsq_case(n, gdt)
    ref = R.d(g).pow(2).sum()
    out = torch.zeros(1)
    B32.grad_sumsq(g, out, False)
    agree("grad_sumsq", {"s": out}, {"s": ref.reshape(1)}, inscale=0.0)
    B32.grad_sumsq(g, out, True)
    B32.grad_sumsq(g, out, True)
    agree("grad_sumsq_acc", {"s": out}, {"s": 3 * ref.reshape(1)}, inscale=0.0)
    for sumsq, max_norm in [(out, 1.0), (out, 1e6), (out, 0.0), (torch.zeros(1), 1.0)]:
        norm, coef = B32.clip_coef(sumsq, max_norm)
        n64, c64 = R.clip_coef64(sumsq.item(), max_norm)
        agree("clip_coef", {"norm": norm, "coef": coef},
              {"norm": torch.tensor(n64, dtype=R.F64), "coef": torch.tensor(c64, dtype=R.F64)}, inscale=0.0)


@pytest.mark.parametrize("pattern", [None] + R.DEAD_PATTERNS)
@pytest.mark.parametrize("kind", R.ROW_V + ["sliced"])
def test_logprob_rows(kind, pattern):
    x = R.rows_case(kind).clone()
    N, V = x.shape
    tgt = R.rows_targets(N, V)
    if pattern is not None:
        dead = R.dead_mask(V, pattern)
        x[R.DEAD_ROW, dead] = R.NINF
        tgt[R.DEAD_ROW] = int(dead.nonzero()[0])  # this row's target sits on a -inf logit
    ref = R.logprob64(x, tgt)
    assert torch.isfinite(ref["lse"]).all()
    if pattern is not None:
        assert ref["logp"][R.DEAD_ROW] == R.NINF
    agree("logprob_fwd", B32.logprob(x, tgt), ref, inscale=16.0)
    g = torch.randn(N, generator=R.gen(5))
    agree("logprob_bwd", {"d": B32.logprob_bwd(x, tgt, g)}, {"d": R.logprob_bwd64(x, tgt, g)})


@pytest.mark.parametrize("K", R.ENS_K)
@pytest.mark.parametrize("N,V", R.ENS_SHAPES)
def test_ensemble_kl(N, V, K):
    c = R.ensemble_case(N, V, K)
    ref = R.ensemble_kl64(**c)
    assert torch.isfinite(ref["kl"]).all()
    agree("ensemble_kl", B32.ensemble_kl(**c), ref)
