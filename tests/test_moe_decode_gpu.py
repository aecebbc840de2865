"""MI355X: the decode-shaped MoE expert kernels (csrc/moe_decode.hip) against an fp64 reference of
the formula of record, their refusals, and the path through MoE.forward / generate.

Bound per output element, S = sum_j |topv_j| sum_f |a_f| |W_d[n, f]| in fp64:
    |out - ref64| <= 2^-8 S + half a bf16 ulp of ref64
(2^-9 S is the single bf16 rounding of `a`; the factor 2 covers fp32 accumulation, depth * 2^-24 of
the same sums at K <= 1024, and __expf). Each case prints its worst err / bound."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E = 8


def _C():
    from distributed_llm_alignment_amd.ops import _ext

    return _ext.require()


def _rand(*shape, g, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(torch.bfloat16)


def _ref64(h2, topv, topi, w_up, w_down):
    """(ref, S) in fp64 on the same bf16 tensors, `a` rounded to bf16 once; only routed experts are read."""
    Fd = w_down.shape[2]
    ref = torch.zeros(h2.shape, dtype=torch.float64, device=DEV)
    S = torch.zeros_like(ref)
    for e in topi.unique().tolist():
        hit = topi == e
        rows = hit.any(1)
        w = (topv.double() * hit).sum(1)[rows].unsqueeze(1)
        gu = h2[rows].double() @ w_up[e].double().t()
        a = (F.silu(gu[:, :Fd]) * gu[:, Fd:]).to(torch.bfloat16).double()
        ref[rows] += w * (a @ w_down[e].double().t())
        S[rows] += w.abs() * (a.abs() @ w_down[e].double().abs().t())
    return ref, S


def _case(H, Fd, M, k, planted=False):
    g = torch.Generator(device=DEV).manual_seed(1000 * M + 10 * k + H)
    h2 = _rand(M, H, g=g)
    w_up = _rand(E, 2 * Fd, H, g=g, scale=H ** -0.5)
    w_down = _rand(E, H, Fd, g=g, scale=Fd ** -0.5)
    topv = torch.softmax(torch.randn(M, k, device=DEV, generator=g), -1)
    if planted:  # every token on experts {0, 3}; the idle experts' weights must never be read
        topi = torch.tensor([0, 3], dtype=torch.int32, device=DEV).repeat(M, 1)
        idle = [e for e in range(E) if e not in (0, 3)]
        w_up[idle] = float("nan")
        w_down[idle] = float("nan")
    else:
        topi = torch.rand(M, E, device=DEV, generator=g).argsort(1)[:, :k].to(torch.int32).contiguous()
    return h2, topv, topi, w_up, w_down


def _check(H, Fd, M, k, planted=False):
    h2, topv, topi, w_up, w_down = _case(H, Fd, M, k, planted)
    C = _C()
    out = C.moe_decode_down(C.moe_decode_glu(h2, topi, w_up), topv, topi, w_down)
    again = C.moe_decode_down(C.moe_decode_glu(h2, topi, w_up), topv, topi, w_down)
    assert out.shape == (M, H) and out.dtype == torch.bfloat16
    assert torch.equal(out, again), "two runs must give equal bits"
    assert torch.isfinite(out).all()
    ref, S = _ref64(h2, topv, topi, w_up, w_down)
    half_ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref).exponent - 1 - 8)
    bound = 2.0 ** -8 * S + half_ulp
    ratio = ((out.double() - ref).abs() / bound).max().item()
    print(f"moe_decode H={H} F={Fd} M={M} k={k} planted={planted}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("H,Fd", [(256, 512), (1024, 256)])
def test_ops_match_fp64_reference(H, Fd, M, k):
    _check(H, Fd, M, k)


@pytest.mark.parametrize("M", [64, 17])
@pytest.mark.parametrize("H,Fd", [(256, 512), (1024, 256)])
def test_planted_routing_never_reads_idle_experts(H, Fd, M):
    """One expert with four full row tiles (M = 64) or a tile boundary (17 rows); the six idle
    experts hold NaN in both weight tensors."""
    _check(H, Fd, M, 2, planted=True)


@pytest.mark.parametrize("what", ["M=65", "k=9", "H=40", "fp16 weights", "int64 topi", "w_down mismatch",
                                  "unaligned view"])
def test_refusals(what):
    H, Fd, M, k = 256, 512, 4, 2
    if what == "M=65":
        M = 65
    elif what == "k=9":
        k = 9
    elif what == "H=40":
        H = 40
    g = torch.Generator(device=DEV).manual_seed(0)
    Ex = 16 if what == "k=9" else E
    h2 = _rand(M, H, g=g)
    w_up = _rand(Ex, 2 * Fd, H, g=g, scale=0.05)
    w_down = _rand(Ex, H, Fd, g=g, scale=0.05)
    topi = torch.arange(k, dtype=torch.int32, device=DEV).repeat(M, 1)
    topv = torch.full((M, k), 1.0 / k, device=DEV)
    a = _rand(M * k, Fd, g=g)
    C = _C()
    if what == "fp16 weights":
        w_up, w_down = w_up.half(), w_down.half()
    elif what == "int64 topi":
        topi = topi.long()
    elif what == "unaligned view":
        h2 = _rand(M * H + 8, g=g)[1:1 + M * H].view(M, H)
        a = _rand(M * k * Fd + 8, g=g)[1:1 + M * k * Fd].view(M * k, Fd)
    elif what == "w_down mismatch":
        w_down = _rand(Ex, H, Fd + 32, g=g)
    if what != "w_down mismatch":
        with pytest.raises(RuntimeError):
            C.moe_decode_glu(h2, topi, w_up)
    with pytest.raises(RuntimeError):
        C.moe_decode_down(a, topv, topi, w_down)
    torch.cuda.synchronize()


def _tiny_mixtral(seed):
    from distributed_llm_alignment_amd.models import build_model, get_config

    cfg = get_config("tiny-mixtral", hidden_size=256, head_dim=64, intermediate_size=512, num_experts=8)
    return cfg, build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=seed)


def test_generate_moe_decode_graph_matches_eager_and_arms_keep_their_graphs():
    from distributed_llm_alignment_amd.models import generate
    from distributed_llm_alignment_amd.models import generation as gen

    gen.clear_graph_cache()
    cfg, m = _tiny_mixtral(3)
    g = torch.Generator(device=DEV).manual_seed(6)
    ids = torch.randint(3, cfg.vocab_size, (3, 17), device=DEV, generator=g)
    am = torch.ones_like(ids)
    am[2, :4] = 0
    ids[2, :4] = 0
    kw = dict(max_new_tokens=16, do_sample=False, eos_token_id=-1)
    eager = generate(m, ids, am, use_graph=False, moe_decode=True, **kw)
    graphs, toks = [], []
    for arm in (False, True, False):
        toks.append(generate(m, ids, am, use_graph=True, moe_decode=arm, **kw))
        slot = gen._GRAPH_SLOT[id(m)]
        assert slot[3].graph is not None
        assert slot[1][-1] == arm  # the arm is part of the reuse key
        graphs.append(slot[3])
    assert torch.equal(toks[1], eager)
    assert torch.equal(toks[0], toks[2])
    assert graphs[0] is not graphs[1] and graphs[1] is not graphs[2]  # never the other arm's graph
    gen.clear_graph_cache()


def test_moe_layer_on_decode_kernels_matches_reference():
    from distributed_llm_alignment_amd import ops

    cfg, m = _tiny_mixtral(2)
    moe = m.layers[0].mlp
    h = _rand(1, 24, cfg.hidden_size, g=torch.Generator(device=DEV).manual_seed(5))
    with torch.no_grad(), ops.moe.skinny_decode():
        out = moe(h)
    with torch.no_grad():
        grouped = moe(h)
    ref = ops.moe.ref_moe(h.reshape(-1, cfg.hidden_size), moe.router, moe.expert_up, moe.expert_down,
                          cfg.num_experts_per_tok).view_as(h)
    rel = ((out.float() - ref).norm() / ref.norm()).item()
    assert rel < 2e-2, rel
    assert not torch.equal(out, grouped)  # the switch did change the path (y is not rounded per expert)
