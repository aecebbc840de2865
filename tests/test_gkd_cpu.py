"""CPU tier of on-policy distillation (GKD): the CPU `ops.generalized_jsd` against the fp64 reference,
its autograd against the closed-form gradient, the chunked objective, the position mask, the dataset's
prompt fields, the trainer's start-up errors and short trainer runs at lmbda 0 and 1.

Tolerance of the fp32 CPU formula against fp64: every log-probability is a difference of numbers as
large as the scaled logit range, each carrying a few fp32 ulps, and L sums probability-weighted
differences of them, so |L32 - L64| <= TOL_ULPS * eps32 * (max |i z| + |L|) with TOL_ULPS = 64 (a few
ulps per operand, a handful of operands per term, the V-term log-sum-exp)."""
import json
import math
from pathlib import Path

import pytest
import torch
import yaml

import _refs64 as R
import _refs64_gkd as RG

from distributed_llm_alignment_amd import ops
from distributed_llm_alignment_amd.data import TeacherRolloutDataset, write_jsonl
from distributed_llm_alignment_amd.models import ByteTokenizer, build_model, get_config
from distributed_llm_alignment_amd.objectives import chunked_gkd, gkd_loss, gkd_position_mask
from distributed_llm_alignment_amd.training import train_distill

ROOT = Path(__file__).resolve().parents[1]
TOL_ULPS = 64.0


def _tol(c, it, ref):
    fin = torch.isfinite(c["s"].float())
    zmax = max(c["s"].float()[fin].abs().max().item(), c["t"].float()[torch.isfinite(c["t"].float())].abs().max().item())
    return TOL_ULPS * R.EPS32 * (zmax * it + ref.abs().max().item())


@pytest.mark.parametrize("tau", RG.TEMPS)
@pytest.mark.parametrize("beta", RG.BETAS)
def test_cpu_formula_against_fp64(beta, tau):
    it = RG.inv32(tau)
    for K in (1, 3):
        c = RG.case(9, 1003, K, beta)
        ref = RG.forward(c["s"], c["t"], beta, it)["loss"]
        got = ops.generalized_jsd(c["s"], c["t"], beta=beta, temperature=tau)
        assert got.dtype == torch.float32 and got.shape == (9,)
        err = (got.double() - ref).abs().max().item()
        print(f"FIG cpu generalized_jsd beta {beta} T {tau} K {K}: err {err:.3e} tol {_tol(c, it, ref):.3e}")
        assert err <= _tol(c, it, ref)


@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_cpu_gap_row_stays_finite(beta):
    """Student and teachers put +100 on different entries at i = 2: 200 nats apart. The log-domain
    formula stays finite in fp32 where log(exp(.)) of an underflowed probability does not."""
    c = RG.gap_case(3, beta)
    ref = RG.forward(c["s"], c["t"], beta, 2.0)["loss"]
    got = ops.generalized_jsd(c["s"], c["t"], beta=beta, temperature=0.5)
    assert torch.isfinite(got).all()
    assert (got.double() - ref).abs().max().item() <= _tol(c, 2.0, ref)


@pytest.mark.parametrize("tau", [1.0, 0.9])
@pytest.mark.parametrize("beta", RG.BETAS)
def test_cpu_autograd_against_closed_form(beta, tau):
    """Rows without -inf: autograd of the CPU formula equals the closed form of the docstring."""
    it = RG.inv32(tau)
    g = R.gen(5)
    s = (3.0 * torch.randn(5, 257, generator=g)).bfloat16().float().requires_grad_(True)
    t = (2.0 * torch.randn(2, 5, 257, generator=g)).bfloat16()
    up = torch.randn(5, generator=g)
    (ga,) = torch.autograd.grad(ops.generalized_jsd(s, t, beta=beta, temperature=tau), s, up)
    ref = RG.grad(s.detach(), t, beta, it, up)
    scale = ref.abs().max().item()
    assert (ga.double() - ref).abs().max().item() <= TOL_ULPS * R.EPS32 * max(scale, 1.0)


def test_cpu_dead_entries_get_zero_gradient():
    c = RG.case(9, 1003, 3, 0.5)
    s = c["s"].float().requires_grad_(True)
    (ga,) = torch.autograd.grad(ops.generalized_jsd(s, c["t"], beta=0.5, temperature=0.9), s, c["g"])
    dead = c["s"].float() == R.NINF
    assert dead.any() and torch.isfinite(ga).all() and (ga[dead] == 0).all()


def test_beta0_temperature1_is_ensemble_kl():
    c = R.ensemble_case(33, 1003, 3)
    a = ops.generalized_jsd(c["s"], c["t"], beta=0.0, temperature=1.0)
    b = ops.ensemble_kl(c["s"], c["t"])
    ref = R.ensemble_kl64(c["s"], c["t"], c["g"])["kl"]
    tol = TOL_ULPS * R.EPS32 * (c["s"].float().abs().max().item() + ref.abs().max().item())
    assert (a.double() - ref).abs().max().item() <= tol and (a - b).abs().max().item() <= 2 * tol


def test_row_mask_zeros_rows():
    c = RG.case(9, 1003, 1, 0.5)
    mask = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1, 0], dtype=torch.float32)
    s = c["s"].float().requires_grad_(True)
    full = ops.generalized_jsd(s, c["t"], beta=0.5, temperature=0.9)
    got = ops.generalized_jsd(s, c["t"], beta=0.5, temperature=0.9, row_mask=mask)
    assert (got[mask == 0] == 0).all() and torch.equal(got[mask != 0], full[mask != 0])
    (ga,) = torch.autograd.grad(got, s, c["g"])
    assert (ga[mask == 0] == 0).all() and ga[mask != 0].abs().sum() > 0
    assert torch.equal(got, ops.generalized_jsd(s, c["t"], beta=0.5, temperature=0.9, row_mask=mask.to(torch.uint8)))


@pytest.mark.parametrize("bad", [dict(beta=-0.1), dict(beta=1.5), dict(temperature=0.0), dict(temperature=math.inf)])
def test_bad_scalars_raise(bad):
    c = RG.case(1, 1000, 1, 0.5)
    with pytest.raises(ValueError):
        ops.generalized_jsd(c["s"], c["t"], **bad)


# ----------------------------------------------------------------------------------- objectives
@pytest.fixture(scope="module")
def tiny():
    cfg = get_config("tiny-llama")
    student = build_model(cfg, device="cpu", seed=0)
    teachers = [build_model(cfg, device="cpu", seed=s).requires_grad_(False) for s in (1, 2)]
    return cfg, student, teachers


def test_chunked_gkd_equals_unchunked(tiny):
    cfg, student, teachers = tiny
    g = R.gen(3)
    N = 10
    ths = [torch.randn(N, cfg.hidden_size, generator=g).to(student.head_weight.dtype) for _ in teachers]
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 0, 1, 1, 1], dtype=torch.float32)
    res = []
    for chunk in (None, 4):
        hs = torch.randn(N, cfg.hidden_size, generator=R.gen(4)).to(student.head_weight.dtype).requires_grad_(True)
        L = chunked_gkd(student, teachers, hs, ths, 0.5, 0.9, mask, chunk=chunk)
        student.zero_grad()
        (mask * L).sum().backward()
        res.append((L.detach(), hs.grad.clone(), student.head_weight.grad.clone()))
    # the same products, but the CPU GEMM of another row count may sum them in another order
    for a, b in zip(*res):
        assert (a.double() - b.double()).abs().max().item() <= TOL_ULPS * R.EPS32 * max(b.abs().max().item(), 1.0)
    assert (res[0][0][mask == 0] == 0).all()


def test_position_mask_right_and_left_padded():
    # right-padded dataset rows, T = 6: prompt only (5 real, prompt 5 -> clipped by last - 1),
    # response of one token, full row
    am = torch.tensor([[1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    got = gkd_position_mask(am, torch.tensor([5, 3, 2]))
    want = torch.tensor([[0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 1, 1, 1, 1, 0]], dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    # left-padded generated rows, Tp = 4, two new tokens: 1 pad + 3 prompt, EOS after one token, no pad
    am = torch.tensor([[0, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1]])
    got = gkd_position_mask(am, torch.tensor([3, 2, 4]))
    want = torch.tensor([[0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 1, 0]], dtype=torch.float32)
    assert torch.equal(got, want)
    # an int prompt_len, a prompt-only left-padded row and an empty row
    am = torch.tensor([[0, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]])
    want = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 0]], dtype=torch.float32)
    assert torch.equal(gkd_position_mask(am, 2), want)


def test_gkd_loss_is_masked_mean_and_checks(tiny):
    cfg, student, teachers = tiny
    g = R.gen(9)
    ids = torch.randint(3, cfg.vocab_size, (2, 12), generator=g)
    am = torch.ones(2, 12, dtype=torch.long)
    am[1, 9:] = 0
    loss = gkd_loss(student, teachers, ids, am, torch.tensor([4, 3]), 0.5, 0.9)
    assert loss.dim() == 0 and torch.isfinite(loss) and loss.item() > 0
    loss.backward()
    assert student.head_weight.grad is not None and torch.isfinite(student.head_weight.grad).all()
    student.zero_grad()
    with pytest.raises(ValueError):
        gkd_loss(student, [], ids, am, 4, 0.5, 0.9)
    other = build_model(get_config("tiny-llama", vocab_size=cfg.vocab_size + 8), device="cpu", seed=3)
    with pytest.raises(ValueError):
        gkd_loss(student, [other], ids, am, 4, 0.5, 0.9)
    for attr, val in (("vocab_parallel", (0, cfg.vocab_size)), ("sp", object())):
        setattr(student, attr, val)
        try:
            with pytest.raises(ValueError):
                gkd_loss(student, teachers, ids, am, 4, 0.5, 0.9)
        finally:
            setattr(student, attr, None)


# ---------------------------------------------------------------------------------------- data
def test_dataset_with_prompt_fields(tmp_path):
    tok = ByteTokenizer()
    recs = [{"prompt": " why? ", "teacher_response": "because", "reward": 0.5}, {"prompt": "c", "teacher_response": "dd"}]
    plain = TeacherRolloutDataset(tokenizer=tok, max_length=32, records=recs)
    ds = TeacherRolloutDataset(tokenizer=tok, max_length=32, records=recs, with_prompt=True)
    assert set(plain[0]) == {"input_ids", "attention_mask", "labels", "reward"}
    for i in range(2):
        a, b = plain[i], ds[i]
        assert set(b) == set(a) | {"index", "prompt_len"}
        for k in a:
            assert torch.equal(a[k], b[k])
        assert b["index"].dim() == 0 and b["index"].dtype == torch.long and int(b["index"]) == i
        assert b["prompt_len"].dim() == 0 and b["prompt_len"].dtype == torch.long
    assert int(ds[0]["prompt_len"]) == len(tok("why?\n\n")["input_ids"])
    assert ds.prompt_text(0) == "why?\n\n"
    batch = ds.collate([ds[0], ds[1]])
    assert batch["index"].tolist() == [0, 1] and batch["prompt_len"].shape == (2,)
    short = TeacherRolloutDataset(tokenizer=tok, max_length=4, records=recs, with_prompt=True)[0]
    assert int(short["prompt_len"]) == len(short["input_ids"]) - 1  # clipped: one response position stays


# ------------------------------------------------------------------------------------- trainer
def _base(tmp, **gkd):
    return {"model": {"student_model_name_or_path": "tiny-llama", "max_seq_length": 64},
            "distill": {"teacher_model_name_or_path": "tiny-llama", "gkd": {"enabled": True, **gkd}},
            "data": {"teacher_samples_path": str(Path(tmp) / "r.jsonl"), "num_workers": 0},
            "optimization": {"micro_batch_size": 2, "learning_rate": 1e-3, "max_train_steps": 3},
            "logging": {"output_dir": str(Path(tmp) / "ck"), "log_dir": str(Path(tmp) / "logs"),
                        "log_every_steps": 1, "save_every_steps": 0}}


def _edit(cfg, path, value):
    *head, last = path.split(".")
    d = cfg
    for k in head:
        d = d.setdefault(k, {})
    d[last] = value
    return cfg


@pytest.mark.parametrize("path,value", [
    ("distill.gkd.beta", -0.1), ("distill.gkd.beta", 1.1), ("distill.gkd.lmbda", -0.5), ("distill.gkd.lmbda", 2.0),
    ("distill.gkd.temperature", 0.0), ("distill.gkd.temperature", -1.0), ("distill.gkd.temperature", float("inf")),
    ("distill.gkd.temperature", float("nan")), ("distill.teacher_model_name_or_path", None),
    ("hardware.tp_size", 2), ("hardware.sp_size", 2), ("hardware.zero_stage", 3),
    ("hardware.fsdp", {"sharding_strategy": "FULL_SHARD"}), ("distill.use_kl", True), ("distill.gkd.betta", 0.5),
])
def test_startup_errors(tmp_path, path, value):
    cfg = _edit(_base(tmp_path, lmbda=0.5), path, value)
    with pytest.raises(ValueError):
        train_distill.gkd_settings(cfg)
    p = tmp_path / "bad.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError):  # and from the entry point, before anything is loaded
        train_distill.main(["--config", str(p)])


def test_settings_defaults_and_off(tmp_path):
    assert train_distill.gkd_settings({"distill": {"use_kl": True}}) is None
    assert train_distill.gkd_settings(_edit(_base(tmp_path), "distill.gkd.enabled", False)) is None
    g = train_distill.gkd_settings(_base(tmp_path))
    assert (g["beta"], g["lmbda"], g["temperature"], g["max_new_tokens"], g["top_p"], g["top_k"]) == (0.5, 0.5, 0.9, 128, 1.0, 0)
    # ZeRO-3 is only refused for student rollouts
    assert train_distill.gkd_settings(_edit(_base(tmp_path, lmbda=0.0), "hardware.zero_stage", 3))["lmbda"] == 0.0


@pytest.mark.parametrize("lmbda", [0.0, 1.0])
def test_trainer_three_steps(tmp_path, lmbda):
    from distributed_llm_alignment_amd.data.synthetic import synthetic_prompt_records

    recs = [{"prompt": r["prompt"], "teacher_response": "a short answer", "reward": 0.25}
            for r in synthetic_prompt_records(6, seed=4)]
    write_jsonl(tmp_path / "r.jsonl", recs)
    cfg = _base(tmp_path, lmbda=lmbda, max_new_tokens=6)
    p = tmp_path / "gkd.yaml"
    p.write_text(yaml.safe_dump(cfg))
    assert train_distill.main(["--config", str(p)]) == 0
    m = [json.loads(l) for l in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines()]
    m = [r for r in m if "train/loss" in r]
    assert len(m) == 3
    for r in m:
        assert math.isfinite(r["train/loss"]) and r["train/gkd_on_policy"] == lmbda
        assert r["train/reward_mean"] == pytest.approx(0.25)
        assert (0 < r["train/gkd_gen_len"] <= 6) if lmbda else r["train/gkd_gen_len"] == 0
    assert (tmp_path / "ck" / "final" / "model_1.safetensors").exists()  # student, then the teacher


def test_shipped_config_loads():
    from distributed_llm_alignment_amd.utils.config import load_config

    cfg = load_config(ROOT / "config" / "distill_gkd.yaml")
    g = train_distill.gkd_settings(cfg)
    assert g is not None and g["beta"] == 0.5 and g["lmbda"] == 0.5 and g["temperature"] == 0.9
    assert train_distill.teacher_paths(cfg) == ["checkpoints/dpo/latest"]
