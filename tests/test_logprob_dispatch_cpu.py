"""CPU tier: `ops.logprob.rows_fwd` / `rows_bwd` pick the LM-head row op and its positional arguments.

The tables below are written out from the if-ladders these two functions replaced (in
`_LinearLogprobFn`, `_LinearLogprobEntropyFn` and the vocab-parallel `_local_*` helpers): one row per
{inv_temp None / value} x {keep or not} x {entropy (forward) / grad_ent (backward) or not} x {off 0 /
nonzero} (x {transposed or not} for the backward). A row maps to (op name, positional arguments), or to
None where no op exists: the keep ops take an inv_temp and neither the entropy nor a vocab shard. A
zero vocab offset is the schemas' default and is not passed.
"""
import itertools

import pytest

from distributed_llm_alignment_amd.ops import _ext
from distributed_llm_alignment_amd.ops import logprob as L

# the ops record their arguments and do nothing else, so plain strings stand in for the tensors
LG, TG, LSE, ENT, G, GE, K, KR = "logits", "targets", "lse", "ent", "g", "ge", "keep", "keep_rows"
IT, OFF = 0.7, 1024

# (inv_temp, keep, entropy, off) -> (op, args)
FWD = {
    (None, False, False, 0): ("logprob_fwd", (LG, TG)),
    (None, False, False, OFF): ("logprob_fwd", (LG, TG, OFF)),
    (None, False, True, 0): ("logprob_entropy_fwd", (LG, TG)),
    (None, False, True, OFF): ("logprob_entropy_fwd", (LG, TG, OFF)),
    (IT, False, False, 0): ("logprob_fwd_temp", (LG, TG, IT)),
    (IT, False, False, OFF): ("logprob_fwd_temp", (LG, TG, IT, OFF)),
    (IT, False, True, 0): ("logprob_entropy_fwd_temp", (LG, TG, IT)),
    (IT, False, True, OFF): ("logprob_entropy_fwd_temp", (LG, TG, IT, OFF)),
    (IT, True, False, 0): ("logprob_fwd_keep", (LG, TG, K, KR, IT)),
    (IT, True, False, OFF): None,
    (IT, True, True, 0): None,
    (IT, True, True, OFF): None,
    (None, True, False, 0): None,
    (None, True, False, OFF): None,
    (None, True, True, 0): None,
    (None, True, True, OFF): None,
}

# (inv_temp, keep, grad_ent given, transposed, off) -> (op, args)
BWD = {
    (None, False, False, False, 0): ("logprob_bwd", (LG, TG, LSE, G)),
    (None, False, False, False, OFF): ("logprob_bwd", (LG, TG, LSE, G, OFF)),
    (None, False, False, True, 0): ("logprob_bwd_t", (LG, TG, LSE, G)),
    (None, False, False, True, OFF): ("logprob_bwd_t", (LG, TG, LSE, G, OFF)),
    (None, False, True, False, 0): ("logprob_entropy_bwd", (LG, TG, LSE, ENT, G, GE)),
    (None, False, True, False, OFF): ("logprob_entropy_bwd", (LG, TG, LSE, ENT, G, GE, OFF)),
    (None, False, True, True, 0): ("logprob_entropy_bwd_t", (LG, TG, LSE, ENT, G, GE)),
    (None, False, True, True, OFF): ("logprob_entropy_bwd_t", (LG, TG, LSE, ENT, G, GE, OFF)),
    (IT, False, False, False, 0): ("logprob_bwd_temp", (LG, TG, LSE, G, IT)),
    (IT, False, False, False, OFF): ("logprob_bwd_temp", (LG, TG, LSE, G, IT, OFF)),
    (IT, False, False, True, 0): ("logprob_bwd_t_temp", (LG, TG, LSE, G, IT)),
    (IT, False, False, True, OFF): ("logprob_bwd_t_temp", (LG, TG, LSE, G, IT, OFF)),
    (IT, False, True, False, 0): ("logprob_entropy_bwd_temp", (LG, TG, LSE, ENT, G, GE, IT)),
    (IT, False, True, False, OFF): ("logprob_entropy_bwd_temp", (LG, TG, LSE, ENT, G, GE, IT, OFF)),
    (IT, False, True, True, 0): ("logprob_entropy_bwd_t_temp", (LG, TG, LSE, ENT, G, GE, IT)),
    (IT, False, True, True, OFF): ("logprob_entropy_bwd_t_temp", (LG, TG, LSE, ENT, G, GE, IT, OFF)),
    (IT, True, False, False, 0): ("logprob_bwd_keep", (LG, TG, LSE, G, K, KR, IT)),
    (IT, True, False, True, 0): ("logprob_bwd_t_keep", (LG, TG, LSE, G, K, KR, IT)),
    (IT, True, False, False, OFF): None,
    (IT, True, False, True, OFF): None,
    (IT, True, True, False, 0): None,
    (IT, True, True, False, OFF): None,
    (IT, True, True, True, 0): None,
    (IT, True, True, True, OFF): None,
    (None, True, False, False, 0): None,
    (None, True, False, False, OFF): None,
    (None, True, False, True, 0): None,
    (None, True, False, True, OFF): None,
    (None, True, True, False, 0): None,
    (None, True, True, False, OFF): None,
    (None, True, True, True, 0): None,
    (None, True, True, True, OFF): None,
}


class _Recorder:
    """Stands in for `torch.ops.dla`: every attribute is an op that records (name, args, kwargs)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def op(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return ("out", name)
        return op


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_ext, "require", lambda: r)
    return r


def test_tables_are_complete():
    assert set(FWD) == set(itertools.product((None, IT), (False, True), (False, True), (0, OFF)))
    assert set(BWD) == set(itertools.product((None, IT), (False, True), (False, True), (False, True), (0, OFF)))
    # each of the 15 ops appears
    assert len({v[0] for v in list(FWD.values()) + list(BWD.values()) if v}) == 15


@pytest.mark.parametrize("key", list(FWD), ids=str)
def test_rows_fwd(rec, key):
    it, keep, entropy, off = key
    kw = dict(inv_temp=it, off=off, keep=K if keep else None, keep_rows=KR if keep else None, entropy=entropy)
    if FWD[key] is None:
        with pytest.raises(ValueError):
            L.rows_fwd(LG, TG, **kw)
        assert rec.calls == []
        return
    name, args = FWD[key]
    assert L.rows_fwd(LG, TG, **kw) == ("out", name)
    assert rec.calls == [(name, args, {})]


@pytest.mark.parametrize("key", list(BWD), ids=str)
def test_rows_bwd(rec, key):
    it, keep, with_ge, transposed, off = key
    # the saved entropy is passed whether or not a gradient arrives for it, as the Functions do
    kw = dict(ent=ENT, ge=GE if with_ge else None, inv_temp=it, off=off, keep=K if keep else None,
              keep_rows=KR if keep else None, transposed=transposed)
    if BWD[key] is None:
        with pytest.raises(ValueError):
            L.rows_bwd(LG, TG, LSE, G, **kw)
        assert rec.calls == []
        return
    name, args = BWD[key]
    out = L.rows_bwd(LG, TG, LSE, G, **kw)
    assert out == (("out", name) if transposed else None)  # dlogits^T, or None after the in-place op
    assert rec.calls == [(name, args, {})]


def test_keep_without_keep_rows_raises(rec):
    with pytest.raises(ValueError):
        L.rows_fwd(LG, TG, inv_temp=IT, keep=K)
    with pytest.raises(ValueError):
        L.rows_bwd(LG, TG, LSE, G, inv_temp=IT, keep_rows=KR)
    assert rec.calls == []
