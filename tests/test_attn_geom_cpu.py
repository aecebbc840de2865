"""Launch plan of the training attention (csrc/attn_geom.h) against a recorded table.

The GPU tests compare attn_fwd / attn_bwd with tolerances, so a changed launch decision (heads per
workgroup, persistent or not, the backward's head split, bf16 or fp32 scratch, a reduce grid) would
pass them while changing the summation order, the rounding points and the speed. Here a small
driver is compiled with g++ against the header (pure host C++) and every row of
tests/golden/attn_geometry.json must come out as recorded, under each environment setting the plan
reads, one fresh process per setting (DLA_ATTN_FWD_HP is read once per process). The table was
recorded from the launch code as it stood before the plan header existed, not from the header.

Grid (golden["grid"]): every (Tq, Tk) against every head shape; forward rows take each of
non-causal / causal / causal with a shared prefix (the prefix needs Tq == Tk) with the head dim
cycling, backward rows take every head dim, causal and not, with the fused RoPE backward (full
rotary, 32 of 80 dims at D = 80) on every other row. B x cus is thinned to a cycle over its nine
pairs, which keeps the file under 100 KB. A forward setting records forward rows only, a backward
setting backward rows only."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

import _attn_ref64 as R

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "distributed_llm_alignment_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "attn_geometry.json"
ENV_KEYS = ("DLA_ATTN_FWD_HP", "DLA_ATTN_FWD_PERSIST", "DLA_ATTN_BWD_WAVES", "DLA_ATTN_DQ_BF16",
            "DLA_ATTN_DKV_BF16")
SETTINGS = [{}, {"DLA_ATTN_FWD_HP": "1"}, {"DLA_ATTN_FWD_HP": "2"}, {"DLA_ATTN_FWD_PERSIST": "0"},
            {"DLA_ATTN_FWD_PERSIST": "1"}, {"DLA_ATTN_BWD_WAVES": "4"}, {"DLA_ATTN_DQ_BF16": "0"},
            {"DLA_ATTN_DKV_BF16": "0"}]
FWD_COLS = ("hp", "bq", "nblk", "persist", "grid")
BWD_COLS = ("waves", "nkb", "slab_rows", "slab16", "hsplit", "part16", "delta_grid", "grid", "dq_grid", "dkv_grid")

# stdin: "F B Hq Hkv Tq Tk D causal prefix cus" -> FWD_COLS; "W B Hq Hkv Tq Tk D causal rope rot cus" -> BWD_COLS
DRIVER = r"""
#include <cstdio>
#include "attn_geom.h"
int main() {
  char kind;
  long long B, Hq, Hkv, Tq, Tk;
  int D, causal;
  while (scanf(" %c %lld %lld %lld %lld %lld %d %d", &kind, &B, &Hq, &Hkv, &Tq, &Tk, &D, &causal) == 8) {
    if (kind == 'F') {
      int prefix, cus;
      if (scanf("%d %d", &prefix, &cus) != 2) return 1;
      const dla::AttnFwdPlan g = dla::attn_fwd_plan(B, Hq, Hkv, Tq, Tk, D, causal != 0, prefix != 0, cus);
      printf("%d %d %lld %d %lld\n", g.hp, g.bq, (long long)g.nblk, (int)g.persist, (long long)g.grid);
    } else {
      int rope, rot, cus;
      if (scanf("%d %d %d", &rope, &rot, &cus) != 3) return 1;
      const dla::AttnBwdPlan g = dla::attn_bwd_plan(B, Hq, Hkv, Tq, Tk, D, causal != 0, rope != 0, rot, cus);
      printf("%d %lld %lld %d %d %d %lld %lld %lld %lld\n", g.waves, (long long)g.nkb, (long long)g.slab_rows,
             (int)g.slab16, g.hsplit, (int)g.part16, (long long)g.delta_grid, (long long)g.grid,
             (long long)g.dq_grid, (long long)g.dkv_grid);
    }
  }
  return 0;
}
"""


def grid(spec):
    """Driver input lines of the recorded grid: (forward lines, backward lines)."""
    pairs = [(b, c) for b in spec["B"] for c in spec["cus"]]
    Ds = spec["D"]
    fwd, bwd, m, k = [], [], 0, 0
    for Tq, Tk in spec["T"]:
        for Hq, Hkv in spec["heads"]:
            for mi, (causal, prefix) in enumerate(((0, 0), (1, 0), (1, 1))):
                if prefix and Tq != Tk:
                    continue
                B, cus = pairs[(3 * m + mi) % len(pairs)]
                fwd.append(f"F {B} {Hq} {Hkv} {Tq} {Tk} {Ds[(m + mi) % len(Ds)]} {causal} {prefix} {cus}")
            for di, D in enumerate(Ds):
                for causal in (0, 1):
                    B, cus = pairs[k % len(pairs)]
                    rope = int(Tq == Tk and (m + di + causal) % 2 == 1)
                    bwd.append(f"W {B} {Hq} {Hkv} {Tq} {Tk} {D} {causal} {rope} {D if D != 80 else 32} {cus}")
                    k += 1
            m += 1
    return fwd, bwd


def run(exe, lines, setting):
    env = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
    env.update(setting)
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", env=env, capture_output=True, text=True,
                         check=True, timeout=60).stdout
    return [[int(x) for x in ln.split()] for ln in out.splitlines()]


def compile_driver(source, out, include=CSRC, extra=()):
    src = out.with_suffix(".cpp")
    src.write_text(source)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, f"-I{include}", str(src), "-o", str(out)],
                   check=True, capture_output=True, text=True, timeout=120)
    return out


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    return compile_driver(DRIVER, tmp_path_factory.mktemp("attn_geom") / "driver")


def test_header_is_pure_host_cpp():
    text = (CSRC / "attn_geom.h").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i in ("<algorithm>", "<cstdint>", "<cstdlib>") for i in includes), includes


def test_recorded_settings_and_grid(golden):
    """The table holds the settings, the shapes and the plan branches it is meant to."""
    assert [s["env"] for s in golden["settings"]] == SETTINGS
    spec = golden["grid"]
    same = [1, 31, 32, 33, 255, 256, 257, 512, 513, 1024, 4096]
    assert spec["T"][:len(same)] == [[t, t] for t in same]
    assert len(spec["T"]) == len(same) + 2 and all(tq == 5 and tk > 5 for tq, tk in spec["T"][len(same):])
    assert spec["B"] == [1, 2, 8] and spec["cus"] == [8, 256, 304] and spec["D"] == [64, 80, 128]
    assert spec["heads"] == [[4, 4], [6, 3], [8, 2], [8, 1], [3, 1], [32, 8], [64, 8]]
    fwd, bwd = grid(spec)
    for s in golden["settings"]:
        keys = "".join(s["env"])
        assert len(s.get("fwd", [])) == (0 if "BWD" in keys or "BF16" in keys else len(fwd))
        assert len(s.get("bwd", [])) == (0 if "FWD" in keys else len(bwd))
    # every (T, head shape): backward rows at every D, causal and not; forward rows causal and not
    # and, at Tq == Tk, with a prefix; every (B, cus) pair occurs in both directions
    seen = {}
    for ln in fwd + bwd:
        f = ln.split()
        seen.setdefault((f[0],) + tuple(f[2:6]), set()).add(tuple(f[6:9]))
    for (kind, _, _, tq, tk), v in seen.items():
        if kind == "W":
            assert {(d, c) for d, c, _ in v} == {(str(d), c) for d in spec["D"] for c in "01"}
        else:
            assert {(c, p) for _, c, p in v} == {("0", "0"), ("1", "0")} | ({("1", "1")} if tq == tk else set())
    for lines in (fwd, bwd):
        assert {(int(ln.split()[1]), int(ln.split()[-1])) for ln in lines} == {(b, c) for b in spec["B"]
                                                                               for c in spec["cus"]}
    rows_f = [r for s in golden["settings"] for r in s.get("fwd", [])]
    rows_b = [r for s in golden["settings"] for r in s.get("bwd", [])]
    col = lambda rows, cols, name: {r[cols.index(name)] for r in rows}  # noqa: E731
    assert col(rows_b, BWD_COLS, "hsplit") == {1, 2, 4, 8}
    assert col(rows_f, FWD_COLS, "persist") == {0, 1}
    assert col(rows_f, FWD_COLS, "hp") == {1, 2, 4}
    assert col(rows_b, BWD_COLS, "part16") == {0, 1}
    assert col(rows_b, BWD_COLS, "slab16") == {0, 1} and col(rows_b, BWD_COLS, "waves") == {4, 8}
    assert GOLDEN.stat().st_size < 100 * 1024


@pytest.mark.parametrize("index", range(len(SETTINGS)))
def test_plan_matches_recorded_table(golden, driver, index):
    setting = golden["settings"][index]
    fwd, bwd = grid(golden["grid"])
    lines = (fwd if "fwd" in setting else []) + (bwd if "bwd" in setting else [])
    got = run(driver, lines, setting["env"])
    assert len(got) == len(lines)
    want = setting.get("fwd", []) + setting.get("bwd", [])
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, f"{setting['env']}: {len(bad)} rows differ, first {bad[:3]}"


def test_plan_matches_the_fp64_reference_cases(driver):
    """nkb, hsplit, slab16 and part16 of every case of _attn_ref64.grid() as Case.numerics states
    them (its own statement of the rule, which fixes the rounding points of the fp64 bound)."""
    by_env = {}
    for c in R.grid():
        waves, dq16, dkv16 = c.bwd
        env = (("DLA_ATTN_BWD_WAVES", str(waves)), ("DLA_ATTN_DQ_BF16", str(dq16)), ("DLA_ATTN_DKV_BF16", str(dkv16)))
        by_env.setdefault(env, []).append(c)
    for env, cases in by_env.items():
        for cus in (8, 256):
            lines = [f"W {c.B} {c.Hq} {c.Hkv} {c.Tq} {c.Tk} {c.D} {int(c.causal)} {int(c.rot > 0)} {c.rot} {cus}"
                     for c in cases]
            got = run(driver, lines, dict(env))
            assert len(got) == len(cases)
            for c, row in zip(cases, got):
                g, num = dict(zip(BWD_COLS, row)), c.numerics(cus)
                assert (g["nkb"], g["hsplit"], bool(g["slab16"]), bool(g["part16"])) == (
                    num["nkb"], num["hs"], num["slab16"], num["part16"]), (c.name, cus, g, num)
