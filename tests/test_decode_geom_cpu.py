"""Split geometry of the decode attention launches (csrc/decode_geom.h) against a recorded table.

The GPU tests compare decode attention with tolerances, so a changed split choice (chunks per
block, number of partial slots, fused or separate combine) would pass them while changing the
summation order and the speed. Here a small driver is compiled with g++ against the header (pure
host C++) and every row of tests/golden/decode_geometry.json must come out as recorded, under each
environment setting the launchers read."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "distributed_llm_alignment_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "decode_geometry.json"
ENV_KEYS = ("DLA_DECODE_LOOP", "DLA_DECODE_BLOCKS", "DLA_DECODE_LOOP_MIN")

# stdin: "R Tmax B Hkv" -> "cpb nsplit"; "G Tmax B Hq Hkv G Tp" -> the nine DecGroupGeom fields
DRIVER = r"""
#include <cstdio>
#include "decode_geom.h"
int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'R') {
      int Tmax, B, Hkv;
      if (scanf("%d %d %d", &Tmax, &B, &Hkv) != 3) return 1;
      printf("%d %d\n", dla::decode_cpb(Tmax, B, Hkv), dla::decode_num_splits(Tmax, B, Hkv));
    } else {
      int Tmax, B, Hq, Hkv, G, Tp;
      if (scanf("%d %d %d %d %d %d", &Tmax, &B, &Hq, &Hkv, &G, &Tp) != 6) return 1;
      const dla::DecGroupGeom g = dla::decode_group_geom(Tmax, B, Hq, Hkv, G, Tp);
      printf("%d %d %d %d %d %d %d %d %d\n", g.rpt, g.ntile, g.nt, g.cpb_p, g.cpb_s, g.npre, g.nsuf, g.c0,
             (int)g.fuse);
    }
  }
  return 0;
}
"""


def grid(spec):
    """Driver input lines of the recorded grid, per-row shapes first."""
    r, g = spec["rows"], spec["group"]
    lines = [f"R {T} {B} {Hkv}" for T in r["Tmax"] for B in r["B"] for Hkv in r["Hkv"]]
    n_rows = len(lines)
    for T in g["Tmax"]:
        for Tp in sorted({t for t in g["Tp"] + [T] if t <= T}):
            for G, P, Hkv in zip(g["G"], g["P"], g["Hkv"]):  # prompts and kv heads vary with G
                for ratio in g["ratio"]:
                    lines.append(f"G {T} {P * G} {ratio * Hkv} {Hkv} {G} {Tp}")
    return lines, n_rows


def run(exe, lines, setting):
    env = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
    env.update(setting)
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", env=env, capture_output=True, text=True,
                         check=True, timeout=60).stdout
    return [[int(x) for x in ln.split()] for ln in out.splitlines()]


def compile_driver(source, out, include=CSRC):
    src = out.with_suffix(".cpp")
    src.write_text(source)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{include}", str(src), "-o", str(out)],
                   check=True, capture_output=True, text=True, timeout=120)
    return out


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    return compile_driver(DRIVER, tmp_path_factory.mktemp("decode_geom") / "driver")


def test_header_is_pure_host_cpp():
    text = (CSRC / "decode_geom.h").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i in ("<algorithm>", "<cstdint>", "<cstdlib>") for i in includes), includes


def test_recorded_settings_and_grid(golden):
    """The table holds the settings and boundary shapes it is meant to."""
    got = {tuple(sorted(s["env"].items())) for s in golden["settings"]}
    want = [{}, {"DLA_DECODE_LOOP": "0"}] + [{"DLA_DECODE_BLOCKS": b} for b in ("2", "4", "16", "60")] + [
        {"DLA_DECODE_LOOP_MIN": m} for m in ("1", "3")]
    assert got == {tuple(sorted(w.items())) for w in want}
    r, g = golden["grid"]["rows"], golden["grid"]["group"]
    assert r == {"Tmax": [1, 127, 128, 129, 256, 640, 1024, 1152, 1153, 4096, 8192], "B": [1, 5, 8, 48, 64],
                 "Hkv": [1, 2, 8]}
    assert g["G"] == [1, 5, 8, 16, 64] and g["ratio"] == [1, 4, 8]
    assert {127, 128, 129} <= set(g["Tp"]) and {127, 128, 129} <= set(g["Tmax"])
    lines, n_rows = grid(golden["grid"])
    default = golden["settings"][0]
    assert default["env"] == {} and len(default["rows"]) == n_rows
    assert len(default["group"]) == len(lines) - n_rows
    # rows where the suffix alone takes every slot of the in-kernel combine (nsuf >= kDecMaxFuse = 8)
    assert any(row[6] >= 8 and row[8] == 0 for row in default["group"])
    assert GOLDEN.stat().st_size < 100 * 1024


@pytest.mark.parametrize("index", range(8))
def test_geometry_matches_recorded_table(golden, driver, index):
    setting = golden["settings"][index]
    lines, n_rows = grid(golden["grid"])
    got = run(driver, lines, setting["env"])
    assert len(got) == len(lines)
    want = setting["rows"] + setting["group"]
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, f"{setting['env']}: {len(bad)} rows differ, first {bad[:3]}"
