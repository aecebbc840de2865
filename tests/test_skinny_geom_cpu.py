"""Launch geometry of the decode projection GEMMs (csrc/skinny_geom.h) against a recorded table.

The GPU tests compare the projections with fp32 references at tolerances, so a changed split count,
kernel family, waves-per-workgroup or ring-depth choice would pass them while changing the
summation order and the speed. Here a small driver is compiled with g++ against the header (pure
host C++) and every row of tests/golden/skinny_geometry.json must come out as recorded, under each
environment setting the launchers read (once per process, so one driver run per setting)."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "distributed_llm_alignment_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "skinny_geometry.json"
ENV_KEYS = ("DLA_SKINNY_WG", "DLA_M64_WG", "DLA_SKINNY_DEEP_K", "DLA_KS_F8_DEPTH", "DLA_GLU_IL_DEPTH",
            "DLA_GLU_IL_F8_DEPTH", "DLA_GLU_IL_WAVES", "DLA_M64_F8_DEPTH")

GRID = {
    "splits": {"M": [1, 8, 16], "N": [16, 128, 4096, 6144, 14336, 16256, 16384, 28672, 128256],
               "K": [256, 512, 1024, 4096, 8192, 14336]},
    "m64": {"N": [128, 1024, 4096, 6144, 14336, 28672], "K": [256, 512, 1024, 1792, 2048, 3584, 4096, 14336],
            "cus": [256, 304, 64]},
    "glu_il": {"ntiles": [1, 8, 255, 1024, 1792, 2048, 3584], "M": [1, 16]},
    "depth": {"K": [4096, 8191, 8192, 14336]},
}
SETTINGS = [{}, {"DLA_SKINNY_WG": "128"}, {"DLA_SKINNY_WG": "512"}, {"DLA_M64_WG": "192"}, {"DLA_M64_WG": "384"},
            {"DLA_SKINNY_DEEP_K": "4096"}, {"DLA_KS_F8_DEPTH": "4"}, {"DLA_GLU_IL_DEPTH": "3"},
            {"DLA_GLU_IL_DEPTH": "9"}, {"DLA_GLU_IL_F8_DEPTH": "1"}, {"DLA_GLU_IL_WAVES": "4"},
            {"DLA_GLU_IL_WAVES": "7"}, {"DLA_M64_F8_DEPTH": "2"}, {"DLA_M64_F8_DEPTH": "5"}]

# stdin -> stdout, one line each:
#   "S M N K"      -> skinny_splits, LDS bytes of x at that split
#   "U N K"        -> skinny_use_ksplit skinny_glu_ks_ok m64_shape_ok
#   "M N K cus"    -> m64_splits
#   "W ntiles M"   -> glu_il_waves on the bf16 weight, on the fp8 weight
#   "D K"          -> skinny_ks_depth skinny_ks_f8_depth glu_il_depth(bf16) glu_il_depth(fp8) m64_f8_depth
#   "C"            -> the LDS limits and the m64 ring sizes at 2 and 4 row tiles
DRIVER = r"""
#include <cstdio>
#include "skinny_geom.h"
using namespace dla;
int main() {
  char kind;
  int a, b, c;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'S') {
      if (scanf("%d %d %d", &a, &b, &c) != 3) return 1;
      const int s = skinny_splits(a, b, c);
      printf("%d %lld\n", s, (long long)skinny_lds_bytes(a, c / s));
    } else if (kind == 'U') {
      if (scanf("%d %d", &a, &b) != 2) return 1;
      printf("%d %d %d\n", (int)skinny_use_ksplit(a, b), (int)skinny_glu_ks_ok(a, b), (int)m64_shape_ok(a, b));
    } else if (kind == 'M') {
      if (scanf("%d %d %d", &a, &b, &c) != 3) return 1;
      printf("%d\n", m64_splits(a, b, c));
    } else if (kind == 'W') {
      if (scanf("%d %d", &a, &b) != 2) return 1;
      printf("%d %d\n", glu_il_waves(a, b, false), glu_il_waves(a, b, true));
    } else if (kind == 'D') {
      if (scanf("%d", &a) != 1) return 1;
      printf("%d %d %d %d %d\n", skinny_ks_depth(a), skinny_ks_f8_depth(), glu_il_depth(false), glu_il_depth(true),
             m64_f8_depth());
    } else {
      printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)kSkLdsMax, (long long)kSkLdsGluMax,
             (long long)kSkLdsNormMax, (long long)kSkLdsNormX, (long long)kM64LdsMax,
             (long long)m64_lds_bytes(m64_row_tiles(17)), (long long)m64_lds_bytes(m64_row_tiles(33)));
    }
  }
  return 0;
}
"""


def grid(spec):
    """Driver input lines of the recorded grid."""
    s, m, w = spec["splits"], spec["m64"], spec["glu_il"]
    lines = [f"S {M} {N} {K}" for M in s["M"] for N in s["N"] for K in s["K"]]
    lines += [f"U {N} {K}" for N in s["N"] for K in s["K"]]
    lines += [f"M {N} {K} {cus}" for N in m["N"] for K in m["K"] for cus in m["cus"]]
    lines += [f"W {t} {M}" for t in w["ntiles"] for M in w["M"]]
    lines += [f"D {K}" for K in spec["depth"]["K"]]
    return lines + ["C"]


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
    return compile_driver(DRIVER, tmp_path_factory.mktemp("skinny_geom") / "driver")


def test_header_is_pure_host_cpp():
    text = (CSRC / "skinny_geom.h").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i in ("<algorithm>", "<cstdint>", "<cstdlib>") for i in includes), includes


def test_each_switch_has_one_reader():
    """Every DLA_* switch of the projection launchers is read in skinny_geom.h, once, and nowhere
    else in the sources of the decode projections."""
    geom = (CSRC / "skinny_geom.h").read_text()
    rest = "".join((CSRC / f).read_text() for f in ("skinny.hip", "skinny64.hip", "skinny_ks.h", "skinny_params.h",
                                                   "bindings_decode.cpp"))
    for key in ENV_KEYS:
        assert geom.count(f'skinny_env("{key}"') == 1, key
        assert f'"{key}"' not in rest, key
    assert geom.count("getenv(") == 1  # the helper


def test_recorded_settings_and_grid(golden):
    """The table holds the settings and shapes it is meant to."""
    assert golden["grid"] == GRID
    assert [s["env"] for s in golden["settings"]] == SETTINGS
    n = len(grid(GRID))
    assert all(len(s["rows"]) == n for s in golden["settings"])
    assert GOLDEN.stat().st_size < 100 * 1024


@pytest.mark.parametrize("index", range(len(SETTINGS)))
def test_geometry_matches_recorded_table(golden, driver, index):
    setting = golden["settings"][index]
    lines = grid(golden["grid"])
    got = run(driver, lines, setting["env"])
    assert len(got) == len(lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, setting["rows"]) if g != w]
    assert not bad, f"{setting['env']}: {len(bad)} rows differ, first {bad[:3]}"
