"""The host arithmetic the replicate-simulation entry points share, compiled from the library's own headers by
tests/cpp/replicate_passes.cpp: tile_geometry of conditional-ude_amd/csrc/cude_tilesort.h against the table of
tests/test_tilesort_host.py (lds = 8 Kp C), subject_passes of csrc/cude_passes.h against the expressions it replaced in
cude_predictive_bands, cude_bootstrap_conditional and cude_npde -- over N in {1, 57, 64, 65, 700, 100000}, option caps
{0, 1, 64, 65, 1000} and budgets that give one workgroup per pass, a few, and all -- and against what passes must be:
[0, N) exactly once, in order, every start a multiple of 64.  Built twice: plain, and with -fsanitize=address,undefined
(plain host code, a program of its own; a host compiler without the sanitizers' runtimes fails that test, it does not skip)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "replicate_passes.cpp")
INC = os.path.join(ROOT, "conditional-ude_amd", "csrc")


def _run(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines()}
    assert set(out) == {"tile_geometry", "subject_passes", "ranks_increasing"}
    assert all(v[0] == "1" for v in out.values()), out
    import test_tilesort_host as ts
    assert int(out["tile_geometry"][1]) == 4 * len(ts.TABLE)           # Kp, C, 1 << lgC, lds of every K of the table
    # 6 N x 5 caps x 3 K x 3 budgets x 3 call sites; per set of passes 2 comparisons and 4 per pass
    assert int(out["subject_passes"][2]) == 6 * 5 * 3 * 3 * 3
    assert int(out["subject_passes"][1]) > 6 * int(out["subject_passes"][2])
    assert int(out["ranks_increasing"][1]) == 6


def test_the_driver_states_the_table_of_the_tile_test():
    import test_tilesort_host as ts
    src = open(SRC).read()
    for K, (Kp, C) in ts.TABLE.items():
        assert f"{{{K}, {Kp}, {C}}}" in src, K


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_geometry_and_passes_equal_the_expressions_they_replaced(tmp_path):
    exe = str(tmp_path / "replicate_passes")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_geometry_and_passes_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "replicate_passes_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    _run(exe)
