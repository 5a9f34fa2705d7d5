"""The context-free launch rules of conditional-ude_amd/csrc/cude_select.hip (sets_per_launch, nearest_divisor,
shared_simd_rate), compiled from that file by tests/cpp/select_rules.cpp and compared there, over a grid of sizes,
budgets and option caps, with the expressions they replaced at their call sites: every integer must be equal.  Built
twice: plain, and with -fsanitize=address,undefined (plain host code, a program of its own)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "select_rules.cpp")
INC = os.path.join(ROOT, "conditional-ude_amd", "csrc")


def _run(exe, env=None):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines()}
    assert set(out) == {"sets_per_launch", "nearest_divisor", "chunk_starts", "shared_simd_rate"}
    assert all(v[0] == "1" for v in out.values()), out
    # 5 n x 6 N x 3 P x (4 uncapped + 4 caps x (2 + 3 budgets x 3) + 3 budgets x 2 splits); 4 S x 2 targets
    assert int(out["sets_per_launch"][1]) == 90 * (4 + 4 * 11 + 6)
    assert int(out["nearest_divisor"][1]) == 8


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_launch_rules_return_the_integers_of_the_expressions_they_replaced(tmp_path):
    exe = str(tmp_path / "select_rules")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_launch_rules_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "select_rules_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr
    _run(exe)
