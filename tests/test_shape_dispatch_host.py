"""The shape dispatch of conditional-ude_amd/csrc/cude_shapes.h (one visitor per shape list, the activation pairs, and the
two-level "general shape x activation pair" visitors), compiled from that header alone by tests/cpp/shape_dispatch.cpp and
compared there, over a grid of shapes, with the if-chains the visitors replaced, expanded by hand from the same list
macros: the callable runs once with the matching tag or not at all, and every result is equal.  The header's own
static_asserts (the c-peptide groups partition their list, ...) are checked by the same compile.  Built twice: plain, and
with -fsanitize=address,undefined (plain host code, a program of its own)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shape_dispatch.cpp")
INC = os.path.join(ROOT, "conditional-ude_amd", "csrc")

GRID = 6 * 10 * 7                   # nin 0..5 x width 0..9 x depth 0..6
PAIRS = 4 * 3                       # hact 0..3 x oact 0..2
# visitor: (comparisons, those with the shape in the list).  The c-peptide lists match on (nin, width, depth): one hit per
# entry; the suppression lists match on (width, depth) alone: one hit per entry and nin of the grid; 5 activation pairs
WANT = {
    "cpep_shapes": (GRID, 24), "cpep_shapes_0": (GRID, 8), "cpep_shapes_1": (GRID, 8), "cpep_shapes_2": (GRID, 8),
    "cpep_general_shapes": (GRID, 3),
    "supp_shapes": (GRID, 16 * 6), "supp_general_shapes": (GRID, 2 * 6), "supp_ad_unrolled": (GRID, 4 * 6),
    "supp_ad_shapes": (GRID, 12 * 6),
    "cpep_general": (GRID * PAIRS, 3 * 5), "supp_general": (GRID * PAIRS, 2 * 6 * 5),
    "general_acts": (PAIRS, 5), "general_acts_compiled": (PAIRS, 5),
}


def _run(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines()}
    assert set(out) == set(WANT)
    assert all(v[0] == "1" for v in out.values()), out
    assert {k: (int(v[1]), int(v[2])) for k, v in out.items()} == WANT


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_visitors_dispatch_as_the_if_chains_they_replaced(tmp_path):
    exe = str(tmp_path / "shape_dispatch")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_visitors_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "shape_dispatch_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_one_body_variant_of_the_lists_compiles(tmp_path):
    """-DCUDE_ADAPT_ONE_BODY (A/B builds): the one-body adaptive kernel takes every suppression shape."""
    exe = str(tmp_path / "shape_dispatch_one_body")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-DCUDE_ADAPT_ONE_BODY", "-I", INC, SRC, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines()}
    assert run.returncode == 0 and out["supp_ad_shapes"] == ["1", str(GRID), str(16 * 6)], run.stdout
