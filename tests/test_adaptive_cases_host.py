"""The inputs of tests/test_gpu_adaptive_shapes.py (tests/adaptive_cases.py) are adequate -- shown on the CPU oracle alone,
so that they cannot degrade without a test saying so: every loss finite, a sensible number of accepted steps, every bias
live, every layer's weight block and bias block of the network gradient within 1e3 of the largest (so that the device
test's max-norm tolerance of 1e-8 says something about each of them), and no accept / reject decision close enough to its
threshold for a relative perturbation of 1e-9 of the tolerances to flip it (so that a device whose error estimate differs
from the oracle's in the last places must reproduce the oracle's decisions)."""
import os
import re

import numpy as np
import pytest

import cude_oracle as o
import adaptive_cases as ac

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conditional-ude_amd", "csrc")


def _macro(header, name):
    """The X(...) tuples of `#define name(X) ...` in csrc/<header>."""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^#define " + name + r"\(X\)(.*)$", f.read(), re.M)
    return [tuple(int(v) for v in t.split(",")) for t in re.findall(r"X\(([0-9, ]+)\)", m.group(1))]


def test_shape_lists_restate_the_headers():
    groups = [_macro("cude_shapes.h", f"CUDE_CPEP_SHAPES_{q}") for q in range(3)]
    assert [len(g) for g in groups] == [8, 8, 8]
    assert ac.CPEP_SHAPES == groups[0] + groups[1] + groups[2] and ac.TEAM_SHAPES == groups[0]
    assert ac.TWO_WORKGROUPS == [g[0] for g in groups]
    assert ac.SUPP_SHAPES == _macro("cude_shapes.h", "CUDE_SUPP_SHAPES")
    assert ac.SUPP_UNROLLED == _macro("cude_shapes.h", "CUDE_SUPP_AD_UNROLLED")
    assert set(ac.SUPP_UNROLLED) <= set(ac.SUPP_SHAPES)
    with open(os.path.join(CSRC, "cude_adaptive.h")) as f:
        assert re.search(r"kUnrolledKnots = (\d+);", f.read()).group(1) == "5"
    assert len(ac.TP5) == 5 and len(ac.TP6) == 6


def test_general_lists_restate_the_headers():
    """The lists tests/test_gpu_tangent_shapes.py walks for the other activation functions, and its 70-subject cases."""
    assert ac.CPEP_GENERAL_SHAPES == _macro("cude_shapes.h", "CUDE_CPEP_GENERAL_SHAPES")
    assert ac.SUPP_GENERAL_SHAPES == _macro("cude_shapes.h", "CUDE_SUPP_GENERAL_SHAPES")
    assert set(ac.CPEP_GENERAL_SHAPES) <= set(ac.CPEP_SHAPES) and set(ac.SUPP_GENERAL_SHAPES) <= set(ac.SUPP_SHAPES)
    with open(os.path.join(CSRC, "cude_shapes.h")) as f:
        pairs = re.search(r"^#define CUDE_GENERAL_ACTS\(Y\)(.*)$", f.read(), re.M).group(1)
    pairs = [tuple(int(v) for v in t.split(",")) for t in re.findall(r"Y\(([0-9, ]+)\)", pairs)]
    with open(os.path.join(CSRC, "cude_kernels.h")) as f:
        text = f.read()
    code = {name: int(v) for name, v in re.findall(r"kAct(Hidden\w+|Out\w+) = (\d+)", text)}
    hidden = {code["HiddenTanh"]: "tanh", code["HiddenRelu"]: "relu", code["HiddenSigmoid"]: "sigmoid"}
    output = {code["OutSoftplus"]: "softplus", code["OutIdentity"]: "identity"}
    assert ac.GENERAL_ACTS == [(hidden[h], output[q]) for h, q in pairs] and len(pairs) == 5
    assert ("tanh", "softplus") not in ac.GENERAL_ACTS               # the specialised default is not a general pair
    assert all(a[0] in o.HIDDEN_ACTS and a[1] in o.OUTPUT_ACTS for a in ac.GENERAL_ACTS)
    assert [ac.supp_subjects(s) for s in ac.SUPP_SHAPES] == [70 if s in [(3, 5), (4, 3), (3, 1)] else 12 for s in ac.SUPP_SHAPES]
    assert [ac.cpep_subjects(a) for a in ac.CPEP_SHAPES] == [70 if a in ac.TWO_WORKGROUPS else 16 for a in ac.CPEP_SHAPES]


@pytest.mark.parametrize("arch", [(2, 4, 2), (3, 6, 2), (2, 8, 3), (4, 3, 5), (4, 8, 1)])
def test_biased_params(arch):
    nn, plain = ac.biased_params(arch, 5), o.glorot_params(arch, 5)
    assert nn.size == o.n_params(arch)
    bias = np.zeros(nn.size, bool)
    bias[ac.bias_index(arch)] = True
    assert bias.sum() == arch[1] * arch[2] + 1 and np.all(plain[bias] == 0.0) and np.all(plain[~bias] != 0.0)
    assert np.all(nn[bias] != 0.0)
    scaled = np.zeros(nn.size, bool)
    if arch[0] == 3:
        scaled[2 * arch[1]:3 * arch[1]] = True
    assert np.array_equal(nn[~bias & ~scaled], plain[~bias & ~scaled]) and np.array_equal(nn[scaled], plain[scaled] / 50.0)
    # the blocks tile the parameter vector, and a bias is what cude_oracle.mlp reads as one: with all weights zero and
    # an identity output the network returns its output bias, whatever the inputs
    cover = np.concatenate([np.arange(s.start, s.stop) for _, s in ac.layer_blocks(arch)])
    assert np.array_equal(cover, np.arange(nn.size))
    only_bias = np.where(bias, nn, 0.0)
    assert o.mlp(np, [1.0] * arch[0], only_bias, tuple(arch) + ("tanh", "identity")) == only_bias[-1]


def _check(loss, g_nn, arch, solves):
    assert np.isfinite(loss)
    assert all(out is not None and 8 <= len(rec) <= 200 for out, rec, _ in solves(1.0))
    ratios = ac.block_ratios(g_nn, arch)
    print(f"{arch}: smallest block {min(ratios.values()):.2e} of the largest, "
          f"{min(len(rec) for _, rec, _ in solves(1.0))} ... {max(len(rec) for _, rec, _ in solves(1.0))} accepted steps")
    assert min(ratios.values()) >= 1e-3, ratios
    ref = [dec for _, _, dec in solves(1.0)]
    for scale in (1.0 + 1e-9, 1.0 - 1e-9):
        assert [dec for _, _, dec in solves(scale)] == ref, scale


@pytest.mark.parametrize("tp", [ac.TP5, ac.TP6], ids=["TP5", "TP6"])
@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=[str(a) for a in ac.CPEP_SHAPES])
def test_cpep_case(k, tp):
    arch = ac.CPEP_SHAPES[k]
    N = ac.cpep_subjects(arch)
    c = ac.cpep_case(arch, k, tp, N)
    pop = ac.cpep_population(c)
    assert np.all(c["nn"][ac.bias_index(arch)] != 0.0)
    loss, g_nn, g_b, _ = o.cpep_adaptive_loss_grad(c["nn"], c["beta"], pop, arch)
    assert np.all(g_b != 0.0)
    _check(loss, g_nn, arch, lambda scale: [ac.cpep_solve(c, pop, i, scale) for i in range(N)])


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=[str(s) for s in ac.SUPP_SHAPES])
def test_supp_case(k):
    s = ac.supp_case(ac.SUPP_SHAPES[k], k, 12)
    assert np.all(s["nn"][ac.bias_index(s["arch"])] != 0.0)
    # (without the penalty's share 2 lambda nn, which would lift every block)
    loss, g_nn, g_t, _ = o.supp_adaptive_loss_grad(s["nn"], s["theta"], s["data"], s["tp"], s["arch"], 0.0)
    assert np.all(g_t != 0.0)
    _check(loss, g_nn, s["arch"], lambda scale: [ac.supp_solve(s, i, scale) for i in range(12)])


def test_decision_record_is_the_solvers():
    """adaptive_cases._solve reconstructs the accept / reject sequence from the count of right-hand sides: check it on a
    solve with rejections against the accepted steps themselves (an accepted step starts where the one before ended, a
    rejected one where it started itself)."""
    c = ac.cpep_case((2, 6, 2), 1, ac.TP6, 16)
    pop = ac.cpep_population(c)
    n_rej = 0
    for i in range(16):
        out, rec, dec = ac.cpep_solve(c, pop, i)
        plain = []
        c0 = float(pop.c0[i])
        o.solve_adaptive(o.cpep_rhs_scalar(pop, i, c["nn"], float(np.exp(c["beta"][i])), c["arch"]),
                         [c0, float(pop.k2[i] / pop.k1[i]) * c0], pop.timepoints, record=plain)
        assert rec == plain and sum(dec) == len(rec) and dec[-1]
        n_rej += len(dec) - sum(dec)
    assert n_rej > 0
