"""Clamp-free sweeps of the fixed-step c-peptide gradient kernel (option `lean_clamp`, csrc/cude_cpep.hip).

Where a wave's parameter set proves that the tanh layers above the first see |z| <= 19.5 and the output unit |x| <= 690
(Mlp::lean_ok), the wave runs both sweeps without min(|z|, 20) and max(-0.5 |x|, -350).  Those clamps would have returned
their argument, so `lean_clamp` = -1 (the rule) must return the bytes of `lean_clamp` = 0 (every wave clamped) -- for
weights inside the bound, for weights outside it (the kernel's own test keeps those waves clamped: with row bounds of
60 behind saturated first-layer outputs the clamp acts, and with every row there a wave that went without it returns
NaN), for two parameter sets in one launch of which one is inside and one outside, and for a NaN weight, which fails the
test and the solve alike.

Every case runs the one-lane kernel (`cpep_path` = 1; a population this small would otherwise be time-split) with
S = 30 steps over T = 5 observation times on N = 130 subjects: two full waves and one wave with two lanes.  One comparison
with the C oracle at the tolerances of tests/test_gpu_prio_clock.py: loss 1e-10, gradients 1e-9 of the gradient's
max-norm."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (imported first so PyTorch and libcude_hip share one HIP runtime)

from conftest import make_cpep_case

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-10
GRAD_RTOL = 1e-9
S = 30
N = 130
SHAPES = [((2, 6, 2), 2), ((2, 6, 2), 3), ((2, 7, 2), 3)]
RULE, CLAMPED = -1, 0


@functools.lru_cache(maxsize=None)
def _case(arch):
    c = make_cpep_case(N, arch, n_steps=S)
    assert len(c["tp"]) == 5
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _l1(arch):
    nin, w, _ = arch
    return w * nin + w


def _row_bound(arch, nn, j):
    """|b_j| + sum_k |W_jk| of hidden layer 2 (weights column-major behind the first layer, then the biases)."""
    w, o = arch[1], _l1(arch)
    return abs(nn[o + w * w + j]) + sum(abs(nn[o + w * k + j]) for k in range(w))


def _out_bound(arch, nn):
    return float(np.sum(np.abs(nn[-(arch[1] + 1):])))


def _with_row_bound(arch, j, bound):
    """The case's Glorot weights with row j of hidden layer 2 scaled to the given bound."""
    c = _case(arch)
    w, o = arch[1], _l1(arch)
    nn = c["nn"].copy()
    f = bound / _row_bound(arch, nn, j)
    nn[o + w * w + j] *= f
    for k in range(w):
        nn[o + w * k + j] *= f
    assert abs(_row_bound(arch, nn, j) - bound) < 1e-9
    return nn


def _saturated_with_rows_at_60(arch, rows):
    """First-layer biases of +-30 by the sign of subject 0's baseline pre-activation (its first-layer outputs are then +-1
    to the last bit, inside the exponent table's range) and the given rows of layer 2 = 10 * the signs of those outputs:
    z_j = 60 there, three times the clamp's threshold.  One such row leaves the layer's shared reciprocal finite without
    the clamp; all of them overflow it (e^720), so a wave that wrongly went without would return NaN."""
    c = _case(arch)
    nin, w, _ = arch
    o = _l1(arch)
    nn = c["nn"].copy()
    x = np.array([0.0, np.exp(c["beta"][0])])
    z1 = sum(nn[w * i:w * i + w] * x[i] for i in range(nin)) + nn[w * nin:o]
    nn[w * nin:o] += 30.0 * np.sign(z1)
    for j in rows:
        for k in range(w):
            nn[o + w * k + j] = 10.0 * np.sign(z1[k])
        nn[o + w * w + j] = 0.0
        assert _row_bound(arch, nn, j) == 10.0 * w
    return nn


def _engine(arch, n_state, monkeypatch):
    from cude.engine import Engine
    c = _case(arch)
    monkeypatch.setenv("CUDE_CPEP_PATH", "1")          # read when the context is created
    eng = Engine("cpep", arch, n_steps=S, n_state=n_state)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    return eng


def _same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _both(eng, call):
    eng.set_option("lean_clamp", CLAMPED)
    ref = call()
    eng.set_option("lean_clamp", RULE)
    return call(), ref


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_glorot_weights_rule_equals_clamped(arch, n_state, monkeypatch):
    c = _case(arch)
    assert max(_row_bound(arch, c["nn"], j) for j in range(arch[1])) < 19.5 and _out_bound(arch, c["nn"]) < 690.0
    eng = _engine(arch, n_state, monkeypatch)
    got, ref = _both(eng, eng.loss_grad)
    assert eng.n_failed() == 0
    assert np.isfinite(ref[0]) and np.any(ref[1] != 0.0) and np.any(ref[2] != 0.0)
    assert _same_bits(got, ref)
    eng.close()


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_two_sets_per_launch_each_row_decides_for_itself(arch, n_state, monkeypatch):
    c = _case(arch)
    nn_sets = np.stack([c["nn"], _saturated_with_rows_at_60(arch, [1])])          # inside the bound, outside it
    cond_sets = np.stack([c["beta"], c["beta"] + 0.2 * np.random.default_rng(11).standard_normal(N)])
    eng = _engine(arch, n_state, monkeypatch)
    eng.set_option("ms_split", 0)                       # the one-lane kernel with the sets in grid y
    got, ref = _both(eng, lambda: eng.multistart_loss_grad(nn_sets, cond_sets))
    assert np.all(np.isfinite(ref[0])) and ref[0][0] != ref[0][1]
    assert _same_bits(got, ref)
    # and the rows are the single-set launches, under the rule and clamped
    for mode in (RULE, CLAMPED):
        eng.set_option("lean_clamp", mode)
        for k in (1, 0):
            eng.set_params(nn_sets[k], cond_sets[k])
            assert _same_bits(eng.loss_grad(), (ref[0][k], ref[1][k], ref[2][k])), (mode, k)
    eng.close()


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_a_layer_2_row_below_at_and_far_beyond_the_bound(arch, n_state, monkeypatch):
    c = _case(arch)
    eng = _engine(arch, n_state, monkeypatch)
    j = arch[1] - 1
    for name, nn in (("19.4", _with_row_bound(arch, j, 19.4)), ("19.6", _with_row_bound(arch, j, 19.6)),
                     ("60, saturated", _saturated_with_rows_at_60(arch, [j])),
                     ("every row at 60, saturated", _saturated_with_rows_at_60(arch, range(arch[1])))):
        eng.set_params(nn, c["beta"])
        got, ref = _both(eng, eng.loss_grad)
        assert eng.n_failed() == 0 and np.isfinite(ref[0]), name
        assert _same_bits(got, ref), name
    eng.close()


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_output_weights_past_the_bound(arch, n_state, monkeypatch):
    c = _case(arch)
    nn = c["nn"].copy()
    nn[-(arch[1] + 1):-1] *= 800.0 / _out_bound(arch, nn)
    assert _out_bound(arch, nn) > 690.0
    eng = _engine(arch, n_state, monkeypatch)
    eng.set_params(nn, c["beta"])
    got, ref = _both(eng, eng.loss_grad)
    assert np.isfinite(ref[0]) and np.any(ref[1] != 0.0)
    assert _same_bits(got, ref)
    eng.close()


@pytest.mark.parametrize("where", ["layer 2", "output", "layer 1"])
def test_a_nan_weight_fails_and_skips_the_update_as_clamped(where, monkeypatch):
    arch, n_state = (2, 6, 2), 3
    c = _case(arch)
    nn = c["nn"].copy()
    nn[{"layer 2": _l1(arch) + 8, "output": len(nn) - 3, "layer 1": 2}[where]] = np.nan
    seen = {}
    for mode in (CLAMPED, RULE):
        eng = _engine(arch, n_state, monkeypatch)
        eng.set_option("lean_clamp", mode)
        eng.set_params(nn, c["beta"])
        loss = eng.loss_grad()[0]
        failed = eng.n_failed()
        eng.adam_init(1e-2)
        step = eng.adam_step()
        seen[mode] = (loss, failed, step) + tuple(eng.get_params())
        eng.close()
    loss, failed, step, nn_after, cond_after = seen[CLAMPED]
    assert loss == np.inf and failed == N and step == np.inf
    assert nn_after.tobytes() == nn.tobytes() and cond_after.tobytes() == c["beta"].tobytes()      # update skipped
    assert seen[RULE][:3] == seen[CLAMPED][:3] and _same_bits(seen[RULE][3:], seen[CLAMPED][3:])


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_rule_result_against_the_oracle(arch, n_state, monkeypatch):
    import c_oracle as co
    c = _case(arch)
    ref = co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, c["nn"], c["beta"], S, n_state)
    eng = _engine(arch, n_state, monkeypatch)
    eng.set_option("lean_clamp", RULE)
    loss, g_nn, g_cond = eng.loss_grad()
    assert eng.n_failed() == 0
    eng.close()
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    e_nn, e_cond = _rel(g_nn, ref["g_nn"]), _rel(g_cond, ref["g_beta"])
    print(f"{arch} {n_state}: loss {e_loss:.3e} g_nn {e_nn:.3e} g_cond {e_cond:.3e}")
    assert e_loss <= LOSS_RTOL
    assert e_nn <= GRAD_RTOL and e_cond <= GRAD_RTOL


def _adam(arch, n_state, mode, monkeypatch):
    eng = _engine(arch, n_state, monkeypatch)
    eng.set_option("lean_clamp", mode)
    eng.adam_init(1e-2)
    losses = eng.adam_run(4)
    nn, cond = eng.get_params()
    eng.close()
    return losses, nn, cond


def test_adam_run_under_the_rule_equals_clamped(monkeypatch):
    arch, n_state = (2, 6, 2), 3
    ref = _adam(arch, n_state, CLAMPED, monkeypatch)
    assert np.all(np.isfinite(ref[0])) and ref[0][0] != ref[0][3]
    assert _same_bits(_adam(arch, n_state, RULE, monkeypatch), ref)
