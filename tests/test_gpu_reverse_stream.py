"""The reverse sweep of the fixed-step c-peptide gradient kernel with the hidden layer held for the whole sweep
(csrc/cude_device.h Mlp::eval_grad_rw): the smallest cases in which a resident copy of the weights can go wrong --
inactive lanes and a partial last wave, both layer-1 forms in both sweeps, a run that leaves the exponent table
mid-sweep, two parameter sets in one launch, and parameters replaced between two launches.

Every case runs the one-lane kernel (`cpep_path` = 1; a population this small would otherwise be time-split) and is
compared with the C oracle at the tolerances of tests/test_gpu_parity.py: loss 1e-10, gradients 1e-9 of the
gradient's max-norm.  The grid is S = 30 steps over T = 5 observation times: steps inside a glucose piece (table form
of layer 1) and steps that straddle a knot (direct exponentials)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (imported first so PyTorch and libcude_hip share one HIP runtime)

from conftest import make_cpep_case

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-10
GRAD_RTOL = 1e-9
S = 30


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(N, arch):
    c = make_cpep_case(N, arch, n_steps=S)
    assert len(c["tp"]) == 5
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _oracle(N, arch, n_state):
    import c_oracle as co
    c = _case(N, arch)
    return co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, c["nn"], c["beta"], S, n_state)


def _engine(c, arch, n_state, monkeypatch):
    from cude.engine import Engine
    monkeypatch.setenv("CUDE_CPEP_PATH", "1")          # read when the context is created
    eng = Engine("cpep", arch, n_steps=S, n_state=n_state)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    return eng


def _check(got, ref, what):
    loss, g_nn, g_cond = got
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    e_nn, e_cond = _rel(g_nn, ref["g_nn"]), _rel(g_cond, ref["g_beta"])
    print(f"{what}: loss {e_loss:.3e} g_nn {e_nn:.3e} g_cond {e_cond:.3e}")
    assert e_loss <= LOSS_RTOL, what
    assert e_nn < GRAD_RTOL and e_cond < GRAD_RTOL, what


@pytest.mark.parametrize("n_state", [2, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_resident_layer_with_inactive_lanes_and_partial_waves(N, n_state, monkeypatch):
    arch = (2, 6, 2)
    c = _case(N, arch)
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_params(c["nn"], c["beta"])
    got = eng.loss_grad()
    assert eng.n_failed() == 0
    eng.close()
    _check(got, _oracle(N, arch, n_state), (N, n_state))


def test_run_that_fails_the_table_range_check_mid_sweep(monkeypatch):
    """One subject's glucose jumps by 4000 between the third and the fourth knot: with first-layer weights of order one
    its pre-activations leave +-300, the wave's range check fails for the runs from there on and those runs take the
    full exponentials, while the runs before the jump keep the table -- in the forward and in the reverse sweep."""
    import c_oracle as co
    arch, N = (2, 6, 2), 65
    c = dict(_case(N, arch))
    G = c["G"].copy()
    G[7, 3:] += 4000.0
    c["G"] = G
    assert np.max(np.abs(c["nn"][:6])) * 4000.0 > 300.0          # W1[:, 0]: the jump does leave the table's range
    for n_state in (2, 3):
        ref = co.cpep(c["tp"], G, c["obs"], c["age"], c["t2dm"], arch, c["nn"], c["beta"], S, n_state)
        eng = _engine(c, arch, n_state, monkeypatch)
        eng.set_params(c["nn"], c["beta"])
        got = eng.loss_grad()
        assert eng.n_failed() == 0
        eng.close()
        _check(got, ref, ("jump", n_state))


def test_two_parameter_sets_in_one_launch_keep_their_own_layers(monkeypatch):
    """Grid row y of a multi-set launch holds set y's hidden layer: each set's results equal its own single-set launch
    bit for bit (and the oracle's), with hidden layers that differ in every entry."""
    import c_oracle as co
    import cude_oracle as o
    arch, N, n_state = (2, 6, 2), 130, 3
    c = _case(N, arch)
    rng = np.random.default_rng(5)
    nn_sets = np.stack([c["nn"], o.glorot_params(arch, 99)])
    assert np.all(nn_sets[0, 18:54] != nn_sets[1, 18:54])        # the 6 x 6 layer
    cond_sets = np.stack([c["beta"], c["beta"] + 0.2 * rng.standard_normal(N)])
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_option("ms_split", 0)                                # the one-lane kernel with the sets in grid y
    eng.set_params(c["nn"], c["beta"])
    loss, g_nn, g_cond = eng.multistart_loss_grad(nn_sets, cond_sets)
    for k in (1, 0):
        eng.set_params(nn_sets[k], cond_sets[k])
        l1, gn1, gc1 = eng.loss_grad()
        assert l1 == loss[k] and np.array_equal(gn1, g_nn[k]) and np.array_equal(gc1, g_cond[k]), k
        ref = co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, nn_sets[k], cond_sets[k], S, n_state)
        _check((loss[k], g_nn[k], g_cond[k]), ref, ("set", k))
    eng.close()


@pytest.mark.parametrize("arch", [(2, 7, 2), (2, 4, 2), (2, 8, 2)])
def test_shapes_without_a_resident_layer(arch, monkeypatch):
    """Width 7 (exponent table, weights streamed), width 4 and width 8: the shapes around the one that changed."""
    N, n_state = 65, 3
    c = _case(N, arch)
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_params(c["nn"], c["beta"])
    got = eng.loss_grad()
    eng.close()
    _check(got, _oracle(N, arch, n_state), arch)


def test_nothing_resident_survives_a_launch(monkeypatch):
    """Two gradient calls with set_params between them: the second equals a fresh context's bit for bit, and the
    oracle's at the second parameters."""
    import c_oracle as co
    import cude_oracle as o
    arch, N, n_state = (2, 6, 2), 65, 3
    c = _case(N, arch)
    nn2 = o.glorot_params(arch, 4321)
    beta2 = c["beta"] - 0.25
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_params(c["nn"], c["beta"])
    first = eng.loss_grad()
    eng.set_params(nn2, beta2)
    second = eng.loss_grad()
    eng.close()
    fresh = _engine(c, arch, n_state, monkeypatch)
    fresh.set_params(nn2, beta2)
    alone = fresh.loss_grad()
    fresh.close()
    assert second[0] == alone[0] and np.array_equal(second[1], alone[1]) and np.array_equal(second[2], alone[2])
    assert first[0] != second[0]
    _check(first, _oracle(N, arch, n_state), "first")
    _check(second, co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, nn2, beta2, S, n_state), "second")
