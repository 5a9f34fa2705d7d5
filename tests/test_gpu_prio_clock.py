"""Issue priority of co-resident waves keyed on the shader clock (option `prio_clock`, csrc/cude_cpep.hip).

Priority changes WHEN instructions issue, never what they compute: the fixed-step c-peptide gradient kernel must return
the same bytes whether its waves never alternate (`prio_shift` = 0), alternate by their own progress (`prio_shift` = 5,
`prio_clock` = 0) or by bit k of the shader clock (`prio_clock` = k: 17 is the scale of the headline launch, 10 flips a
few times per evaluation, 1 flips within every evaluation and exercises the path hardest).

Every case runs the one-lane kernel (`cpep_path` = 1; a population this small would otherwise be time-split) with
S = 30 steps over T = 5 observation times on N = 130 subjects: two full waves and one wave with two lanes.  The library's
own rule alternates only in launches that fill the chip, so the modes are set explicitly; an explicit `prio_shift` also
reaches the launches with several parameter sets in the grid's y dimension.  One comparison with the C oracle at the
tolerances of tests/test_gpu_parity.py: loss 1e-10, gradients 1e-9 of the gradient's max-norm."""
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
OFF = (0, 0)                                            # (prio_shift, prio_clock)
MODES = {"progress 5": (5, 0), "clock 1": (5, 1), "clock 10": (5, 10), "clock 17": (5, 17)}


@functools.lru_cache(maxsize=None)
def _case(arch):
    c = make_cpep_case(N, arch, n_steps=S)
    assert len(c["tp"]) == 5
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _sets(arch):
    import cude_oracle as o
    c = _case(arch)
    rng = np.random.default_rng(11)
    nn_sets = np.stack([c["nn"], o.glorot_params(arch, 77)])
    cond_sets = np.stack([c["beta"], c["beta"] + 0.2 * rng.standard_normal(N)])
    return nn_sets, cond_sets


def _engine(arch, n_state, monkeypatch):
    from cude.engine import Engine
    c = _case(arch)
    monkeypatch.setenv("CUDE_CPEP_PATH", "1")          # read when the context is created
    eng = Engine("cpep", arch, n_steps=S, n_state=n_state)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    return eng


def _mode(eng, mode):
    eng.set_option("prio_shift", mode[0])
    eng.set_option("prio_clock", mode[1])


def _same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_loss_grad_has_the_same_bits_in_every_mode(arch, n_state, monkeypatch):
    eng = _engine(arch, n_state, monkeypatch)
    _mode(eng, OFF)
    ref = eng.loss_grad()
    assert eng.n_failed() == 0
    assert np.isfinite(ref[0]) and np.any(ref[1] != 0.0) and np.any(ref[2] != 0.0)
    for name, mode in MODES.items():
        _mode(eng, mode)
        assert _same_bits(eng.loss_grad(), ref), name
    eng.close()


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_two_sets_per_launch_have_the_same_bits_in_every_mode(arch, n_state, monkeypatch):
    nn_sets, cond_sets = _sets(arch)
    eng = _engine(arch, n_state, monkeypatch)
    eng.set_option("ms_split", 0)                       # the one-lane kernel with the sets in grid y
    _mode(eng, OFF)
    ref = eng.multistart_loss_grad(nn_sets, cond_sets)
    assert np.all(np.isfinite(ref[0])) and ref[0][0] != ref[0][1]
    for name, mode in MODES.items():
        _mode(eng, mode)
        assert _same_bits(eng.multistart_loss_grad(nn_sets, cond_sets), ref), name
    # and the rows are the single-set launches of the same mode
    for k in (1, 0):
        eng.set_params(nn_sets[k], cond_sets[k])
        assert _same_bits(eng.loss_grad(), (ref[0][k], ref[1][k], ref[2][k])), k
    eng.close()


@pytest.mark.parametrize("arch,n_state", SHAPES)
def test_clock_keyed_result_against_the_oracle(arch, n_state, monkeypatch):
    import c_oracle as co
    c = _case(arch)
    ref = co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, c["nn"], c["beta"], S, n_state)
    eng = _engine(arch, n_state, monkeypatch)
    _mode(eng, MODES["clock 17"])
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
    _mode(eng, mode)
    eng.adam_init(1e-2)
    losses = eng.adam_run(4)
    nn, cond = eng.get_params()
    eng.close()
    return losses, nn, cond


@pytest.mark.parametrize("k", [1, 17])
def test_adam_run_under_clock_mode_equals_no_alternation(k, monkeypatch):
    arch, n_state = (2, 6, 2), 3
    ref = _adam(arch, n_state, OFF, monkeypatch)
    assert np.all(np.isfinite(ref[0])) and ref[0][0] != ref[0][3]
    assert _same_bits(_adam(arch, n_state, (5, k), monkeypatch), ref)
