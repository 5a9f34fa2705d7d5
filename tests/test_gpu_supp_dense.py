"""Dense output of the suppression model (cude_simulate on a suppression context; `simul` at save times other than the
data's own): the reference's figure script simulates its fitted model on range(0, 30, length = 100)
(suppression/figures.jl:66-74 through simul, suppression/src/suppression_model.jl:107-115: u0 from the data, the
problem's time span, saveat = the given times).  Checked against the oracle's fixed-step and adaptive solves at the same
output times, against cude_forward's trajectory at the data times (the same solve), on every kernel family the model can
land on (tuned fixed-step, adaptive unrolled, adaptive one-body, fallback network), through api.simul, and -- at the
data's own times, against cude_forward's trajectory -- for every network shape and activation pair the dense-output
kernels are compiled for."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (first: shared HIP runtime)

import adaptive_cases as ac
from conftest import make_supp_case

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden():
    g = np.load(os.path.join(GOLD, "suppression_lambda0.npz"))
    data = np.concatenate([g["group_data"], g["validation_data"]], axis=2)      # 37 training + 30 validation subjects
    theta = np.random.default_rng(11).standard_normal(data.shape[2]) * 0.5
    return g["timepoints"], data, g["nn_4x3x5x1"][0], theta


def _dense(tp):
    """0:0.1:30 with the data times in it, and where the data times sit"""
    grid = np.union1d(np.round(np.arange(0.0, 30.0 + 1e-9, 0.1), 10), tp)
    return grid, np.searchsorted(grid, tp)


def _oracle_chunked(fn, times, u0, k=28):
    """fn(timepoints, data) -> (3, T, N) of an oracle limited to 32 times per call: the output times in pieces, each
    between the span's end points (which fix the fixed-step grid and the adaptive span alike)"""
    N = u0.shape[1]
    out = np.empty((3, times.size, N))
    for a in range(0, times.size, k):
        tp = np.concatenate([[0.0], times[a:a + k], [30.0]])
        fake = np.ones((3, tp.size, N))
        fake[:, 0, :] = u0
        out[:, a:a + k] = fn(tp, fake)[:, 1:-1]
    return out


def _engine(arch, tp, data, nn, theta, n_steps, acts=()):
    from cude.engine import Engine
    eng = Engine("supp", arch, n_steps=n_steps)
    if acts:
        eng.set_option("hidden_activation", acts[0])
        eng.set_option("output_activation", acts[1])
    eng.set_population_supp(tp, data)
    eng.set_params(nn, theta)
    return eng


def test_fixed_step_tuned_kernel_matches_the_oracle():
    import c_oracle as co
    tp, data, nn, theta = _golden()
    arch = (4, 3, 5)
    eng = _engine(arch, tp, data, nn, theta, 30)
    dense, at = _dense(tp)
    got = eng.simulate(dense)
    assert got.shape == (3, dense.size, data.shape[2])
    ref = _oracle_chunked(lambda t, d: co.supp(t, d, arch, nn, theta, 0.0, 30, want_grad=False, want_traj=True)["traj"],
                          dense, data[:, 0, :])
    assert np.allclose(got, ref, rtol=1e-10, atol=1e-12), np.max(np.abs(got - ref))
    # the data times are columns of the same solve: cude_forward's trajectory bit for bit
    assert np.array_equal(got[:, at], eng.forward(want_traj=True)["traj"])
    # both device layouts and several launches give the same bits
    for layout in (0, 1):
        eng.set_option("dense_layout", layout)
        assert np.array_equal(eng.simulate(dense), got)
    eng.set_option("dense_chunk", 37)
    assert np.array_equal(eng.simulate(dense), got)
    with pytest.raises(Exception):
        eng.simulate([0.0, 31.0])                       # outside the span
    with pytest.raises(Exception):
        eng.simulate([10.0, 5.0])                       # decreasing
    eng.close()


@pytest.mark.parametrize("arch", [(4, 3, 5), (4, 4, 2)], ids=["unrolled-4-3x5-1", "one-body-4-4x2-1"])
def test_adaptive_matches_the_oracle_and_keeps_the_steps(arch):
    import c_oracle as co
    if arch == (4, 3, 5):
        tp, data, nn, theta = _golden()
    else:
        c = make_supp_case(70, arch)
        tp, data, nn, theta = c["tp"], c["data"], c["nn"], c["theta"]
    eng = _engine(arch, tp, data, nn, theta, 0)
    dense, at = _dense(tp)
    got = eng.simulate(dense)
    ref = _oracle_chunked(lambda t, d: co.supp_adaptive(t, d, arch, nn, theta), dense, data[:, 0, :])
    assert np.all(np.isfinite(ref))
    # saveat does not change the steps taken
    fwd = eng.forward(want_traj=True)["traj"]
    assert np.max(np.abs(got[:, at] - fwd)) <= 1e-12
    # against the oracle: 1e-7 relative (tests/test_gpu_adaptive.py) for every subject whose solve follows the oracle's
    # step sequence -- as cude_forward's does at the data times; a step accepted on one side and rejected on the other
    # (error estimate within rounding of 1) moves a whole trajectory, which DESIGN.md section 2 bounds by distribution
    ref_at = co.supp_adaptive(tp, data, arch, nn, theta)
    rel = np.empty(data.shape[2])
    for i in range(data.shape[2]):
        scale = max(1.0, np.max(np.abs(ref[:, :, i])))
        rel[i] = np.max(np.abs(got[:, :, i] - ref[:, :, i])) / scale
        if rel[i] > 1e-7:
            assert np.max(np.abs(fwd[:, :, i] - ref_at[:, :, i])) / scale > 1e-8, (i, rel[i])
    assert np.count_nonzero(rel > 1e-7) <= max(1, data.shape[2] // 10), rel
    assert np.median(rel) <= 2e-7 and np.max(rel) <= 1e-3
    eng.set_option("dense_chunk", 50)
    eng.set_option("dense_layout", 0)
    assert np.array_equal(eng.simulate(dense), got)
    eng.close()


def _data_times_against_forward(shape, n_steps, acts=()):
    """simulate() at the data's own times is cude_forward's solve: the same bits with a fixed step (the property
    test_fixed_step_tuned_kernel_matches_the_oracle holds 4-3x5-1 to), within 1e-12 in adaptive mode (the bar of
    test_adaptive_matches_the_oracle_and_keeps_the_steps: saveat does not change the steps taken).  12 subjects, the
    inputs of tests/test_gpu_adaptive_shapes.py (live biases; tests/test_adaptive_cases_host.py shows them adequate)."""
    s = ac.supp_case(shape, ac.SUPP_SHAPES.index(shape), 12)
    eng = _engine(s["arch"], s["tp"], s["data"], s["nn"], s["theta"], n_steps, acts)
    assert not eng.fallback_kernel
    got = eng.simulate(s["tp"])
    fwd = eng.forward(want_traj=True)["traj"]
    eng.close()
    assert got.shape == fwd.shape == (3, len(s["tp"]), 12) and np.all(np.isfinite(fwd))
    print(f"{s['arch']} {'-'.join(acts)} n_steps {n_steps}: max |simulate - forward| {np.max(np.abs(got - fwd)):.3e}")
    if n_steps:
        assert np.array_equal(got, fwd)
    else:
        assert np.max(np.abs(got - fwd)) <= 1e-12


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("shape", ac.SUPP_SHAPES, ids=str)
def test_every_compiled_shape_at_the_data_times(shape, n_steps):
    """launch_supp_dense and the dense-output leg of launch_supp_adaptive (unrolled and one-body), all 16 shapes"""
    _data_times_against_forward(shape, n_steps)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=["-".join(a) for a in ac.GENERAL_ACTS])
@pytest.mark.parametrize("shape", ac.SUPP_GENERAL_SHAPES, ids=str)
def test_every_compiled_activation_pair_at_the_data_times(shape, acts):
    _data_times_against_forward(shape, 30, acts)


@pytest.mark.parametrize("n_steps", [20, 0], ids=["fixed", "adaptive"])
def test_fallback_network(n_steps):
    import cude_oracle as o
    arch = (4, (5, 4), ("tanh", "relu"), "softplus")       # chain([5, 4], [tanh, relu]; input_dims = 4)
    N = 6
    c = make_supp_case(N, (4, 3, 5))
    nn = o.glorot_params(arch, 4)
    eng = _engine(arch, c["tp"], c["data"], nn, c["theta"], n_steps)
    assert eng.fallback_kernel
    times = np.round(np.arange(0.0, 30.0 + 1e-9, 0.25), 10)
    got = eng.simulate(times)
    if n_steps:
        fake = np.repeat(c["data"][:, :1, :], times.size, axis=1)
        sol = o.supp_forward(np, nn, c["theta"], fake, times, arch, n_steps)
        ref = np.stack([np.stack(sol[k]) for k in range(times.size)], axis=1)      # (3, T, N)
        assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref))
    else:
        for i in range(N):
            et = float(np.exp(c["theta"][i]))
            rhs = lambda t, u: [float(v) for v in o.supp_rhs(np, nn, et, arch, t, [np.float64(x) for x in u])]
            sol = np.array(o.solve_adaptive(rhs, list(c["data"][:, 0, i]), list(times)))      # (T, 3)
            assert np.max(np.abs(got[:, :, i].T - sol)) <= 1e-7 * max(1.0, np.max(np.abs(sol))), i
    eng.close()


@pytest.mark.parametrize("mode", ["adaptive", "fixed"])
def test_simul_at_the_figure_scripts_save_times(mode):
    """simul(ComponentArray(theta, neural), prob, test_data, range(0, 30, length = 100)) (figures.jl:66-74)"""
    from cude import api
    tp, data, nn, theta = _golden()
    prev = api.set_default_steps("fixed" if mode == "fixed" else api.ADAPTIVE)
    try:
        net = api.neural_network_model(5, 3, input_dims=4)
        prob = api.SuppressionProblem(net)
        assert prob.tspan == (0.0, 30.0)
        p = api.ComponentArray(theta=theta, neural=nn)
        sims = api.simul(p, prob, data, np.linspace(0.0, 30.0, 100))
        assert sims.shape == (3, 100, data.shape[2]) and np.all(np.isfinite(sims))
        dense, at = _dense(tp)
        got = api.simul(p, prob, data, dense)
        at_data = api.simul(p, prob, data, tp)             # one save time per data column: cude_forward's trajectory
        if mode == "fixed":
            assert np.array_equal(got[:, at], at_data)
        else:
            assert np.max(np.abs(got[:, at] - at_data)) <= 1e-12
        # a span of its own: the solve ends there, and save times beyond it are refused
        short = api.SuppressionProblem(net, (0.0, 20.0))
        sub = api.simul(p, short, data, np.linspace(0.0, 20.0, 41))
        assert sub.shape == (3, 41, data.shape[2])
        u0 = data[:, :1]
        eng = _engine((4, 3, 5), np.array([0.0, 20.0]), np.concatenate([u0, u0], axis=1), nn, theta,
                      api.DEFAULT_STEPS if mode == "fixed" else api.ADAPTIVE)
        assert np.array_equal(eng.simulate(np.linspace(0.0, 20.0, 41)), sub)
        eng.close()
        with pytest.raises(ValueError):
            api.simul(p, short, data, np.linspace(0.0, 30.0, 100))
        with pytest.raises(ValueError):
            api.simul(p, prob, data, np.array([0.0, 10.0, 5.0]))
    finally:
        api.set_default_steps(prev)
        api.clear_cache()


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_a_failing_subject_leaves_the_others_alone(n_steps):
    """Non-finite theta for one subject: its entries are NaN at every output time, every other subject's are those of
    the all-finite run (include/cude.h, cude_simulate)."""
    tp, data, nn, theta = _golden()
    dense, _ = _dense(tp)
    eng = _engine((4, 3, 5), tp, data, nn, theta, n_steps)
    ok = eng.simulate(dense)
    bad_theta = theta.copy()
    bad_theta[3] = np.nan
    eng.set_params(nn, bad_theta)
    got = eng.simulate(dense)
    others = np.arange(data.shape[2]) != 3
    assert np.array_equal(got[:, :, others], ok[:, :, others])
    assert np.all(np.isnan(got[:, :, 3]))
    eng.close()
