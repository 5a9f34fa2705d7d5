"""The device's arithmetic below the parity bars: the activations of csrc/cude_math.h, the layer functions and one
network evaluation + reverse sweep of csrc/cude_device.h, run on the device by the test-only probe
(tests/hip/numerics_probe.hip, compiled with the product's flags) and compared with 50-digit references
(tests/numerics_ref.py); param_check at every parameter index, in the probe and end to end through the engine.

The parity tests (test_gpu_parity.py) compare whole solves at 1e-10 / 1e-9: an activation wrong by 1e-12 passes them.
The bars here are the host twin's measured maxima (elementwise), C u S (networks) and bit equality (the LDS table)."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported first so PyTorch and the probe share one HIP runtime)

import numerics_ref as nr
from test_gpu_parity import CPEP_SHAPES, SUPP_SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    nr.build(timeout=300)
    return nr.load_probe()


@pytest.fixture(scope="module")
def twin():
    nr.build(timeout=300)
    return nr.load_twin()


# ------------------------------------------------------------------------------------ elementwise primitives
@pytest.mark.parametrize("op", range(7), ids=nr.OP_NAMES)
def test_elementwise_against_50_digits_and_the_host_twin(probe, twin, op):
    x = nr.elementwise_inputs(op)
    y, s = nr.elementwise(probe.probe_elementwise, op, x)
    ev, es = nr.elementwise_errors(op, x, y, s)
    bar_v, bar_s = nr.ELEM_BARS[op]
    print(f"{nr.OP_NAMES[op]}: device max error {ev.max():.3g} (bar {bar_v:.3g})"
          + (f", logistic {es.max():.3g} (bar {bar_s:.3g})" if bar_s else ""))
    assert ev.max() <= bar_v, (x[np.argmax(ev)], y[np.argmax(ev)], ev.max())
    if bar_s is not None:
        assert es.max() <= bar_s, (x[np.argmax(es)], s[np.argmax(es)], es.max())
    # the same primitive compiled for the host: the device-only paths (v_rcp_f64 seed, v_fma_f64 with SGPR addends,
    # __double2loint table index, hipcc's FP contraction) may move a result by rounding only
    yt, st = nr.elementwise(twin.twin_elementwise, op, x)
    du = nr.ulp_distance(y, yt)
    assert du.max() <= nr.ULP_AGREE, (x[np.argmax(du)], y[np.argmax(du)], yt[np.argmax(du)])
    if bar_s is not None:
        ds = nr.ulp_distance(s, st)
        assert ds.max() <= nr.ULP_AGREE, (x[np.argmax(ds)], s[np.argmax(ds)], st[np.argmax(ds)])


def test_signed_zero_and_odd_symmetry(probe):
    x = np.array([0.0, -0.0, 1e-310, -1e-310, 0.3, -0.3, 7.0625, -7.0625, 30.0, -30.0])
    for op in (nr.TANH, nr.TANH_TAB):
        y, _ = nr.elementwise(probe.probe_elementwise, op, x)
        assert np.array_equal(np.signbit(y), np.signbit(x)), (nr.OP_NAMES[op], y)
        assert np.array_equal(y[0::2], -y[1::2]), nr.OP_NAMES[op]


def test_lds_tanh_table_is_correctly_rounded(probe):
    """cude_tanh_table.h claims tanh(k/8), correctly rounded: what tanh_tab_init leaves in LDS, bit for bit"""
    out = np.empty(161)
    assert probe.probe_tanh_table(nr.ptr(out), 161) == 0
    ref = nr.tanh_table_reference()
    bad = np.nonzero(out.view(np.int64) != ref.view(np.int64))[0]
    assert bad.size == 0, [(int(k), out[k], ref[k]) for k in bad[:5]]


# ------------------------------------------------------------------------------------ layer functions
@pytest.mark.parametrize("kind", range(5), ids=nr.LAYER_NAMES)
def test_layer_functions(probe, twin, kind):
    """act_hidden_vec<W, HA, TT> (tanh by table and by exponential, relu, logistic) and m_tanh_from_exp<W>, W = 1..8,
    with mixed and extreme units in one layer; act_hidden_deriv applied to the layer's own outputs, against the exact
    derivative (absolute)"""
    worst, worst_d = 0.0, 0.0
    for W in range(1, 9):
        z = nr.layer_inputs(kind, W)
        n = z.shape[0]
        h, dh = np.empty_like(z), np.empty_like(z)
        assert probe.probe_layer(kind, W, nr.ptr(z), nr.ptr(h), nr.ptr(dh), n) == 0
        href, dref = nr.layer_reference(kind, z)
        err = np.abs(h - href)
        derr = np.abs(dh - dref)
        assert err.max() <= nr.LAYER_BARS[kind], (W, z[np.unravel_index(np.argmax(err), z.shape)], err.max())
        assert derr.max() <= nr.DERIV_BAR, (W, z[np.unravel_index(np.argmax(derr), z.shape)], derr.max())
        if kind in (nr.L_TANH_EXP, nr.L_TANH_TAB):
            assert np.array_equal(np.signbit(h[z == 0]), np.signbit(z[z == 0])), W
        if kind in (nr.L_TANH_EXP, nr.L_TANH_TAB, nr.L_TANH_FROM_EXP):
            ht = np.empty_like(z)
            assert twin.twin_layer(kind, W, nr.ptr(z), nr.ptr(ht), n) == 0
            du = nr.ulp_distance(h, ht)
            assert du.max() <= nr.ULP_AGREE, (W, z[np.unravel_index(np.argmax(du), z.shape)])
        worst, worst_d = max(worst, err.max()), max(worst_d, derr.max())
    print(f"{nr.LAYER_NAMES[kind]}: device max error {worst:.3g} (bar {nr.LAYER_BARS[kind]:.3g}), derivative "
          f"{worst_d:.3g} (bar {nr.DERIV_BAR:.3g})")


# ------------------------------------------------------------------------------------ networks
GENERAL = [(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]      # (hidden, output) activation pairs compiled besides tanh/softplus
NETS = ([("cpep", 0, nin, w, d, 0, 0) for nin, w, d in CPEP_SHAPES] + [("supp", 1, 4, w, d, 0, 0) for w, d in SUPP_SHAPES]
        + [("cpepG", 2, 2, 4, 2, ha, oa) for ha, oa in GENERAL] + [("suppG", 3, 4, 3, 5, ha, oa) for ha, oa in GENERAL])


def _net_id(n):
    return f"{n[0]}-{n[2]}-{n[3]}x{n[4]}-a{n[5]}{n[6]}"


def _glorot(nin, W, D, seed):
    import cude_oracle as o
    return o.glorot_params((nin, W, D), seed)


def _net_inputs(model, nin, n, rng):
    """varying inputs x [n, NV] and per-subject constants cst [n, NC] (exp(conditional) [, age]) in the ranges the
    kernels see, the last quarter of the lanes extreme"""
    nv = 1 if model in ("cpep", "cpepG") else 3
    if nv == 1:
        x = rng.uniform(-4.0, 15.0, (n, 1))                  # glucose above baseline
    else:
        x = rng.uniform(0.0, 12.0, (n, 3))                   # suppression states
    cst = np.exp(rng.normal(-1.0, 1.0, (n, 1)))
    if nin - nv == 2:
        cst = np.concatenate([cst, rng.uniform(20.0, 79.0, (n, 1))], axis=1)      # age
    q = 3 * n // 4
    x[q:] = 10.0 ** rng.uniform(1.5, 4.0, x[q:].shape) * rng.choice([-1.0, 1.0], x[q:].shape)
    cst[q:, 0] = np.exp(rng.uniform(-8.0, 8.0, n - q))
    return x, cst


@pytest.mark.parametrize("net", NETS, ids=[_net_id(n) for n in NETS])
def test_network_value_and_vjp_against_50_digits(probe, net):
    """first_layer_offset, eval, eval_grad (weight 1, zeroed accumulators) and expand of the production network types
    against the same network at 50 digits, forward and reverse: |error| <= C u S per output, S the absolute-value
    propagation (cond. number x value).  Weights Glorot x1, x6, x40; widths 6-7 also through the exponent table."""
    model, fam, nin, W, D, ha, oa = net
    info = np.zeros(4, dtype=np.int32)
    assert probe.probe_net_info(fam, nin, W, D, ha, oa, nr.ptr(info)) == 0, "network not compiled in the probe"
    P, has_tab = int(info[0]), bool(info[1])
    nv = 1 if model in ("cpep", "cpepG") else 3
    rng = np.random.default_rng(1000 * nin + 100 * W + 10 * D + 3 * ha + oa + fam)
    worst = {}
    for scale, n in ((1.0, 48), (6.0, 24), (40.0, 24)):
        p = _glorot(nin, W, D, int(rng.integers(1 << 30))) * scale
        assert p.size == P
        x, cst = _net_inputs(model, nin, n, rng)
        refs = [nr.net_reference(nin, nv, W, D, ha, oa, p, x[i], cst[i]) for i in range(n)]
        for use_tab in ((0, 1) if has_tab else (0,)):
            ye, yg, g = np.empty(n), np.empty(n), np.empty((n, P))
            dc, dx = np.empty(n), np.empty((n, nv))
            rc = probe.probe_net(fam, nin, W, D, ha, oa, nr.ptr(p), nr.ptr(np.ascontiguousarray(x)),
                                 nr.ptr(np.ascontiguousarray(cst)), n, use_tab, nr.ptr(ye), nr.ptr(yg), nr.ptr(g),
                                 nr.ptr(dc), nr.ptr(dx))
            assert rc == 0
            for i, r in enumerate(refs):
                for name, got, ref, S in (("eval", ye[i], r["y"], r["Sy"]), ("eval_grad", yg[i], r["y"], r["Sy"]),
                                          ("grad", g[i], r["g"], r["Sg"]), ("dcond", dc[i], r["dcond"], r["Sdcond"]),
                                          ("dx", dx[i], r["dx"], r["Sdx"])):
                    ratio = np.max(np.abs(np.asarray(got) - ref) / (nr.U * np.maximum(S, 1e-300)))
                    worst[name] = max(worst.get(name, 0.0), float(ratio))
                    assert ratio <= nr.NET_C, (name, scale, use_tab, i, got, ref, S)
    print(f"{_net_id(net)}: max |error| / (u S): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("net", NETS, ids=[_net_id(n) for n in NETS])
def test_param_check_at_every_index(probe, net):
    """The clamped activations swallow NaN / Inf (tanh_tab(NaN) = +-1, softplus(NaN) ~ 1e-304): param_check is the only
    thing that turns a non-finite parameter into a failed solve.  NaN, +Inf and -Inf at every index -> NaN; finite
    -> 0 (the rolled groups of 8 and the tail)."""
    model, fam, nin, W, D, ha, oa = net
    info = np.zeros(4, dtype=np.int32)
    assert probe.probe_net_info(fam, nin, W, D, ha, oa, nr.ptr(info)) == 0
    P = int(info[0])
    base = _glorot(nin, W, D, 5) * 3.0
    sets = [base]
    for bad in (np.nan, np.inf, -np.inf):
        for q in range(P):
            s = base.copy()
            s[q] = bad
            sets.append(s)
    sets.append(np.full(P, 1.7e308))
    sets.append(np.full(P, -5e-324))
    p = np.ascontiguousarray(np.array(sets))
    out = np.empty(len(sets))
    assert probe.probe_param_check(fam, nin, W, D, ha, oa, nr.ptr(p), len(sets), nr.ptr(out)) == 0
    assert out[0] == 0.0 and out[-1] == 0.0 and out[-2] == 0.0
    miss = np.nonzero(~np.isnan(out[1:1 + 3 * P]))[0]
    assert miss.size == 0, [("nan", "+inf", "-inf")[k // P] + f"@{k % P}" for k in miss[:8]]


# ------------------------------------------------------------------------------------ end to end
def _cpep_engine(arch, c, family):
    from cude.engine import Engine
    eng = Engine("cpep", arch, n_steps=0 if family == "adaptive" else 6, n_state=2)
    if family == "fallback":
        eng.set_option("force_fallback", 1)
        eng.set_network([arch[1]] * arch[2], ["tanh"] * arch[2] + ["softplus"])
        assert eng.fallback_kernel
    elif family in ("one-lane", "time-split"):
        eng.set_option("cpep_path", "1" if family == "one-lane" else "2:3")
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    return eng


def _bad_sets(P, tail):
    """(index, value): NaN at every index, +-Inf at the tail entries (the output layer)"""
    return [(q, np.nan) for q in range(P)] + [(q, v) for q in range(P - tail, P) for v in (np.inf, -np.inf)]


@pytest.mark.parametrize("arch", [(2, 4, 2), (2, 6, 2)], ids=["2-4-4-1", "2-6-6-1"])
@pytest.mark.parametrize("family", ["one-lane", "time-split", "adaptive", "fallback"])
def test_engine_fails_every_subject_on_a_non_finite_parameter_cpep(arch, family):
    from conftest import make_cpep_case
    N = 20
    c = make_cpep_case(N, arch, n_steps=6)
    eng = _cpep_engine(arch, c, family)
    eng.set_params(c["nn"], c["beta"])
    assert np.isfinite(eng.forward()["loss"]) and eng.n_failed() == 0
    missed = []
    for q, v in _bad_sets(eng.P, arch[1] + 1):
        nn = c["nn"].copy()
        nn[q] = v
        eng.set_params(nn, c["beta"])
        loss = eng.forward()["loss"]
        if not (loss == np.inf and eng.n_failed() == N):
            missed.append((q, v, loss, eng.n_failed()))
    eng.set_params(c["nn"], c["beta"])
    assert np.isfinite(eng.forward()["loss"]) and eng.n_failed() == 0
    eng.close()
    assert not missed, missed[:8]


@pytest.mark.parametrize("family", ["fixed", "adaptive", "fallback"])
def test_engine_fails_every_subject_on_a_non_finite_parameter_supp(family):
    """4-3x5-1 (table tanh, LDS biases): loss +Inf, every subject failed, and simulate gives NaN at every output time
    (include/cude.h, cude_simulate)"""
    from conftest import make_supp_case
    from cude.engine import Engine
    arch, N = (4, 3, 5), 20
    c = make_supp_case(N, arch, n_steps=6)
    eng = Engine("supp", arch, n_steps=0 if family == "adaptive" else 6, lam=0.01)
    if family == "fallback":
        eng.set_option("force_fallback", 1)
        eng.set_network([3] * 5, ["tanh"] * 5 + ["softplus"])
        assert eng.fallback_kernel
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], c["theta"])
    times = np.linspace(0.0, 30.0, 7)
    assert np.isfinite(eng.forward()["loss"]) and np.isfinite(eng.simulate(times)).all()
    missed = []
    for q, v in _bad_sets(eng.P, 4):
        nn = c["nn"].copy()
        nn[q] = v
        eng.set_params(nn, c["theta"])
        loss = eng.forward()["loss"]
        nf = eng.n_failed()
        sim = eng.simulate(times)
        if not (loss == np.inf and nf == N and np.isnan(sim).all()):
            missed.append((q, v, loss, nf, int(np.isnan(sim).sum())))
    eng.close()
    assert not missed, missed[:8]
