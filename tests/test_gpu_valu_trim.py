"""The three places where the fixed-step c-peptide gradient kernel stopped issuing vector instructions the result does
not need, each where it could go wrong:

 * the clamp of m_tanh_from_exp sits behind the add (csrc/cude_math.h): a run on the layer-1 exponent table whose
   exponentials EXCEED the cap e^40 (pre-activations between 20 and 300: the range check passes, the clamp works);
 * the reverse sweep branches on the wave-uniform stage instead of selecting per lane (csrc/cude_cpep.hip): oracle
   parity for the shapes with a factor table, widths 6 and 7, two and three states;
 * the final reduction reads doubled rows at constant offsets (csrc/cude_device.h block_reduce_expand_wide): a second
   wave with one active lane, repeated calls, two parameter sets in one launch, and the failure count, which is reduced
   in the 5-column last chunk.

Every case runs the one-lane kernel (`cpep_path` = 1; a population this small would otherwise be time-split), S = 30
steps over T = 5 observation times, and is compared with the C oracle at the tolerances of tests/test_gpu_parity.py:
loss 1e-10, gradients 1e-9 of the gradient's max-norm."""
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


def _same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- (a) oracle parity
@pytest.mark.parametrize("n_state", [2, 3])
@pytest.mark.parametrize("N", [1, 64, 65])
@pytest.mark.parametrize("arch", [(2, 6, 2), (2, 7, 2)])
def test_oracle_parity_of_the_shapes_with_a_factor_table(arch, N, n_state, monkeypatch):
    c = _case(N, arch)
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_params(c["nn"], c["beta"])
    got = eng.loss_grad()
    assert eng.n_failed() == 0
    eng.close()
    _check(got, _oracle(N, arch, n_state), (arch, N, n_state))


# ---- (b) the clamp at work on the table path
@pytest.mark.parametrize("arch", [(2, 6, 2), (2, 7, 2)])
def test_exponentials_beyond_the_cap_on_the_table_path(arch, monkeypatch):
    """One subject's glucose excursion is scaled by 20.  Its layer-1 pre-activations z_j = W1[j,0] dG + c_j then pass 20
    in the pieces behind the first knot -- exp(2 z) > e^40, the clamp is what keeps the product of the denominators
    finite -- but stay inside +-300 with steps of less than 300, so the wave's range check passes and those runs take
    the table (tab_safe: |z| at both ends of the piece and |W1 d| at most 300)."""
    import c_oracle as co
    W, N, who = arch[1], 65, 7
    c = dict(_case(N, arch))
    G = c["G"].copy()
    G[who] = G[who, 0] + 20.0 * (G[who] - G[who, 0])
    c["G"] = G
    w0, w1, b1 = c["nn"][:W], c["nn"][W:2 * W], c["nn"][2 * W:3 * W]
    x = G - G[:, :1]                                                            # [subject][knot]: the network's input
    z = w0[None, None, :] * x[:, :, None] + (b1 + w1 * np.exp(c["beta"])[:, None])[:, None, :]
    step = np.abs(w0[None, None, :] * np.diff(x, axis=1)[:, :, None])
    assert np.max(np.abs(z)) < 300.0 and np.max(step) < 300.0                   # every lane passes the range check
    both_ends = np.minimum(z[who, 1:-1], z[who, 2:])                            # pieces 1, 2, 3 of the scaled subject
    assert np.all(both_ends.max(axis=1) > 20.0), both_ends.max(axis=1)          # a unit beyond the cap all along each
    assert np.max(z[np.arange(N) != who]) < 20.0                                # and nobody else near it
    for n_state in (2, 3):
        ref = co.cpep(c["tp"], G, c["obs"], c["age"], c["t2dm"], arch, c["nn"], c["beta"], S, n_state)
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["g_nn"]).all() and np.isfinite(ref["g_beta"]).all()
        eng = _engine(c, arch, n_state, monkeypatch)
        eng.set_params(c["nn"], c["beta"])
        got = eng.loss_grad()
        assert eng.n_failed() == 0
        eng.close()
        _check(got, ref, ("cap", arch, n_state))


# ---- (c) the final reduction
@pytest.mark.parametrize("N", [65, 130])
def test_reduction_repeats_and_keeps_sets_apart(N, monkeypatch):
    """Two calls give the same bits (the doubled rows are rewritten per chunk, nothing of an earlier chunk or launch is
    summed); the rows of a two-set launch equal the single-set launches bit for bit, and the oracle."""
    import c_oracle as co
    import cude_oracle as o
    arch, n_state = (2, 6, 2), 3
    c = _case(N, arch)
    rng = np.random.default_rng(11)
    nn_sets = np.stack([c["nn"], o.glorot_params(arch, 77)])
    cond_sets = np.stack([c["beta"], c["beta"] + 0.2 * rng.standard_normal(N)])
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_option("ms_split", 0)                                # the one-lane kernel with the sets in grid y
    eng.set_params(c["nn"], c["beta"])
    first = eng.loss_grad()
    again = eng.loss_grad()
    assert _same_bits(first, again)
    _check(first, _oracle(N, arch, n_state), ("single", N))
    loss, g_nn, g_cond = eng.multistart_loss_grad(nn_sets, cond_sets)
    for k in (1, 0):
        eng.set_params(nn_sets[k], cond_sets[k])
        assert _same_bits(eng.loss_grad(), (loss[k], g_nn[k], g_cond[k])), k
        ref = co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, nn_sets[k], cond_sets[k], S, n_state)
        _check((loss[k], g_nn[k], g_cond[k]), ref, ("set", k, N))
    eng.close()


@pytest.mark.parametrize("N,who", [(65, 64), (130, 3)])
def test_failure_count_comes_through_the_last_chunk(N, who, monkeypatch):
    """Loss and failure count are columns P and P + 1 of the reduction: the last chunk, 5 of 16 rows in use.  One subject
    with a NaN conditional parameter -- the only active lane of the second wave, or a lane of the first of three -- is
    counted once."""
    arch, n_state = (2, 6, 2), 3
    c = _case(N, arch)
    beta = c["beta"].copy()
    beta[who] = np.nan
    eng = _engine(c, arch, n_state, monkeypatch)
    eng.set_params(c["nn"], beta)
    loss, g_nn, g_cond = eng.loss_grad()
    assert eng.n_failed() == 1
    assert np.isinf(loss) and loss > 0
    eng.set_params(c["nn"], c["beta"])
    good = eng.loss_grad()
    assert eng.n_failed() == 0
    eng.close()
    _check(good, _oracle(N, arch, n_state), ("after a failure", N))
