"""cude_sensitivity without a GPU: the reference helper checks itself (so that a broken helper cannot hide a broken
kernel), the ABI surface, the interval arithmetic of the mirrors, and the cross-compilation of the new translation unit.

Bounds of the self-checks: complex step and reverse-mode autograd evaluate the same fp64 arithmetic in different orders; the
two agreed to 6e-15 of max|S| and the gradient identity to 2e-14 when the checks were written, and 1e-12 leaves two
orders of magnitude for another BLAS / torch build while staying three below the 1e-9 the kernels are held to."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

from conftest import make_cpep_case, make_supp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF_TOL = 1e-12


def _pop(c):
    import cude_oracle as o
    return o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(c["arch"][0] == 3))


@pytest.mark.parametrize("arch,n_state", [((2, 6, 2), 2), ((2, 6, 2), 3), ((2, 4, 2), 2), ((3, 6, 2), 2)])
def test_complex_step_agrees_with_autograd_cpep(arch, n_state):
    import cude_oracle as o
    import sensitivity_ref as ref
    c = make_cpep_case(9, arch)
    pop = _pop(c)
    sens, info, score, sse = ref.cpep_sens(c["nn"], c["beta"], pop, arch, 30, n_state)
    st = ref.cpep_sens_torch(c["nn"], c["beta"], pop, arch, 30, n_state)
    assert sens.shape == (n_state, pop.T, 9) and np.all(sens[:, 0] == 0.0)
    assert np.max(np.abs(sens - st)) <= SELF_TOL * np.max(np.abs(sens))
    # g_cond = 2 score / N, and the SSE, against the oracle's reverse-mode gradient
    _, _, g_b, osse = o.cpep_loss_grad_torch(c["nn"], c["beta"], pop, arch, 30, n_state)
    assert np.max(np.abs(2.0 * score / 9 - g_b)) <= SELF_TOL * np.max(np.abs(g_b))
    assert np.max(np.abs(sse - osse)) <= SELF_TOL * np.max(osse)
    assert np.all(info >= 0.0) and np.count_nonzero(info) >= 8


def test_complex_step_agrees_with_autograd_supp():
    import cude_oracle as o
    import sensitivity_ref as ref
    c = make_supp_case(7)
    sens, info, score, sse = ref.supp_sens(c["nn"], c["theta"], c["data"], c["tp"], c["arch"], 30)
    st = ref.supp_sens_torch(c["nn"], c["theta"], c["data"], c["tp"], c["arch"], 30)
    assert np.all(sens[0] == 0.0) and np.all(sens[:, 0] == 0.0)        # state 1 depends on no parameter
    assert np.max(np.abs(sens - st)) <= SELF_TOL * np.max(np.abs(sens))
    _, _, g_t, osse = o.supp_loss_grad_torch(c["nn"], c["theta"], c["data"], c["tp"], c["arch"], 30, 0.0)
    assert np.max(np.abs(2.0 * score / 7 - g_t)) <= SELF_TOL * np.max(np.abs(g_t))
    assert np.max(np.abs(sse - osse)) <= SELF_TOL * np.max(osse)


def test_replay_of_the_fixed_grid_is_the_fixed_step_reference():
    """The adaptive helper (replay of given steps) on the uniform step sequence agrees with the fixed-step helper where the
    two interpolate alike: at observation times that are step ends."""
    import sensitivity_ref as ref
    c = make_cpep_case(5, (2, 4, 2), n_steps=32)
    pop = _pop(c)
    h = (c["tp"][-1] - c["tp"][0]) / 32
    steps = [[(c["tp"][0] + n * h, h) for n in range(32)]] * 5
    a = ref.cpep_sens(c["nn"], c["beta"], pop, (2, 4, 2), 32)
    b = ref.cpep_sens_replay(c["nn"], c["beta"], pop, (2, 4, 2), steps)
    assert np.max(np.abs(a[0] - b[0])) <= 1e-10 * np.max(np.abs(a[0]))
    s = make_supp_case(4)
    hs = 30.0 / 35
    a = ref.supp_sens(s["nn"], s["theta"], s["data"], s["tp"], s["arch"], 35)        # 8 times on a 35-step grid: step ends
    b = ref.supp_sens_replay(s["nn"], s["theta"], s["data"], s["tp"], s["arch"], [[(n * hs, hs) for n in range(35)]] * 4)
    assert np.max(np.abs(a[0] - b[0])) <= 1e-10 * np.max(np.abs(a[0]))


# ----------------------------------------------------------------------------- ABI
def test_symbol_is_declared_and_exported():
    from cude import _lib
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    assert "int32_t cude_sensitivity(cude_ctx* ctx, double* sens, double* info, double* score, double* sse);" in hdr
    assert "g_cond_i = 2 * score_i / n_global" in hdr and "parameter-estimation.jl:59" in hdr
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cude_sensitivity")
    assert "cude_sensitivity" in _lib.exported_symbols()


def test_bad_arguments_return_a_status():
    from cude import _lib
    lib = _lib.load()
    assert lib.cude_sensitivity(None, None, None, None, None) == -1          # CUDE_ERR_ARG, no abort
    assert b"null context" in lib.cude_last_error()
    with pytest.raises(_lib.CudeError):
        _lib.check(lib.cude_sensitivity(None, None, None, None, None))


# ----------------------------------------------------------------------------- interval arithmetic of the mirror
def test_standard_errors_and_wald_intervals(monkeypatch):
    from cude import api
    info = np.array([4.0, 0.0, 25.0, 1e-300])
    sse = np.array([8.0, 2.0, 0.5, 2.0])
    calls = []

    def fake(theta, args, *, n_steps=None):
        calls.append((theta, args, n_steps))
        return None, info, info * 0.0, sse
    monkeypatch.setattr(api, "sensitivities", fake)
    betas, tp = np.array([-2.0, -1.0, 0.5, 0.0]), [0.0, 30.0, 60.0, 120.0]          # n_i = 4 observations
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                              # info == 0: inf, silently
        se = api.conditional_standard_errors(betas, [0.1], ["m"] * 4, tp, "data")
        se1 = api.conditional_standard_errors(betas, [0.1], ["m"] * 4, tp, "data", sigma=0.5)
        ci = api.wald_confidence_intervals(betas, [0.1], ["m"] * 4, tp, "data", sigma=0.5)
        ci90 = api.wald_confidence_intervals(betas, [0.1], ["m"] * 4, tp, "data", level=0.9)
    # sigma = None: sigma_i^2 = SSE_i / n_i
    assert se[0] == np.sqrt(8.0 / 4) / 2.0 and se[1] == np.inf and se[2] == np.sqrt(0.5 / 4) / 5.0
    assert np.isfinite(se[3]) and se[3] > 1e100
    assert se1[0] == 0.25 and se1[1] == np.inf and se1[2] == 0.1
    z = 1.959963984540054                                                           # quantile(Normal(), 0.975)
    assert len(ci) == 4 and all(isinstance(p, tuple) and len(p) == 2 for p in ci)
    assert abs(ci[0][0] - (-2.0 - z * 0.25)) < 1e-12 and abs(ci[0][1] - (-2.0 + z * 0.25)) < 1e-12
    assert ci[1] == (-np.inf, np.inf)
    assert abs(ci[2][1] - ci[2][0] - 2 * z * 0.1) < 1e-12
    z90 = 1.6448536269514722
    assert abs((ci90[0][1] - ci90[0][0]) - 2 * z90 * se[0]) < 1e-12
    # what reaches the library: theta = (neural, conditional), args = (models, timepoints, data)
    theta, args, _ = calls[0]
    assert np.all(theta.conditional == betas) and list(theta.neural) == [0.1] and args[1] is tp
    # a failed subject stays NaN
    assert np.isnan(api._standard_errors(np.array([np.nan, 1.0]), np.array([np.nan, 1.0]), 4, None)[0])


def test_julia_quantile_coefficients_give_the_normal_quantile():
    """julia/CUDEHip.jl carries Acklam's rational approximation (no Distributions dependency); restated here from the
    Julia text and held against the exact quantile the Python mirror uses."""
    import re
    from statistics import NormalDist
    src = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    body = src[src.index("function normal_quantile(p)"):]
    tup = {k: [float(v) for v in re.findall(r"[-+]?\d\.\d+e[-+]\d+", body[body.index(f"{k} = ("):body.index(")", body.index(f"{k} = ("))])]
           for k in ("a", "b", "cc", "d")}
    assert [len(tup[k]) for k in ("a", "b", "cc", "d")] == [6, 5, 6, 4]
    a, b = tup["a"], tup["b"]
    for p in (0.5, 0.9, 0.95, 0.975):
        q = p - 0.5
        r = q * q
        x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
            (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1)
        assert abs(x - NormalDist().inv_cdf(p)) <= 2e-9 * max(1.0, abs(x))


# ----------------------------------------------------------------------------- the new translation unit
def test_cude_sens_cross_compiles_for_gfx950(tmp_path):
    csrc = os.path.join(ROOT, "conditional-ude_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the library cannot be built here either")
    procs = [subprocess.Popen([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
                               f"-DCUDE_SENS_PART={k}", "-c", os.path.join(csrc, "cude_sens.hip"), "-o",
                               str(tmp_path / f"sens_p{k}.o")], stderr=subprocess.PIPE) for k in range(4)]
    for k, p in enumerate(procs):
        _, err = p.communicate()
        assert p.returncode == 0, f"part {k}: {err.decode()[-2000:]}"
        assert os.path.getsize(tmp_path / f"sens_p{k}.o") > 10000
