"""The yardstick of tests/test_gpu_npde.py on the CPU: tests/npde_ref.py (cude_npde's rules restated in numpy) against
numpy's own statistics and statistics.NormalDist, the Philox counters of the two new block kinds against a direct
evaluation, the admission of every GPU case, and the calibration study that pins the seeds.

Recorded here (this file prints them; run with -s):
  * AS241 restated vs statistics.NormalDist().inv_cdf at the clip points 1 / (2 n), 1 - 1 / (2 n) of every n_used in [2,
    4096]: worst |difference| / max(1, |x|) = 0 (CPython's inv_cdf is the same algorithm; the bar of the GPU test is 1e-14).
  * Near-ties (margin < 16 R^2 eps cond(C) (1 + |w_obs|)) on the CPU oracle's solves: 0 of 350 pairs in each of the four K =
    65 cases (cond(C) up to 598, 300, 4.8, 5.0e3), 0 of 335 at every K of the N = 67 walk, 0 of 770 / 2170 at T = 12 / 32, 0
    of 350 in the status cases, 0 of 350 in the calibration study.  The smallest margin seen anywhere is 5.3e-7 (K = 4096);
    the threshold is below 1e-8 everywhere (cond(C) <= 9.6e3).
  * Calibration (70 subjects drawn from the model, 500 simulations, n = 350): pooled npde mean -0.0050 (bar 0.214), variance
    1.027 (bar |var - 1| <= 0.302); with prior_mean shifted by 2 prior_sd: mean -0.826."""
import math
import os
import re
from statistics import NormalDist

import numpy as np
import pytest

import npde_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- draws
def test_draw_counters_are_block_kinds_of_their_own():
    """The counters restated in npde_ref equal the words written out here, the blocks a direct Philox evaluation of them; the
    two kinds differ from each other, from every bootstrap block (rows below 96: bits 14 and 15 of the last word clear)
    and from every Metropolis block (last word below 2^31); the source states the layout."""
    from conftest import device_draw, philox4x32_10
    from test_bootstrap_host import bootstrap_draw
    src = open(os.path.join(ROOT, "conditional-ude_amd", "csrc", "cude_rng.h")).read()
    assert "kRngKindNpdeEta = kRngKindBootstrap | 0x8000u, kRngKindNpdeNoise = kRngKindBootstrap | 0x4000u" in src
    assert "c[3] = kind_row | ((uint32_t)((uint64_t)rep >> 32) << 16);" in src
    seed, subject, rep = 0x1234567890ABCDEF, (5 << 32) | 77, (3 << 32) | 9
    key = (seed & 0xFFFFFFFF, seed >> 32)
    assert nr.counter(subject, rep, nr.KIND_ETA) == [77, 5, 9, 0x80008000 | (3 << 16)]
    assert nr.counter(subject, rep, nr.KIND_NOISE | 30) == [77, 5, 9, 0x80004000 | (3 << 16) | 30]
    for ctr, z in (([77, 5, 9, 0x80038000], nr.eta_normal(seed, subject, rep)),
                   ([77, 5, 9, 0x8003401E], nr.noise_normal(seed, subject, rep, 30))):
        c = philox4x32_10(ctr, key)                          # the block's words, from the counter written out
        u1, u2 = nr._u01(c[0], c[1]), nr._u01(c[2], c[3])
        assert z == math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    # no bootstrap row (< 3 * 32) and no Metropolis step (< 2^62) reaches either kind
    assert all((0x80000000 | row) & 0xC000 == 0 for row in range(96))
    assert nr.KIND_ETA & 0xC000 == 0x8000 and nr.KIND_NOISE & 0xC000 == 0x4000 and (nr.KIND_NOISE | 30) & 0xC000 == 0x4000
    z = np.array([nr.eta_normal(12345, 7, b) for b in range(100)] +
                 [nr.noise_normal(12345, 7, b, r) for b in range(40) for r in range(5)])
    assert np.all(np.isfinite(z)) and abs(z.mean()) < 0.25 and 0.8 < z.std() < 1.2 and np.unique(z).size == z.size
    assert nr.eta_normal(12345, 7, 3) != nr.noise_normal(12345, 7, 3, 0) != bootstrap_draw(12345, 7, 3, 0)
    assert nr.eta_normal(12345, 7, 3) != device_draw(12345, 7, 3)[0]


# ----------------------------------------------------------------------------- AS241
def test_as241_against_normaldist_at_every_clip_point():
    nd, worst = NormalDist(), 0.0
    for n in range(2, 4097):
        for p in (1.0 / (2.0 * n), 1.0 - 1.0 / (2.0 * n)):
            x = nd.inv_cdf(p)
            worst = max(worst, abs(nr.as241(p) - x) / max(1.0, abs(x)))
    # the three branches: |q| <= 0.425, r <= 5, r > 5
    for p in (0.5, 0.3, 0.925, 0.0751, 1e-9, 1.0 - 1e-9, 1e-12, 1e-300):
        x = nd.inv_cdf(p)
        worst = max(worst, abs(nr.as241(p) - x) / max(1.0, abs(x)))
    print(f"AS241 restated vs NormalDist.inv_cdf: worst {worst:.3g}")
    assert worst <= 1e-15
    assert nr.as241(0.5) == 0.0 and abs(nr.as241(0.975) - 1.959963984540054) <= 1e-15
    assert nr.clipped(0, 10) == 0.05 and nr.clipped(10, 10) == 0.95 and nr.clipped(3, 10) == 0.3
    # the library's coefficients are these, digit for digit
    src = open(os.path.join(ROOT, "conditional-ude_amd", "csrc", "cude_npde.hip")).read()
    written = {float(tok) for tok in re.findall(r"\d\.\d{15,}e[+-]\d+", src)}
    for table in (nr._A, nr._B[1:], nr._C, nr._D[1:], nr._E, nr._F[1:]):
        assert all(v in written for v in table)


# ----------------------------------------------------------------------------- the restatement against numpy
def test_restatement_against_numpys_own_statistics():
    rng = np.random.default_rng(8)
    K, R, N = 200, 5, 9
    A = rng.standard_normal((N, R, R))
    y = np.einsum("nrs,ksn->krn", A, rng.standard_normal((K, R, N))) + rng.standard_normal((1, R, N))
    y_obs = y[0] + 0.3 * rng.standard_normal((R, N))
    y[3, 2, 4] = np.nan                                      # one simulation of subject 4 is left out
    y[7, 0, 4] = np.inf
    out = nr.reduce(y, y_obs, np.ones(N), want_aux=True)
    for i in range(N):
        yi = y[out["used"][:, i], :, i]
        n = yi.shape[0]
        assert out["n_used"][i] == n == (K - 2 if i == 4 else K)
        assert out["status"][i] == (nr.FAILED_SIMS if i == 4 else 0)
        assert np.allclose(out["pred_mean"][:, i], yi.mean(axis=0), rtol=1e-13, atol=1e-14)
        C = np.cov(yi.T)
        assert np.allclose(out["cov"][:, :, i][np.tril_indices(R)], C[np.tril_indices(R)], rtol=1e-11, atol=1e-13)
        assert np.allclose(out["pred_var"][:, i], np.diag(C), rtol=1e-12)
        w = np.linalg.solve(np.linalg.cholesky(C), (yi - yi.mean(axis=0)).T).T
        assert np.allclose(out["w"][out["used"][:, i], :, i], w, rtol=1e-9, atol=1e-11)
        w_obs = np.linalg.solve(np.linalg.cholesky(C), y_obs[:, i] - yi.mean(axis=0))
        assert np.array_equal(out["below"][:, i], np.sum(yi < y_obs[:, i], axis=0))
        assert np.array_equal(out["below_decorr"][:, i], np.sum(w < w_obs, axis=0))
        # the decorrelated simulations are white
        assert np.allclose(np.cov(w.T), np.eye(R), atol=1e-9)
    nd = NormalDist()
    want = [[nd.inv_cdf(nr.clipped(int(out["below_decorr"][r, i]), int(out["n_used"][i]))) for i in range(N)] for r in range(R)]
    assert np.allclose(out["npde"], want, rtol=1e-15, atol=1e-15)
    # status: a non-finite observation / sigma, too few simulations, a singular covariance
    y_obs2 = y_obs.copy()
    y_obs2[1, 0] = np.nan
    sg = np.ones(N)
    sg[1] = np.inf
    y2 = y.copy()
    y2[:, 4, 2] = 2.0 * y2[:, 1, 2]                          # row 4 of subject 2 is a multiple of row 1
    o2 = nr.reduce(y2, y_obs2, sg)
    assert o2["status"][0] == o2["status"][1] == nr.BAD_OBS and o2["status"][2] == nr.SINGULAR
    assert np.all(o2["n_used"][:2] == -1) and np.all(np.isnan(o2["pd"][:, :2])) and np.all(o2["below"][:, :2] == -1)
    assert np.all(o2["below_decorr"][:, 2] == -1) and np.all(np.isnan(o2["npde"][:, 2])) and np.all(np.isfinite(o2["pd"][:, 2]))
    for k in ("pred_mean", "pd", "npde", "below", "below_decorr", "n_used", "status"):
        assert np.array_equal(o2[k][..., 3:], out[k][..., 3:], equal_nan=True), k
    o3 = nr.reduce(y[:R], y_obs, np.ones(N))
    assert np.all(o3["status"] & nr.FEW) and np.all(o3["below_decorr"] == -1) and np.all(np.isfinite(o3["pd"]))
    o4 = nr.reduce(y[:R + 1], y_obs, np.ones(N))             # (subject 4 loses simulation 3: R used ones are too few)
    assert np.array_equal((o4["status"] & nr.FEW) != 0, np.arange(N) == 4)


# ----------------------------------------------------------------------------- admission of the GPU cases
def _admit(label, cs, K, cond=None, noise=None, sigma=None):
    if cond is None:
        cond, noise = nr.draws(cs, K)
    sigma = cs["sigma"] if sigma is None else sigma
    y = nr.observe(nr.solve_sets(cs, cond), sigma, cs["scale"], noise)
    out = nr.reduce(y, cs["y_obs"], sigma, want_aux=True)
    ties, cond_c = nr.near_ties(out)
    ok = np.isfinite(cond_c)
    margin = np.inf
    for i in np.flatnonzero(ok):
        margin = min(margin, np.min(np.abs(out["w"][out["used"][:, i], :, i] - out["w_obs"][None, :, i])))
    print(f"{label}: near-ties {np.count_nonzero(ties)} of {ties.size}, cond(C) up to {np.max(cond_c[ok], initial=0.0):.3g}, "
          f"smallest margin {margin:.3g}, status {np.bincount(out['status'], minlength=1)}")
    assert np.count_nonzero(ties) <= 0.01 * ties.size, label
    return out


@pytest.mark.parametrize("name", list(nr.CASES))
def test_gpu_cases_are_admitted(name):
    """At most 1 % of a case's (row, subject) pairs may be near-ties of the decorrelated ranks (the docstring above records
    the counts: none)."""
    out = _admit(name, nr.case(name), 65)
    assert np.all(out["status"] == 0)


def test_gpu_geometry_status_and_row_cases_are_admitted():
    cs = nr.case("cpep-2441", 67)
    for K in (2, 64, 65, 257, 1025, 4096):
        out = _admit(f"N=67 K={K}", cs, K)
        assert np.all(out["status"] == (nr.FEW if K <= cs["R"] else 0))
    for T in (12, 32):
        _admit(f"T={T}", nr.case("supp-4355", T=T), 65)
    _admit("supp K=12", nr.case("supp-4355"), 12)
    cs = nr.case("cpep-2441")
    cond, noise = nr.draws(cs, 12)
    sigma, same = cs["sigma"].copy(), cond.copy()
    sigma[5] = 0.0
    same[:, 5] = cond[0, 5]
    out = _admit("singular", cs, 12, same, noise, sigma)
    assert out["status"][5] == nr.SINGULAR and np.all(np.delete(out["status"], 5) == 0)


# ----------------------------------------------------------------------------- calibration
def test_calibration_holds_the_bars_and_a_shifted_prior_breaks_them():
    """Data drawn from the model itself: the pooled npde are standard normal up to sampling error -- |mean| <= 4 / sqrt(n),
    |var - 1| <= 4 sqrt(2 / n), n = N R = 350.  The same data judged with prior_mean shifted by 2 prior_sd are not."""
    cs, cond, noise, out = nr.calibration()
    n = out["npde"].size
    assert (cs["N"], cs["T"], nr.K_CAL, n) == (70, 6, 500, 350)
    mean, var = nr.pooled(out["npde"])
    ties, _ = nr.near_ties(out)
    print(f"calibration: pooled npde mean {mean:.4f} (bar {4 / np.sqrt(n):.3f}), variance {var:.4f} (bar {4 * np.sqrt(2 / n):.3f}); "
          f"near-ties {np.count_nonzero(ties)} of {ties.size}")
    assert np.all(out["status"] == 0) and np.count_nonzero(ties) <= 0.01 * ties.size
    assert abs(mean) <= 4 / np.sqrt(n) and abs(var - 1) <= 4 * np.sqrt(2 / n)
    # pd is uniform too: its mean 1/2 within 4 sd of a mean of n uniforms
    assert abs(out["pd"].mean() - 0.5) <= 4 * np.sqrt(1 / 12 / n)
    _, _, _, shifted = nr.calibration(2.0)
    mean_s, var_s = nr.pooled(shifted["npde"])
    print(f"   prior_mean + 2 prior_sd: mean {mean_s:.4f}, variance {var_s:.4f}")
    assert abs(mean_s) > 4 / np.sqrt(n)


# ----------------------------------------------------------------------------- the documents and mirrors
def test_header_mirrors_and_documents_name_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    for needle in ("int32_t cude_npde(", "int32_t cude_npde_draws(", "CUDE_NPDE_SINGULAR    1", "CUDE_NPDE_FEW         2",
                   "CUDE_NPDE_FAILED_SIMS 4", "CUDE_NPDE_BAD_OBS     8", '"npde_subjects"', "CUDE_NPDE_SUBJECTS", "AS241"):
        assert needle in hdr, needle
    from cude import api, engine
    assert (engine.NPDE_SINGULAR, engine.NPDE_FEW, engine.NPDE_FAILED_SIMS, engine.NPDE_BAD_OBS) == (1, 2, 4, 8)
    assert (nr.SINGULAR, nr.FEW, nr.FAILED_SIMS, nr.BAD_OBS) == (1, 2, 4, 8)
    import inspect
    py = {k: v.default for k, v in inspect.signature(api.npde).parameters.items() if v.default is not inspect.Parameter.empty}
    assert py == dict(n_sims=1000, seed=None, samples=None, noise=None, n_steps=None)
    py = {k: v.default for k, v in inspect.signature(api.suppression_npde).parameters.items()
          if v.default is not inspect.Parameter.empty}
    assert py == dict(state=2, n_sims=1000, seed=None, samples=None, noise=None, n_steps=None)
    jl = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    assert "function npde(p_neural, models, timepoints, cpeptide_data, sigma, prior_η, prior_Ω; n_sims = 1000, seed = nothing," in jl
    assert "prior_Ω; state = 3, n_sims = 1000," in jl                # (1-based: the Python mirror's state = 2)
    for doc, needle in (("README.md", "cude_npde"), ("DESIGN.md", "7l"), ("INTEGRATION.md", "npde_subjects")):
        assert needle in open(os.path.join(ROOT, doc)).read(), (doc, needle)
