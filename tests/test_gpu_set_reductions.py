"""Every geometry of the LDS sorting tile (csrc/cude_tilesort.h) through both reductions that sort with it:
bootstrap_reduce_kernel (cude_bootstrap_conditional, csrc/cude_bootstrap.hip) and predictive_select_kernel
(cude_predictive_bands, csrc/cude_predictive.hip).  A tile holds K values of C neighbouring columns as [Kp][C] doubles, Kp
= K rounded up to a power of two, C = min(64, 8192 / Kp) -- the full 64 KiB from K = 65 on.  tests/test_gpu_predictive.py
stops at K = 130 (C = 32) and tests/test_gpu_bootstrap.py at B = 40 (C = 64); both entry points accept K up to 4096.

GEOMETRY below is the table the tests walk; tests/test_tilesort_host.py holds it to the header's three constants and
holds the network's index arithmetic, restated in numpy, to np.sort at every K of it -- so a failure here with that file
passing points at the kernel around the network (launch attributes, barriers, the load and read-off loops).

Reached (every C through both entry points):
  bootstrap    cpep-2441, N = 67 (odd: the last tile is partial at every C; two fit workgroups, the second with three
               lanes), fixed step, the caller's noise: every K of the table; K = 1025 again under "bootstrap_subjects"
               = 64 and under "bootstrap_chunk" = 400; supp-4355, N = 5 at K = 4096 (the second model's reduce stride)
  rule 5       K = 257 (C = 16) and K = 5 (C = 64), N = 67: subjects with 0, 1, 2, K - 1 and K FAILED replicates (the
               branch ranks[r] < n_used with 0 < n_used < K, the walks over a column with +Inf holes), made from outside
               by non-finite entries of the caller's noise
  predictive   cpep-2441 and supp-4355, N = 5, 11 output times (55 columns, odd), fixed step: K = 257, 513, 1025, 2049,
               4096 (C = 16 ... 2; C = 64 and 32 are tests/test_gpu_predictive.py's); adaptive: cpep-2441 at K = 1025; at
               K = 1025 also "predictive_times" = 3, "profile_chunk" = 300 and a NaN sample
References: for the bootstrap bootstrap_ref.summaries of the device's OWN replicates and statuses with the bars of
tests/test_gpu_bootstrap.py (order and n_used exact, mean and sd to rtol 1e-13); for the bands predictive_ref.bands of the
device's own per-set solves, exact -- computed once per case for SOLVED = 4096 sets and sliced (0.8 s for the c-peptide
case, 1.2 s for the suppression case on the device machine: K = 4096 is checked through this entry point too)."""
import time

import numpy as np
import pytest

import bootstrap_ref as br
import predictive_ref as pr

pytestmark = pytest.mark.gpu

# K -> (Kp, C)
GEOMETRY = {1: (1, 64), 2: (2, 64), 3: (4, 64), 64: (64, 64), 65: (128, 64), 129: (256, 32), 257: (512, 16), 513: (1024, 8),
            1025: (2048, 4), 2049: (4096, 2), 4096: (4096, 2)}
K_MAX = 4096
N_BOOT = 67
FAILED = 4                                      # CUDE_REFINE_FAILED
MEAN_RTOL = 1e-13


def boot_ranks(K):
    """unique(0, 1, K // 2, K - 2, K - 1), filled up to 16 ranks from an even spread at K >= 16"""
    r = {0, min(1, K - 1), K // 2, max(K - 2, 0), K - 1}
    if K >= 16:
        for v in np.linspace(0, K - 1, 16).astype(int):
            if len(r) < 16:
                r.add(int(v))
    return np.array(sorted(r), dtype=np.int32)


_BOOT = {}


def boot_inputs():
    """(case data, centre, sigma, noise (4096, T, 67)) of the 2-4-4-1 population of tests/test_gpu_bootstrap.py at N = 67;
    a test takes the first K replicates of the noise."""
    if not _BOOT:
        import test_gpu_refine as tg
        c = tg._case_data("cpep-2441", N_BOOT)
        noise = np.random.default_rng(11).standard_normal((K_MAX, len(c["tp"]), N_BOOT))
        _BOOT["v"] = (c, np.linspace(-1.5, 0.5, N_BOOT), np.full(N_BOOT, 0.05), noise)
    return _BOOT["v"]


def _boot_engine(name="cpep-2441", N=N_BOOT, options=()):
    import test_gpu_refine as tg
    _, eng, _ = tg._make(name, N, 30)
    for k, v in options:
        eng.set_option(k, v)
    return eng


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _rel(got, want):
    """largest |got - want| / |want| over the entries that are numbers in both (NaN in the same places is asserted apart)"""
    ok = np.isfinite(want) & np.isfinite(got) & (want != 0)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def _own_summaries(tag, got, ranks):
    """Rule 5 restated on the device's own table: order and n_used exact, NaN in the same places, mean and sd to MEAN_RTOL."""
    own = br.summaries(got["replicates"], got["status"], ranks)
    print(f"{tag}: mean {_rel(got['mean'], own['mean']) / MEAN_RTOL:.2e}, sd {_rel(got['sd'], own['sd']) / MEAN_RTOL:.2e} of the bar "
          f"{MEAN_RTOL:.0e}; n_used {own['n_used'].min()}..{own['n_used'].max()}")
    assert np.array_equal(got["n_used"], own["n_used"])
    assert np.array_equal(got["order"], own["order"], equal_nan=True)
    for k in ("mean", "sd"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(own[k])), k
        assert np.allclose(got[k], own[k], rtol=MEAN_RTOL, atol=0, equal_nan=True), k
    return own


# ----------------------------------------------------------------------------- bootstrap: every geometry
@pytest.mark.parametrize("K", sorted(GEOMETRY))
def test_bootstrap_summaries_at_every_geometry(K):
    c, center, sigma, noise = boot_inputs()
    ranks = boot_ranks(K)
    assert ranks.size == (16 if K >= 16 else min(K, 5)) and ranks[-1] == K - 1
    eng = _boot_engine()
    got = eng.bootstrap_conditional(sigma, K, center, ranks=ranks, noise=noise[:K], upper=3.0, want_replicates=True)
    assert eng.n_failed() == 0
    eng.close()
    own = _own_summaries(f"bootstrap K={K} (Kp, C)={GEOMETRY[K]}", got, ranks)
    assert np.all(own["n_used"] == K) and np.isfinite(got["order"]).all()
    if K > 1:                                                # (the synthetic population has a few flat subjects)
        assert np.count_nonzero(got["sd"] > 0) >= 60
        assert np.all(got["order"][0] <= got["order"][-1]) and np.count_nonzero(got["order"][0] < got["order"][-1]) >= 60


def test_bootstrap_splits_at_four_columns():
    K = 1025
    c, center, sigma, noise = boot_inputs()
    out = []
    for options in ((), (("bootstrap_subjects", 64),), (("bootstrap_chunk", 400),)):       # 400 + 400 + 225 replicates
        eng = _boot_engine(options=options)
        out.append(eng.bootstrap_conditional(sigma, K, center, ranks=boot_ranks(K), noise=noise[:K], upper=3.0, want_replicates=True))
        assert eng.n_failed() == 0
        eng.close()
    _same(out[0], out[1])
    _same(out[0], out[2])


def test_bootstrap_full_tile_suppression():
    """K = 4096 on the suppression model: 24 residual rows per replicate, five subjects in three tiles of two."""
    import test_gpu_refine as tg
    K, N = K_MAX, 5
    c = tg._case_data("supp-4355", N)
    noise = np.random.default_rng(12).standard_normal((K, 3 * len(c["tp"]), N))
    eng = _boot_engine("supp-4355", N)
    ranks = boot_ranks(K)
    got = eng.bootstrap_conditional(0.05, K, c["theta"], ranks=ranks, noise=noise, lower=-6.0, upper=4.0, want_replicates=True)
    n_failed = eng.n_failed()
    eng.close()
    own = _own_summaries("bootstrap supp-4355 K=4096", got, ranks)
    assert n_failed == 0 and np.all(own["n_used"] == K) and np.all(got["sd"] > 0)


# ----------------------------------------------------------------------------- rule 5 with some replicates FAILED
def failure_plan(K, chunk):
    """[(replicate, subject, value)]: subject 3 fails its first replicate, subject 40 its last (by +Inf), subject 66 -- the last
    one, lane 2 of the second fit workgroup -- the two replicates on either side of the "bootstrap_chunk" boundary, subject
    10 all but replicate 1, subject 65 all of them.  Failures per subject: 1, 1, 2, K - 1, K; everybody else 0."""
    plan = [(0, 3, np.nan), (K - 1, 40, np.inf), (chunk - 1, 66, np.nan), (chunk, 66, np.nan)]
    plan += [(b, 10, np.nan) for b in range(K) if b != 1]
    plan += [(b, 65, np.nan) for b in range(K)]
    return plan


def poisoned(noise, plan, T):
    """the noise with every planned entry written into a row behind t_0: row 1 + (b + i) % (T - 1)"""
    z = noise.copy()
    for b, i, v in plan:
        z[b, 1 + (b + i) % (T - 1), i] = v
    return z


@pytest.mark.parametrize("K,chunk", [(257, 100), (5, 2)])
def test_partly_failed_subjects(K, chunk):
    c, center, sigma, noise = boot_inputs()
    T = len(c["tp"])
    ranks = boot_ranks(K)
    plan = failure_plan(K, chunk)
    want_failed = np.zeros((K, N_BOOT), dtype=bool)
    for b, i, _ in plan:
        want_failed[b, i] = True
    assert sorted(set(want_failed.sum(axis=0).tolist())) == sorted({0, 1, 2, K - 1, K})
    kw = dict(ranks=ranks, upper=3.0, want_replicates=True)
    eng = _boot_engine()
    clean = eng.bootstrap_conditional(sigma, K, center, noise=noise[:K], **kw)
    assert eng.n_failed() == 0
    # rule 3: entries of t_0 rows are ignored
    z0 = noise[:K].copy()
    for b, i, v in plan:
        z0[b, 0, i] = v
    _same(clean, eng.bootstrap_conditional(sigma, K, center, noise=z0, **kw))
    assert eng.n_failed() == 0
    eng.set_option("bootstrap_chunk", chunk)
    got = eng.bootstrap_conditional(sigma, K, center, noise=poisoned(noise[:K], plan, T), **kw)
    n_failed = eng.n_failed()
    eng.close()
    hit = got["status"] == FAILED
    print(f"K={K}: FAILED pairs {np.count_nonzero(hit)} (planned {np.count_nonzero(want_failed)}), subjects with one {n_failed}")
    assert np.array_equal(hit, want_failed)
    assert np.array_equal(got["replicates"][~hit], clean["replicates"][~hit]) and np.array_equal(got["status"][~hit], clean["status"][~hit])
    n_used = K - want_failed.sum(axis=0)
    assert np.array_equal(got["n_used"], n_used) and n_failed == np.count_nonzero(n_used < K) == 5
    _own_summaries(f"partly failed K={K}", got, ranks)
    assert np.array_equal(np.isnan(got["order"]), ranks[:, None] >= n_used[None, :])
    assert np.array_equal(np.isnan(got["sd"]), n_used < 2) and np.array_equal(np.isnan(got["mean"]), n_used < 1)
    # a subject without a failure keeps every summary
    ok = n_used == K
    for k in ("order", "mean", "sd"):
        assert np.array_equal(got[k][..., ok], clean[k][..., ok]), k


# ----------------------------------------------------------------------------- predictive bands
PRED_KS = (257, 513, 1025, 2049, 4096)
SOLVED = 4096                                   # sets solved one at a time per case (the reference's v)
_V = {}


def pred_inputs(name, n_steps, K_solved):
    """(engine, conditional parameters, times, sets (K_solved, 5), v (K_solved, n_state, 11, 5) = the device's own per-set
    solves), once per (case, mode); the engine stays open for the module."""
    import test_gpu_predictive as tp_
    key = (name, n_steps)
    if key not in _V:
        eng, cond, tp = tp_._make(name, n_steps, 5)
        times = tp_._times(tp)
        sets = tp_._samples(cond, K_solved)
        t0 = time.perf_counter()
        v = tp_._per_set(eng, cond, sets, times)
        print(f"{name} S={n_steps}: {K_solved} per-set solves in {time.perf_counter() - t0:.2f} s")
        _V[key] = (eng, cond, times, sets, v)
    return _V[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng, *_ in _V.values():
        eng.close()
    _V.clear()


def _bands_same(tag, got, want):
    import test_gpu_predictive as tp_
    tp_._same(tag, got, want)


@pytest.mark.parametrize("K", PRED_KS)
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_bands_at_every_geometry(name, K):
    import test_gpu_predictive as tp_
    eng, cond, times, sets, v = pred_inputs(name, 30, SOLVED)
    ranks = boot_ranks(K)
    for state in tp_.CASES[name][2]:
        got = eng.predictive_bands(sets[:K], times, ranks, state=state)
        _bands_same(f"{name} K={K} (Kp, C)={GEOMETRY[K]} state={state}", got, pr.bands(v[:K, state], ranks))
        assert eng.n_failed() == 0 and not got["bad_sets"].any() and np.isfinite(got["order"]).all()
        # (the initial state is every set's: minimum = maximum at t_0; at the last time the sets differ)
        assert np.all(got["order"][..., 0] <= got["order"][..., -1]) and np.all(got["order"][:, -1, 0] < got["order"][:, -1, -1])
    assert np.array_equal(eng.get_params()[1], cond)


def test_bands_adaptive_at_four_columns():
    import test_gpu_predictive as tp_
    K = 1025
    eng, cond, times, sets, v = pred_inputs("cpep-2441", 0, K)
    state = tp_.CASES["cpep-2441"][3][-1]
    got = eng.predictive_bands(sets, times, boot_ranks(K), state=state)
    _bands_same("cpep-2441 adaptive K=1025", got, pr.bands(v[:, state], boot_ranks(K)))
    assert eng.n_failed() == 0 and not got["bad_sets"].any()


@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_bands_splits_and_a_nan_sample_at_four_columns(name):
    """The C = 4 twin of tests/test_gpu_predictive.py::test_forced_splits_change_nothing and
    ::test_nan_sample_marks_its_subject_only (whose comment says why the c-peptide solves turn a NaN sample into finite
    values: rule 4 is a test on the values, and so is this one)."""
    import test_gpu_predictive as tp_
    K = 1025
    eng, cond, times, sets, v = pred_inputs(name, 30, SOLVED)
    state = tp_.CASES[name][2][-1]
    ranks = boot_ranks(K)
    whole = eng.predictive_bands(sets[:K], times, ranks, state=state)
    try:
        for opt, val in (("predictive_times", 3), ("profile_chunk", 300)):
            eng.set_option(opt, val)
            _bands_same(f"{name} {opt}={val}", eng.predictive_bands(sets[:K], times, ranks, state=state), whole)
            eng.set_option(opt, 0)
        bad = sets[:K].copy()
        bad[700, 3] = np.nan
        eng.set_params(None, bad[700])
        vb = v[:K, state].copy()
        vb[700] = eng.simulate(times)[state]
        eng.set_params(None, cond)
        assert np.array_equal(np.delete(vb[700], 3, axis=1), np.delete(v[700, state], 3, axis=1))
        nonfinite = ~np.isfinite(vb[700, :, 3])
        hit = int(nonfinite.any())
        assert hit == (0 if name.startswith("cpep") else 1)
        got = eng.predictive_bands(bad, times, ranks, state=state)
        _bands_same(name + " NaN", got, pr.bands(vb, ranks))
        assert np.array_equal(np.isnan(got["mean"][3]), nonfinite) and np.array_equal(np.isnan(got["order"][3]).all(axis=1), nonfinite)
        assert got["bad_sets"][3] == hit and got["bad_sets"].sum() == hit and eng.n_failed() == hit
        others = np.arange(5) != 3
        assert np.array_equal(got["order"][others], whole["order"][others]) and np.array_equal(got["mean"][others], whole["mean"][others])
    finally:
        eng.set_option("predictive_times", 0)
        eng.set_option("profile_chunk", 0)
