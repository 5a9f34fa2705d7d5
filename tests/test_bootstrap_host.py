"""cude_bootstrap_conditional without a GPU: the admissibility of the cases tests/test_gpu_bootstrap.py holds the device to,
the numpy restatement's summaries (tests/bootstrap_ref.py) against numpy's own statistics, the mirror's percentile interval
against numpy.quantile, the draws' counter layout, the ABI surface and the cross-compilation of the new translation unit;
and, on the restatement alone, the conditions tests/test_gpu_bootstrap_shapes.py and tests/test_gpu_set_reductions.py put on
their cases (the replicates move their subjects; non-finite noise fails exactly its replicate).

Admissibility.  A (replicate, subject) pair is UNSTABLE when the restatement's status or `evals` change under f_info,
f_score = 1 +- 1e-9, together and in opposite directions -- the error the tangent kernels are allowed, the study of
tests/test_refine_host.py.  For an unstable pair the device is held to the |dx| bar and a valid status only.  At most 2 % of
a case's pairs may be unstable: a condition on the case, not a tolerance -- a case over it is replaced, the cap stays.

Measured here (bootstrap_ref.case: centre = the restatement's fit from the case's constant start, sigma = sqrt(SSE / rows),
B = 8, np.random.default_rng(5)); `worst` = largest |dx| / (1 + |x|) between a perturbed run and the base run:

    cpep-2441   0 of 192 unstable                worst 5.3e-12
    supp-4355   1 of 128 unstable (0.8 %)        worst 1.3e-07   (the unstable pair; the x bar of the GPU tests is 1e-6)
    cpep-3441   3 of 192 unstable (1.6 %)        worst 3.3e-11
    sym-raw     0 of 192 unstable                worst 2.3e-12
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADMITTED = ("cpep-2441", "supp-4355", "cpep-3441", "sym-raw")
UNSTABLE_CAP = 0.02
X_BAR = 1e-6


# ----------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", ADMITTED)
def test_case_is_admissible(name):
    import bootstrap_ref as br
    import refine_ref as rr
    cs = br.case(name)
    base, bad, worst = br.unstable_pairs(cs)
    print(f"{name}: {np.count_nonzero(bad)} of {bad.size} pairs unstable, worst |dx|/(1+|x|) {worst:.2e}; status "
          f"{np.bincount(base['status'].ravel(), minlength=5)}, evals {base['evals'].min()}..{base['evals'].max()}")
    assert np.count_nonzero(bad) <= UNSTABLE_CAP * bad.size
    assert worst <= X_BAR                                    # also an unstable pair stays inside the device's x bar
    assert not np.any(base["status"] == rr.FAILED)
    # the replicates are no copies of the centre: the case exercises the fit
    assert np.all(np.std(base["x"], axis=0) > 0)
    # rule 2 on the case's own data: t_0 rows are the population's, everything else moved by sigma s eps
    S = cs["yhat"].shape[0]
    eps = cs["noise"].reshape(cs["B"], S, cs["T"], cs["N"])
    pop = cs["c"]["data"] if cs["model"] == "supp" else cs["c"]["obs"].T[None]
    assert np.array_equal(cs["ystar"][:, :, 0, :], np.broadcast_to(pop[:, 0, :], (cs["B"], S, cs["N"])))
    b, s, t, i = cs["B"] - 1, S - 1, cs["T"] - 1, cs["N"] - 1
    assert cs["ystar"][b, s, t, i] == cs["yhat"][s, t, i] + (cs["sigma"][i] * cs["scale"][s]) * eps[b, s, t, i]


def test_sigma_zero_gives_the_prediction_itself():
    import bootstrap_ref as br
    rng = np.random.default_rng(1)
    yhat, pop = rng.normal(size=(3, 5, 4)), rng.normal(size=(3, 5, 4))
    y = br.replicate_data(yhat, np.zeros(4), np.array([2.0, 3.0, 4.0]), rng.normal(size=(6, 15, 4)), pop)
    assert y.shape == (6, 3, 5, 4)
    assert np.array_equal(y[:, :, 1:], np.broadcast_to(yhat[:, 1:], (6, 3, 4, 4)))
    assert np.array_equal(y[:, :, 0], np.broadcast_to(pop[:, 0], (6, 3, 4)))


# ----------------------------------------------------------------------------- the per-shape and partial-failure cases
SHAPE_CASES = [("cpep", 0, ()), ("cpep", 1, ()), ("cpep", 8, ()), ("supp", 0, ()), ("supp", 10, ()), ("cpep", 2, ("relu", "softplus")),
               ("supp", 0, ("sigmoid", "identity")), ("supp", 5, ("sigmoid", "softplus"))]


@pytest.mark.parametrize("model,k,acts", SHAPE_CASES, ids=[f"{m}-{k}-{'-'.join(a)}" for m, k, a in SHAPE_CASES])
def test_shape_cases_move_their_subjects(model, k, acts):
    """Check 2 of tests/test_gpu_bootstrap_shapes.py (assert_case_can_fail there) on the restatement, with that file's
    inputs -- tangent_case, centre = its conditional parameters, sigma = sqrt(SSE / rows) there, default_rng(17): at least
    three quarters of the subjects that the box does not pin get three pairwise different replicate estimates, none equal
    to the fit of the population's own data, and every replicate has estimates that no other data give -- so a kernel that
    read the population, or one replicate's slab for every replicate, cannot pass.  The population's data ride along as
    a fourth replicate of the stacked population.  Cases: the first shape of a group of either model, two small ones, and
    the four whose fits run into the box most (the last is that file's one PINNED_CASES entry)."""
    import adaptive_cases as ac
    import bootstrap_ref as br
    import cude_oracle as o
    import refine_ref as rr
    import test_gpu_bootstrap_shapes as bs
    c, cond, box = ac.tangent_case(model, k)
    tag = f"{model} {c['arch']} {'-'.join(acts)}".strip()
    c = dict(c, arch=tuple(c["arch"]) + tuple(acts))
    center, N, T = c[cond], c[cond].size, len(c["tp"])
    if model == "supp":
        rows, pop, scale = 3 * T, np.asarray(c["data"], dtype=np.float64), o.supp_scale(c["data"])
        yhat = br.supp_yhat(c, center)
        sse = br.supp_evaluator(c, pop, scale)(center)[2]
    else:
        rows, pop, scale = T, np.asarray(c["obs"], dtype=np.float64).T[None], np.ones(1)
        yhat = br.cpep_yhat(c, center)
        sse = rr.cpep_evaluator(c)(center)[2]
    noise = np.random.default_rng(bs.NOISE_SEED).standard_normal((bs.B, rows, N))
    ystar = np.concatenate([br.replicate_data(yhat, np.sqrt(sse / rows), scale, noise, pop), pop[None]])
    ev = br.supp_evaluator(c, br.supp_stacked_data(ystar), scale) if model == "supp" else rr.cpep_evaluator(br.cpep_stacked(c, ystar))
    fit = br.refit(ev, center, bs.B + 1, *box, xtol=1e-7, max_step=0.5)
    bs.assert_case_can_fail(tag, fit["x"], fit["status"])


def test_nonfinite_noise_fails_its_replicate_alone_in_the_restatement():
    """The K = 5 case of tests/test_gpu_set_reductions.py::test_partly_failed_subjects on the restatement: by rule 1 of
    cude_refine_conditional a non-finite noise entry behind t_0 makes that replicate's first objective non-finite, so
    exactly the planned (replicate, subject) pairs are FAILED and every other pair is what it was; an entry of a t_0 row
    changes nothing (rule 3)."""
    import bootstrap_ref as br
    import refine_ref as rr
    import test_gpu_set_reductions as sr
    K, chunk = 5, 2
    c, center, sigma, noise = sr.boot_inputs()
    N, T = sr.N_BOOT, len(c["tp"])
    pop, yhat = np.asarray(c["obs"], dtype=np.float64).T[None], br.cpep_yhat(c, center)
    plan = sr.failure_plan(K, chunk)
    want = np.zeros((K, N), dtype=bool)
    z0 = noise[:K].copy()
    for b, i, v in plan:
        want[b, i] = True
        z0[b, 0, i] = v
    assert np.array_equal(br.replicate_data(yhat, sigma, np.ones(1), z0, pop), br.replicate_data(yhat, sigma, np.ones(1), noise[:K], pop))
    fits = []
    for z in (noise[:K], sr.poisoned(noise[:K], plan, T)):
        ystar = br.replicate_data(yhat, sigma, np.ones(1), z, pop)
        fits.append(br.refit(rr.cpep_evaluator(br.cpep_stacked(c, ystar)), center, K, -4.0, 3.0, xtol=1e-7, max_step=0.5))
    clean, got = fits
    assert not np.any(clean["status"] == rr.FAILED)
    assert np.array_equal(got["status"] == rr.FAILED, want)
    assert np.array_equal(got["x"][~want], clean["x"][~want]) and np.array_equal(got["status"][~want], clean["status"][~want])
    s = br.summaries(got["x"], got["status"], sr.boot_ranks(K))
    assert np.array_equal(s["n_used"], K - want.sum(axis=0)) and sorted(set(want.sum(axis=0).tolist())) == [0, 1, 2, K - 1, K]
    assert np.array_equal(np.isnan(s["order"]), sr.boot_ranks(K)[:, None] >= s["n_used"][None, :])


# ----------------------------------------------------------------------------- rule 5
def test_summaries_against_numpy():
    import bootstrap_ref as br
    import refine_ref as rr
    rng = np.random.default_rng(3)
    B, N = 11, 9
    reps = rng.normal(size=(B, N))
    status = rng.integers(0, 4, size=(B, N)).astype(np.int32)
    status[[1, 4, 7], 2] = rr.FAILED                         # three failed replicates
    status[:, 3] = rr.FAILED                                 # nothing left
    status[1:, 4] = rr.FAILED                                # one left
    reps[status == rr.FAILED] = np.nan                       # a failed fit's point must not matter
    ranks = [0, 3, 7, 10]
    got = br.summaries(reps, status, ranks)
    for i in range(N):
        x = reps[status[:, i] != rr.FAILED, i]
        n = x.size
        assert got["n_used"][i] == n
        if n == 0:
            assert np.isnan(got["mean"][i]) and np.isnan(got["sd"][i]) and np.all(np.isnan(got["order"][:, i]))
            continue
        assert abs(got["mean"][i] - np.mean(x)) <= 4 * np.finfo(float).eps * np.max(np.abs(x))
        if n < 2:
            assert np.isnan(got["sd"][i])
        else:
            assert abs(got["sd"][i] - np.std(x, ddof=1)) <= 1e-14 * np.std(x, ddof=1)
        xs = np.sort(x)
        for k, r in enumerate(ranks):
            if r < n:
                assert got["order"][k, i] == xs[r]           # a selection: one of the values, bit for bit
            else:
                assert np.isnan(got["order"][k, i])


# ----------------------------------------------------------------------------- the mirror
class _FakeEngine:
    """bootstrap_conditional from given replicates (B, N): what the device returns, by bootstrap_ref.summaries."""

    def __init__(self, reps, status):
        self.reps, self.status, self.calls = reps, status, []
        self.N = reps.shape[1]

    def set_params(self, nn, cond):
        self.calls.append(("set_params", nn is not None, cond is not None))

    def set_rng(self, seed, subject_offset=0):
        self.calls.append(("set_rng", seed))

    def forward(self, want_sse=False, want_traj=False):
        self.calls.append(("forward",))
        return {"loss": 0.0, "sse": np.full(self.N, 20.0)}

    def bootstrap_conditional(self, sigma, n_reps, center=None, *, ranks=(), noise=None, lower=-4.0, upper=3.0,
                              want_replicates=False, **kw):
        import bootstrap_ref as br
        self.calls.append(("bootstrap", np.array(sigma, dtype=float), int(n_reps), lower, upper, noise))
        s = br.summaries(self.reps, self.status, ranks)
        out = {"order": s["order"], "mean": s["mean"], "sd": s["sd"], "n_used": s["n_used"]}
        if want_replicates:
            out["replicates"], out["status"] = self.reps, self.status
        return out


@pytest.mark.parametrize("B,level", [(200, 0.95), (37, 0.9), (2, 0.5), (1, 0.95)])
def test_mirror_interval_is_numpys_type_7_quantile_of_the_replicates(B, level):
    from cude import api
    rng = np.random.default_rng(B)
    N = 6
    reps = rng.normal(size=(B, N))
    status = np.zeros((B, N), dtype=np.int32)
    if B > 2:
        status[1, 5] = 4                                     # one failed replicate: no interval for that subject
    eng = _FakeEngine(reps, status)
    center = rng.normal(size=N)
    r = api._bootstrap(eng, center, None, 5, B, level, 17, None, -4.0, 1.0, True)
    ok = np.all(status == 0, axis=0)
    want = np.quantile(reps, [0.5 - level / 2, 0.5 + level / 2], axis=0)
    assert np.allclose(r.lower[ok], want[0][ok], rtol=1e-15, atol=1e-15) and np.allclose(r.upper[ok], want[1][ok], rtol=1e-15, atol=1e-15)
    assert np.all(np.isnan(r.lower[~ok])) and np.all(np.isnan(r.upper[~ok]))
    # the ranks asked for are quantile_ranks', the interpolation quantile_lerp's
    ranks, lo, hi, g = api.quantile_ranks([0.5 - level / 2, 0.5 + level / 2], B)
    xs = np.sort(reps, axis=0)
    assert np.array_equal(r.lower[ok], api.quantile_lerp(xs[ranks[lo[0]]], xs[ranks[hi[0]]], g[0])[ok])
    assert np.allclose(r.bias[ok], reps.mean(axis=0)[ok] - center[ok], rtol=0, atol=1e-14)
    if B > 1:
        assert np.allclose(r.se[ok], np.std(reps, axis=0, ddof=1)[ok], rtol=1e-13)
    assert np.array_equal(r.n_used, np.count_nonzero(status != 4, axis=0))
    assert r.replicates is reps
    # sigma = None: sqrt(SSE_i / n_i) at the centre (conditional_standard_errors' convention); the seed reaches the stream
    names = [c[0] for c in eng.calls]
    assert names == ["set_params", "forward", "set_rng", "bootstrap"] and eng.calls[2][1] == 17
    assert np.array_equal(eng.calls[3][1], np.full(N, 2.0)) and eng.calls[3][2:5] == (B, -4.0, 1.0)
    with pytest.raises(ValueError):
        api._bootstrap(eng, center, 1.0, 5, B, 1.0, None, None, -4.0, 1.0, False)


def test_mirror_signatures_and_defaults():
    import inspect
    from cude import api
    from cude.engine import Engine
    p = inspect.signature(api.bootstrap_conditional).parameters
    assert list(p)[:5] == ["betas", "nn", "models", "timepoints", "cpeptide_data"]
    want = dict(sigma=None, n_reps=200, level=0.95, seed=None, noise=None, lower=-4.0, upper=1.0, n_steps=None,
                return_replicates=False)
    assert {k: v.default for k, v in p.items() if v.default is not inspect.Parameter.empty} == want
    q = inspect.signature(api.suppression_bootstrap).parameters
    assert list(q)[:2] == ["p", "args"] and q["n_reps"].default == 200 and q["level"].default == 0.95 and q["n_steps"].default is None
    e, r = inspect.signature(Engine.bootstrap_conditional).parameters, inspect.signature(Engine.refine_conditional).parameters
    for k in ("max_evals", "xtol", "max_step", "penalty_weight", "penalty_center", "lower", "upper"):
        assert e[k].default == r[k].default, k
    jl = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    for needle in ("function bootstrap_conditional(betas, neural_network_parameters, models, timepoints, cpeptide_data; sigma = nothing,",
                   "n_reps = 200, level = 0.95, seed = nothing, noise = nothing, lower = -4.0, upper = 1.0,",
                   "function suppression_bootstrap(p, (prob, individual_data, timepoints, λ); sigma = nothing, n_reps = 200, level = 0.95,",
                   "(:cude_bootstrap_conditional, LIB)", "(:cude_bootstrap_noise, LIB)"):
        assert needle in jl, needle


# ----------------------------------------------------------------------------- the draws
def bootstrap_draw(seed, subject, rep, row):
    """The standard normal rule 3 assigns to (seed, global subject, replicate, row): csrc/cude_rng.h rng_bootstrap_normal."""
    import math
    from conftest import philox4x32_10

    def u01(hi, lo):
        return ((((hi << 32) | lo) >> 11) + 0.5) * 2.0 ** -53
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    c = philox4x32_10([subject & 0xFFFFFFFF, (subject >> 32) & 0xFFFFFFFF, rep & 0xFFFFFFFF,
                       0x80000000 | (((rep >> 32) & 0x7FFF) << 16) | row], key)
    return math.sqrt(-2.0 * math.log(u01(c[0], c[1]))) * math.cos(2.0 * math.pi * u01(c[2], c[3]))


def test_draw_counters_are_a_block_kind_of_their_own():
    """The counter of a bootstrap draw differs from every Metropolis block's (conftest.device_draw: last word = (step >>
    32) << 1 | kind, i.e. below 2^31 for every step below 2^62), and the source states the layout restated above."""
    src = open(os.path.join(ROOT, "conditional-ude_amd", "csrc", "cude_rng.h")).read()
    assert "kRngKindBootstrap = 0x80000000u" in src
    assert "c[3] = kRngKindBootstrap | ((uint32_t)((uint64_t)rep >> 32) << 16) | (uint32_t)row;" in src
    z = np.array([bootstrap_draw(12345, 7, b, r) for b in range(40) for r in range(1, 6)])
    assert np.all(np.isfinite(z)) and abs(z.mean()) < 0.25 and 0.75 < z.std() < 1.25 and np.unique(z).size == z.size
    from conftest import device_draw
    assert bootstrap_draw(12345, 7, 3, 0) != device_draw(12345, 7, 3)[0]


# ----------------------------------------------------------------------------- ABI
PROTO = "int32_t cude_bootstrap_conditional(cude_ctx* ctx, const double* center, const double* sigma, int64_t first_rep,"
PROTO_NOISE = "int32_t cude_bootstrap_noise(cude_ctx* ctx, int64_t first_rep, int32_t n_reps, double* noise_out);"


def test_symbols_are_declared_and_exported():
    from cude import _lib
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    assert PROTO in hdr and PROTO_NOISE in hdr
    for cite in ("suppression/src/suppression_model.jl:39-63", '"bootstrap_chunk"', '"bootstrap_subjects"', "CUDE_BOOTSTRAP_CHUNK",
                 "CUDE_BOOTSTRAP_SUBJECTS", "ONE REPLICATE AT"):
        assert cite in hdr, cite
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cude_bootstrap_conditional", "cude_bootstrap_noise"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()


def test_null_context_returns_a_status():
    from cude import _lib
    lib = _lib.load()
    out = np.zeros(4)
    po = out.ctypes.data_as(ctypes.c_void_p)
    args = (None, None, po, 0, 8, None, -4.0, 3.0, 40, 1e-7, 0.5, 0.0, 0.0, 0, None, None, po, None, None, None, None)
    assert lib.cude_bootstrap_conditional(*args) == -1       # CUDE_ERR_ARG, no abort
    assert b"null context" in lib.cude_last_error()
    assert lib.cude_bootstrap_noise(None, 0, 8, po) == -1


def test_one_statement_of_the_rule_and_of_the_sort():
    """The replicate kernels call the refinement's own device statements, and the reduction sorts with the network the
    predictive bands sort with: neither is restated.  Nor are the tile's geometry, launch and fill, the simulated
    observation and the finiteness test of the kernels around the replicate simulations."""
    csrc = os.path.join(ROOT, "conditional-ude_amd", "csrc")
    refine = open(os.path.join(csrc, "cude_refine.hip")).read()
    assert refine.count("void refine_update(") == 1 and refine.count("refine_update(") == 6       # definition + 5 callers
    for fam in ("cpep_refine_reps_kernel", "supp_refine_reps_kernel"):
        body = refine[refine.index(f"void {fam}("):]
        body = body[:body.index("\n}\n")]
        assert "refine_update(" in body and "_tan_sweep<" in body and "refine_start(" in body
    boot = open(os.path.join(csrc, "cude_bootstrap.hip")).read()
    pred = open(os.path.join(csrc, "cude_predictive.hip")).read()
    assert "tile_sort_ascending(" in boot and "tile_sort_ascending(" in pred
    assert "x[u] > y[u]" not in boot and "x[u] > y[u]" not in pred
    # the frame of the four kernels on the sorting tile is cude_tilesort.h's: each sorts with tile_sort_ascending and is
    # launched by tile_launch on tile_geometry; bootstrap_reduce_kernel, vpc_tile_kernel and vpc_interval_kernel fill the
    # tile with tile_fill and spell no fill loop of their own.  predictive_select_kernel may keep its loop -- through
    # tile_fill it compiled to one scalar move more than before (profiles/replicates_split.txt, "Device code"), and a
    # kernel whose instruction count grows keeps its own words -- or call tile_fill: one of the two, not both.
    vpc = open(os.path.join(csrc, "cude_vpc.hip")).read()
    tile = open(os.path.join(csrc, "cude_tilesort.h")).read()
    assert tile.count("void tile_fill(") == 1 and tile.count("const int cc = idx & (C - 1), e = idx >> lgC;") == 1
    may_keep_its_loop = {"predictive_select_kernel"}
    for kernel, src in (("predictive_select_kernel", pred), ("bootstrap_reduce_kernel", boot), ("vpc_tile_kernel", vpc),
                        ("vpc_interval_kernel", vpc)):
        body = src[src.index(f"void {kernel}("):]
        body = body[:body.index("\n}\n")]
        assert body.count("tile_sort_ascending(") == 1, kernel
        fill = body[:body.index("tile_sort_ascending(")]
        own = fill.count("idx & (C - 1)") + fill.count("idx & (TC - 1)")
        assert own == 0 or (own == 1 and kernel in may_keep_its_loop), kernel
        assert fill.count("tile_fill(") == 1 - own, kernel
        assert src.count(f"tile_launch({kernel}, tile_geometry(") == 1, kernel
    for src in (pred, boot, vpc):
        assert "hipFuncSetAttribute" not in src and "while (" not in src[src.index("hipError_t launch_"):]
    # the simulated observation v + (sigma s) eps has one definition, which both generate / observe kernels call; so has the
    # finiteness test of these files
    obs = open(os.path.join(csrc, "cude_observe.h")).read()
    npde = open(os.path.join(csrc, "cude_npde.hip")).read()
    assert obs.count("double simulated_observation(") == 1 and obs.count("bool finite_value(") == 1
    assert "#pragma clang fp contract(off)" in obs[obs.index("double simulated_observation("):]
    assert boot.count("simulated_observation(") == 1 and npde.count("simulated_observation(") == 1
    for src in (pred, boot, npde, vpc):
        assert "amp * eps" not in src and "1.79769313486231570815e308" not in src


# ----------------------------------------------------------------------------- the new translation unit
def test_cude_bootstrap_cross_compiles_for_gfx950(tmp_path):
    csrc = os.path.join(ROOT, "conditional-ude_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the library cannot be built here either")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        os.path.join(csrc, "cude_bootstrap.hip"), "-o", str(tmp_path / "bootstrap.o")], stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert os.path.getsize(tmp_path / "bootstrap.o") > 5000
