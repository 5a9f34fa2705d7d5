"""Every compiled kernel of the replicate family of the fused fits (csrc/cude_refine.hip cpep_refine_reps_kernel<Net>,
supp_refine_reps_kernel<W, D, HA, OA>: what cude_bootstrap_conditional launches in fixed-step mode), for every shape it
is compiled for, against its plain twin -- on inputs whose biases are not zero (tests/adaptive_cases.py).
tests/test_gpu_bootstrap.py runs four of these kernels, on Glorot parameters, whose biases are zero.

Oracle: the library's own one-replicate fused fit, Engine.refine_conditional, in a SECOND context whose observations are
one replicate's data -- the loop a caller wrote before the replicate launch existed (replicate_loop below; also route
(i) of tools/time_bootstrap.py).  tests/test_gpu_tangent_shapes.py groups d and e hold that kernel to tests/refine_ref.py
on every shape with these inputs.  Rule 2 forms the replicate data without contraction, so the host rebuilds them to the
bit (bootstrap_ref.replicate_data) from forward(want_traj=True) at the centre and the noise passed in.  A replicate kernel
differs from its twin in three places -- the data pointer (slab + blockIdx.y * slab_stride), the block offset (blockIdx.x
+ blk_first) and the store (blockIdx.y * rep_stride + i) -- and calls the same sweep and the same rule, so the bar is
bit equality of every estimate and status (WEAKER below names the shapes that have another bar, and why: none).

Which kernel a call lands on is not observable through the engine; the dispatch rule, restated
(csrc/cude_refine.hip launch_cpep_refine / launch_supp_refine with reps != nullptr, option "refine_fused" = 1):

  c-peptide, tanh / softplus   cpep_refine_reps_kernel<Mlp<nin, w, d, 1>>, one kernel for either n_state: CUDE_CPEP_SHAPES_0
                               in translation unit 0, _1 in 1, _2 in 2
  another activation pair      cpep_refine_reps_kernel<CpepNetG<nin, w, d, HA, OA>>: the 3 CUDE_CPEP_GENERAL_SHAPES x the 5
                               CUDE_GENERAL_ACTS (unit 1)
  symbolic model               cpep_refine_reps_kernel<MmProd<true>> (cond_space "raw") / <MmProd<false>> ("log")
  suppression                  supp_refine_reps_kernel<w, d, tanh, softplus>: the 16 CUDE_SUPP_SHAPES; <w, d, HA, OA>: the 2
                               CUDE_SUPP_GENERAL_SHAPES x 5 pairs

Compiled kernels reached: 67 of 67
  a. tuned c-peptide shapes       test_cpep_replicate_kernel[(nin, w, d)]                        24 of 24
  b. symbolic productions         test_symbolic_replicate_kernel[raw], [log]                      2 of 2
  c. general c-peptide kernels    test_cpep_replicate_kernel_general_activations[shape-acts]     15 of 15
  d. tuned suppression shapes     test_supp_replicate_kernel[(w, d)]                             16 of 16
  e. general suppression kernels  test_supp_replicate_kernel_general_activations[shape-acts]     10 of 10
  (test_cpep_replicate_kernel_three_states: the first shape of each CUDE_CPEP_SHAPES_* group again with n_state 3 -- the
  same kernels, another stride of the centre's trajectory, BootstrapGenArgs::traj_states)

Inputs: ac.tangent_case(model, k) (its own box; 70 subjects for the first shape of each group -- a second workgroup whose
last 58 lanes are padding --, 16 / 12 otherwise); centre = the case's conditional parameters; sigma_i = sqrt(SSE_i / rows)
of forward at the centre; noise np.random.default_rng(17).standard_normal((3, rows, N)).  B = 3 under "bootstrap_chunk" =
2: blockIdx.y is 0 and 1 in the first launch and 0 in a second one whose result pointer has moved; the 70-subject shapes
again under "bootstrap_subjects" = 64 (blk_first = 1 in the second pass).

Per shape, every figure printed before it is asserted (pytest -s; DESIGN.md section 5 records the counts per group):
  1. replicates[b] and status[b] equal the twin's fit of replicate b's data, bit for bit, b = 0, 1, 2;
  2. the test can fail: for at least three quarters of the subjects that the box does not pin (moved_subjects below says
     why not of all) the three estimates differ pairwise and from the fit of the population's own data (a kernel that
     read the population, or replicate 0's slab for every y, gives equal ones);
     tests/test_bootstrap_host.py::test_shape_cases_move_their_subjects shows the same on the restatement;
  3. n_used, mean and order (ranks 0, 1, 2) against bootstrap_ref.summaries of the device's own replicates: n_used and
     order exact, mean within 1e-13; no FAILED replicate."""
import numpy as np
import pytest

import adaptive_cases as ac
import bootstrap_ref as br

pytestmark = pytest.mark.gpu

CPEP_IDS = [str(a) for a in ac.CPEP_SHAPES]
SUPP_IDS = [str(s) for s in ac.SUPP_SHAPES]
ACT_IDS = ["-".join(a) for a in ac.GENERAL_ACTS]
B, CHUNK, NOISE_SEED = 3, 2, 17
MOVED_SHARE, LONE_FLOOR = 0.75, 2               # (moved_subjects below)
# tag of a case that cannot meet LONE_FLOOR in every replicate -> (replicates it is asked of, why)
PINNED_CASES = {"supp (4, 3, 3) sigmoid-softplus": (2, "32 of its 36 replicate fits end AT_BOUND (also in the restatement): 4, 4 and "
                                                       "0 lone estimates -- nothing of replicate 2 depends on its data alone")}
X_BAR = 1e-6                                    # tests/test_gpu_refine.py's
# tag of a shape whose two correctly compiled kernels differ in bits -> why; such a shape is held to |dx| <= X_BAR (1 + |x|)
# for every pair, equal status for every bit-equal pair, at most 2 % of its pairs different
# (tests/test_bootstrap_host.py UNSTABLE_CAP).  Empty: every shape is held to bit equality.
WEAKER = {}


def moved_subjects(x, status):
    """x, status (B + 1, N): the replicate fits and, last, the fit of the population's own data.  -> (moved (N,), free
    (N,), lone (B, N)), bool.  moved: the subject's B + 1 estimates differ pairwise.  free: at most one of its B + 1 fits
    is PINNED, i.e. ended AT_BOUND or FLAT.  lone: the replicate's estimate equals no other of the subject's B + 1.

    The cases' observations are not the model's own (adaptive_cases: 0.5 + uniform noise), so about a third of the fits
    run into the box (the restatement: 90 of 280 fits of cpep (2, 4, 2), 88 of 280 of supp (3, 5), 27 of 64 of cpep (2,
    6, 2)); two fits at one bound are one number whatever the data, and a FLAT fit keeps the centre.  Such a subject
    cannot show that its replicates were read from different data, so the three-quarters share is asked of the free
    subjects (MOVED_SHARE).  What a case needs in order to tell a kernel that reads the population's data, or another
    replicate's, is in every replicate an estimate that only that replicate's data give: LONE_FLOOR lone estimates per
    replicate (two, so that not everything hangs on one number)."""
    n = x.shape[0]
    same = np.array([[np.count_nonzero(x[:, i] == x[b, i]) for i in range(x.shape[1])] for b in range(n)])
    pinned = (status == 1) | (status == 3)                   # CUDE_REFINE_AT_BOUND, CUDE_REFINE_FLAT
    return np.all(same == 1, axis=0), pinned.sum(axis=0) <= 1, same[:n - 1] == 1


def assert_case_can_fail(tag, x, status):
    moved, free, lone = moved_subjects(x, status)
    N = moved.size
    print(f"{tag}: {np.count_nonzero(moved)} of {N} subjects with {x.shape[0] - 1} different estimates, none the population's; "
          f"{np.count_nonzero(moved & free)} of the {np.count_nonzero(free)} with at most one pinned fit; lone estimates per "
          f"replicate {lone.sum(axis=1).tolist()}; status {np.bincount(status.ravel(), minlength=5).tolist()}")
    assert np.count_nonzero(moved & free) >= MOVED_SHARE * np.count_nonzero(free)
    floor = lone.sum(axis=1) >= LONE_FLOOR
    assert np.all(floor[:PINNED_CASES[tag][0]] if tag in PINNED_CASES else floor)


def replicate_loop(eng, upload, ystar, center, box, **kw):
    """The host loop the replicate launch replaces: per replicate b, `upload(eng, ystar[b])` puts its observations into the
    context `eng` and refine_conditional fits them from the centre.  -> x (B, N), status (B, N) int32, evals (B, N) int32."""
    n, N = ystar.shape[0], np.size(center)
    x, st, ev = np.empty((n, N)), np.empty((n, N), dtype=np.int32), np.empty((n, N), dtype=np.int32)
    for b in range(n):
        upload(eng, ystar[b])
        r = eng.refine_conditional(center, *box, **kw)
        x[b], st[b], ev[b] = r["x"], r["status"], r["evals"]
    return x, st, ev


def cpep_upload(c):
    def upload(eng, y):                                      # y: (1, T, N) of one replicate
        eng.set_population_cpep(c["tp"], c["G"], np.ascontiguousarray(y[0].T), c["age"], c["t2dm"])
    return upload


def supp_upload(c, N, scale):
    def upload(eng, y):                                      # y: (3, T, N); the loss weights stay the population's (rule 2)
        eng.set_population_supp(c["tp"], y)
        eng.set_global_subjects(N, scale)
    return upload


def _check(tag, make, supp, c, center, box, two_workgroups, max_step=0.5):
    """make() -> a context on the case's population with the shared parameters set."""
    N = center.size
    T = len(c["tp"])
    rows = 3 * T if supp else T
    eng = make()
    eng.set_params(None, center)
    f = eng.forward(want_sse=True, want_traj=True)
    yhat = np.ascontiguousarray(f["traj"] if supp else f["traj"][:1])
    sigma = np.sqrt(f["sse"] / rows)
    assert np.all(np.isfinite(sigma)) and np.all(sigma > 0)
    noise = np.random.default_rng(NOISE_SEED).standard_normal((B, rows, N))
    scale = np.asarray(eng.get_scale()[0], dtype=np.float64) if supp else np.ones(1)
    pop = np.asarray(c["data"], dtype=np.float64) if supp else np.asarray(c["obs"], dtype=np.float64).T[None]
    ystar = br.replicate_data(yhat, sigma, scale, noise, pop)
    # ---- the twin: a second context, one replicate's data at a time
    twin = make()
    own = twin.refine_conditional(center, *box, max_step=max_step)          # the population's own data
    x, st, ev = replicate_loop(twin, supp_upload(c, N, scale) if supp else cpep_upload(c), ystar, center, box, max_step=max_step)
    twin.close()
    print(f"{tag} N {N}: twin status {np.bincount(st.ravel(), minlength=5).tolist()}, evals {ev.min()}..{ev.max()}")
    # ---- 2. the test can fail
    assert_case_can_fail(tag, np.vstack([x, own["x"][None]]), np.vstack([st, own["status"][None]]))
    splits = [(("bootstrap_chunk", CHUNK),)]
    if two_workgroups:
        assert N == 70
        splits.append((("bootstrap_chunk", CHUNK), ("bootstrap_subjects", 64)))
    for options in splits:
        for k, v in options:
            eng.set_option(k, v)
        got = eng.bootstrap_conditional(sigma, B, center, ranks=[0, 1, 2], noise=noise, lower=box[0], upper=box[1],
                                        max_step=max_step, want_replicates=True)
        n_failed = eng.n_failed()
        # ---- 1. the twin, bit for bit
        differ = got["replicates"] != x
        dx = np.abs(got["replicates"] - x) / (1 + np.abs(x))
        print(f"{tag} {dict(options)}: estimates differ in bits for {np.count_nonzero(differ)} of {B * N} pairs (max |dx|/(1+|x|) "
              f"{dx.max():.2e}), statuses for {np.count_nonzero(got['status'] != st)}")
        if tag in WEAKER:
            assert np.all(dx <= X_BAR) and np.array_equal(got["status"][~differ], st[~differ])
            assert np.count_nonzero(differ) <= 0.02 * differ.size
        else:
            assert np.array_equal(got["replicates"], x) and np.array_equal(got["status"], st)
        # ---- 3. rule 5 on the device's own table
        ref = br.summaries(got["replicates"], got["status"], [0, 1, 2])
        dm = np.max(np.abs(got["mean"] - ref["mean"]) / np.abs(ref["mean"]))
        print(f"{tag}: mean vs the restatement {dm:.2e} (relative), n_failed {n_failed}")
        assert np.array_equal(got["n_used"], ref["n_used"]) and np.all(got["n_used"] == B) and n_failed == 0
        assert np.array_equal(got["order"], ref["order"])
        assert np.allclose(got["mean"], ref["mean"], rtol=1e-13, atol=0)
    eng.close()


def _shape(model, k, n_state=None, acts=()):
    from test_gpu_tangent_shapes import _engine
    c, cond, box = ac.tangent_case(model, k)
    supp = model == "supp"
    n_state = (3 if supp else 2) if n_state is None else n_state
    shape = ac.SUPP_SHAPES[k] if supp else ac.CPEP_SHAPES[k]
    two = shape in (ac.SUPP_TWO_WORKGROUPS if supp else ac.TWO_WORKGROUPS)
    tag = f"{model} {c['arch']} {'-'.join(acts)}".strip() + (" n_state 3" if model == "cpep" and n_state == 3 else "")
    _check(tag, lambda: _engine(model, c, 30, n_state, acts), supp, c, c[cond], box, two)


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_replicate_kernel(k):
    _shape("cpep", k)


@pytest.mark.parametrize("shape", ac.TWO_WORKGROUPS, ids=str)
def test_cpep_replicate_kernel_three_states(shape):
    _shape("cpep", ac.CPEP_SHAPES.index(shape), n_state=3)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_replicate_kernel(k):
    _shape("supp", k)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.CPEP_GENERAL_SHAPES, ids=str)
def test_cpep_replicate_kernel_general_activations(shape, acts):
    _shape("cpep", ac.CPEP_SHAPES.index(shape), acts=acts)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.SUPP_GENERAL_SHAPES, ids=str)
def test_supp_replicate_kernel_general_activations(shape, acts):
    _shape("supp", ac.SUPP_SHAPES.index(shape), acts=acts)


def symbolic_case(space):
    """The symbolic model's population of tests/test_gpu_refine.py (24 subjects, observations of its own solve at k = 20
    exp(beta) with 5 % noise) -> (case, centre, box, max_step): k = 20 in the box and with the step of that file's "sym-raw"
    for cond_space "raw", their logarithms and the default step for "log"."""
    import test_gpu_refine as tg
    c = tg._case_data("sym-raw")
    if space == "raw":
        return c, np.full(24, 20.0), tg.CASES["sym-raw"][4], tg.CASES["sym-raw"][6]
    return c, np.full(24, np.log(20.0)), (float(np.log(0.5)), float(np.log(400.0))), 0.5


@pytest.mark.parametrize("space", ["raw", "log"])
def test_symbolic_replicate_kernel(space):
    import test_gpu_refine as tg
    from cude.engine import Engine
    c, center, box, max_step = symbolic_case(space)

    def make():
        eng = Engine("cpep_sym", (1, 0, 0), n_steps=tg.SYM_STEPS, n_state=2, cond_space=space)
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        eng.set_params(c["nn"], center)
        return eng
    _check(f"symbolic {space}", make, False, c, center, box, False, max_step)
