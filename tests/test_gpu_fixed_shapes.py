"""Every compiled FIXED-step loss and gradient kernel, at every shape, on live biases against the CPU oracle.

tests/test_gpu_parity.py::test_every_compiled_shape_against_the_oracle walks the same 24 + 16 shapes on the inputs of
conftest.make_cpep_case / make_supp_case, whose biases are all zero (a kernel that fetched bias j + 1 for unit j passes
there), with one state count per shape and on two option routes.  This module runs the inputs of tests/fixed_cases.py --
every bias live, 70 subjects = a second workgroup of six lanes, three parameter sets that share nothing -- through every
option route that selects another template instance; the docstring of fixed_cases.py is the route table (which option
lands on which instance, with the source line it rests on), tests/test_fixed_cases_host.py holds that table to the source
and shows on the oracle alone that a rotated bias moves these losses by >= 7e-4 and these gradients by >= 3e-2.

Bars: those of tests/test_gpu_parity.py -- loss 1e-10, SSE 1e-10, trajectories 1e-11 of their max (here per state, so that
the quadrature state's larger values do not widen the bar of the other two), gradients 1e-9 of the gradient's max-norm.
Every test prints its largest error / bar per quantity and what its bit comparisons found.  Measured on an MI355X: see
DESIGN.md section 5."""
import contextlib
import time

import numpy as np
import pytest
import torch  # noqa: F401  (imported first so PyTorch and libcude_hip share one HIP runtime)

import adaptive_cases as ac
import fixed_cases as fc
from test_gpu_parity import GRAD_RTOL, LOSS_RTOL, _rel

pytestmark = pytest.mark.gpu

SSE_RTOL, TRAJ_RTOL = 1e-10, 1e-11      # (literals in tests/test_gpu_parity.py)
_DEVICE_ERRORS = []


@contextlib.contextmanager
def _device(who):
    """A status from the library (anything but a failed assertion) ends this module's use of the device: the tests behind
    it fail without launching anything."""
    if _DEVICE_ERRORS:
        pytest.fail(f"not run: {_DEVICE_ERRORS[0]}")
    try:
        yield
    except AssertionError:
        raise
    except BaseException as e:
        _DEVICE_ERRORS.append(f"{who}: {type(e).__name__}: {e}")
        raise


def _bits(x):
    return [np.asarray(v).tobytes() for v in (x if isinstance(x, tuple) else (x,))]


class _Tally:
    """Collects every comparison of one test, prints the largest error / bar per quantity, then fails on any miss."""

    def __init__(self, who):
        self.who, self.worst, self.missed, self.notes, self.t0 = who, {}, [], [], time.perf_counter()

    def hold(self, route, quantity, err, bar, strict=True):
        if not (err < bar if strict else err <= bar):           # (a NaN misses)
            self.missed.append(f"{route}: {quantity} {err:.3e} against {bar:.0e}")
        if quantity not in self.worst or not err / bar <= self.worst[quantity][0]:
            self.worst[quantity] = (err / bar, route)

    def forward(self, route, f, ref, traj=False):
        self.hold(route, "loss", abs(f["loss"] - ref["loss"]) / abs(ref["loss"]), LOSS_RTOL, strict=False)
        self.hold(route, "sse", _rel(f["sse"], ref["sse"]), SSE_RTOL)
        if traj:
            assert f["traj"].shape == ref["traj"].shape, route
            self.hold(route, "traj", max(_rel(a, b) for a, b in zip(f["traj"], ref["traj"])), TRAJ_RTOL)

    def loss(self, route, loss, ref):
        self.hold(route, "loss", abs(loss - ref["loss"]) / abs(ref["loss"]), LOSS_RTOL, strict=False)

    def grad(self, route, got, ref):
        self.loss(route, got[0], ref)
        self.hold(route, "g_nn", _rel(got[1], ref["g_nn"]), GRAD_RTOL)
        self.hold(route, "g_cond", _rel(got[2], ref["g_cond"]), GRAD_RTOL)

    def sets(self, route, got, refs):
        """multistart_loss_grad's (losses, g_nn, g_cond): set j against refs[j % len(refs)]."""
        for j in range(len(got[0])):
            self.grad(f"{route} set {j}", (got[0][j], got[1][j], got[2][j]), refs[j % len(refs)])

    def same_bits(self, route, a, b):
        if _bits(a) != _bits(b):
            self.missed.append(f"{route}: not the same bytes")

    def note(self, text):
        self.notes.append(text)

    def close(self):
        worst = ", ".join(f"{q} {v:.2e} ({r})" for q, (v, r) in self.worst.items())
        print(f"\n{self.who}: largest error / bar: {worst}; {time.perf_counter() - self.t0:.2f} s")
        for n in self.notes:
            print(f"    {n}")
        assert not self.missed, "\n".join(self.missed)


def _cpep_engine(c, n_state, **options):
    from cude.engine import Engine
    eng = Engine("cpep", c["arch"][:3], n_steps=fc.N_STEPS, n_state=n_state)
    for name, value in options.items():                 # before the population: the path and the buffers are fixed there
        eng.set_option(name, value)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    return eng


def _supp_engine(s, **options):
    from cude.engine import Engine
    eng = Engine("supp", s["arch"][:3], n_steps=fc.N_STEPS, lam=fc.SUPP_LAMBDA)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.set_population_supp(s["tp"], s["data"])
    return eng


def _set(got, j):
    return got[0][j], got[1][j], got[2][j]


@pytest.mark.parametrize("k", range(len(fc.CPEP_SHAPES)), ids=[str(a) for a in fc.CPEP_SHAPES])
def test_cpeptide_shape_on_every_route(k):
    arch = fc.CPEP_SHAPES[k]
    c, nn_sets, beta_sets = fc.cpep_fixed_case(k)
    many = np.arange(fc.MANY_SETS) % fc.N_SETS
    t = _Tally(f"c-peptide {arch}")
    with _device(t.who):
        for n_state in (2, 3):
            refs = [fc.cpep_ref(k, n_state, j) for j in range(fc.N_SETS)]
            tag = f"{n_state} states"
            # ---- one lane per subject: cpep_kernel<Net, NS, false> and <Net, NS, true>, one set and three (grid y)
            eng = _cpep_engine(c, n_state, cpep_path="1")
            eng.set_params(nn_sets[0], beta_sets[0])
            f = eng.forward(want_sse=True, want_traj=True)
            assert f["traj"].shape == (n_state, len(ac.TP5), fc.N_SUBJECTS)
            t.forward(f'{tag} "1" forward', f, refs[0], traj=True)
            eng.set_option("lean_clamp", -1)
            plain = eng.loss_grad()
            assert eng.n_failed() == 0
            t.grad(f'{tag} "1" loss_grad', plain, refs[0])
            eng.set_option("lean_clamp", 0)                 # every wave on the clamped sweeps: the same bytes
            clamped = eng.loss_grad()
            t.grad(f'{tag} "1" lean_clamp 0', clamped, refs[0])
            t.same_bits(f'{tag} "1" lean_clamp 0 against -1', clamped, plain)
            eng.set_option("lean_clamp", -1)
            losses = eng.multistart_forward(nn_sets, beta_sets)
            for j in range(fc.N_SETS):
                t.loss(f'{tag} "1" multistart_forward set {j}', losses[j], refs[j])
            got = eng.multistart_loss_grad(nn_sets, beta_sets)
            t.sets(f'{tag} "1" multistart_loss_grad', got, refs)
            t.same_bits(f'{tag} "1" multistart_loss_grad set 0 against loss_grad', _set(got, 0), plain)
            eng.close()
            # ---- kept activations: cpep_kernel<Net, NS, true, 1> and <..., 2> where the shape has them
            for keep in (1, 2):
                eng = _cpep_engine(c, n_state, cpep_path="1", cpep_keep=keep)
                eng.set_params(nn_sets[0], beta_sets[0])
                kept = eng.loss_grad()
                eng.close()
                route = f'{tag} "1" cpep_keep {keep}'
                t.grad(route, kept, refs[0])
                if fc.cpep_has_keep(arch):
                    t.same_bits(f"{route}: loss against cpep_keep 0", kept[0], plain[0])      # the same forward sweep
                    t.note(f"{route} against cpep_keep 0: g_nn {_rel(kept[1], plain[1]):.2e}, g_cond {_rel(kept[2], plain[2]):.2e}"
                           f" of the max-norm")
                else:
                    t.same_bits(f"{route} (no such kernel for this shape) against cpep_keep 0", kept, plain)
            # ---- time-split: cpep2_fwd_kernel<NIN, W, D, NS, VWR> + scan (+ cpep2_rev_kernel)
            for path in ("2:3", "2:7", "2:30"):
                eng = _cpep_engine(c, n_state, cpep_path=path)
                eng.set_params(nn_sets[0], beta_sets[0])
                t.forward(f'{tag} "{path}" forward', eng.forward(want_sse=True), refs[0])
                split = eng.loss_grad()
                assert eng.n_failed() == 0
                t.grad(f'{tag} "{path}" loss_grad', split, refs[0])
                if path == "2:7":                            # three sets in grid z behind the plain scan
                    t.sets(f'{tag} "{path}" multistart_loss_grad', eng.multistart_loss_grad(nn_sets, beta_sets), refs)
                if path == "2:30":
                    # 2 x 30 x 36 = 2160 waves > 2048: the instance WITHOUT the weights in VGPRs, still time-split (2 x 36 <= 512)
                    assert fc.sets_run_time_split(fc.MANY_SETS) and not fc.runs_vwr(30, fc.MANY_SETS) and fc.runs_vwr(30, 1)
                    got = eng.multistart_loss_grad(nn_sets[many], beta_sets[many])
                    t.sets(f'{tag} "{path}" multistart_loss_grad of {fc.MANY_SETS}', got, refs)
                    for j in range(fc.N_SETS, fc.MANY_SETS):
                        t.same_bits(f'{tag} "{path}" set {j} against set {j % fc.N_SETS}', _set(got, j), _set(got, j % fc.N_SETS))
                    # cude_launch.hip eval_sets_device: "a set's result is bit-identical to" cude_loss_grad's -- here across the
                    # two instances of the forward-chunk kernel (measured: the same bytes for all 24 shapes, both state counts)
                    same = _bits(_set(got, 0)) == _bits(split)
                    t.same_bits(f'{tag} "{path}" set 0 of {fc.MANY_SETS} against loss_grad', _set(got, 0), split)
                    t.note(f'{tag} "{path}": set 0 of {fc.MANY_SETS} (plain instance) against loss_grad (VWR instance): '
                           + ("the same bytes" if same else f"loss {abs(got[0][0] - split[0]) / abs(split[0]):.2e}, g_nn "
                              f"{_rel(got[1][0], split[1]):.2e}, g_cond {_rel(got[2][0], split[2]):.2e}"))
                    losses = eng.multistart_forward(nn_sets[many], beta_sets[many])      # (one-lane forward kernel, 36 grid rows)
                    for j in range(fc.MANY_SETS):
                        t.loss(f'{tag} "{path}" multistart_forward set {j} of {fc.MANY_SETS}', losses[j], refs[j % fc.N_SETS])
                        t.same_bits(f'{tag} "{path}" multistart_forward set {j} against set {j % fc.N_SETS}', losses[j],
                                    losses[j % fc.N_SETS])
                eng.close()
            # ---- mixed: block 0 on the one-lane kernel, block 1 in five chunks
            eng = _cpep_engine(c, n_state, cpep_path="3:1:5")
            eng.set_params(nn_sets[0], beta_sets[0])
            mixed = eng.loss_grad()
            assert eng.n_failed() == 0
            eng.close()
            t.grad(f'{tag} "3:1:5" loss_grad', mixed, refs[0])
    t.close()


@pytest.mark.parametrize("k", range(len(fc.SUPP_SHAPES)), ids=[str(s) for s in fc.SUPP_SHAPES])
def test_suppression_shape_on_every_route(k):
    s, nn_sets, theta_sets = fc.supp_fixed_case(k)
    refs = [fc.supp_ref(k, j) for j in range(fc.N_SETS)]
    t = _Tally(f"suppression {s['arch']}")
    out = {}
    with _device(t.who):
        # supp_kernel<W, D, true, STORE = true>, <W, D, true, false> and <W, D, true, false, YONLY = true>
        for route, options in (("supp_store 1", dict(supp_store=1)), ("supp_store 0", dict(supp_store=0)),
                               ("supp_ckpt steps", dict(supp_ckpt="steps"))):
            eng = _supp_engine(s, **options)
            eng.set_params(nn_sets[0], theta_sets[0])
            if route == "supp_store 1":                     # supp_kernel<W, D, false, false>
                f = eng.forward(want_sse=True, want_traj=True)
                t.forward("forward", f, refs[0], traj=True)
                losses = eng.multistart_forward(nn_sets, theta_sets)
                for j in range(fc.N_SETS):
                    t.loss(f"multistart_forward set {j}", losses[j], refs[j])
            one = eng.loss_grad()
            assert eng.n_failed() == 0
            t.grad(f"{route} loss_grad", one, refs[0])
            sets = eng.multistart_loss_grad(nn_sets, theta_sets)
            t.sets(f"{route} multistart_loss_grad", sets, refs)
            eng.close()
            out[route] = (one, sets)
    for q, what in enumerate(("loss_grad", "multistart_loss_grad")):
        t.same_bits(f"supp_store 1 against 0, {what}", out["supp_store 1"][q], out["supp_store 0"][q])
        same = _bits(out["supp_ckpt steps"][q]) == _bits(out["supp_store 0"][q])
        t.note(f"supp_ckpt steps against supp_store 0, {what}: " + ("the same bytes" if same else "g_nn " + (
            f"{_rel(out['supp_ckpt steps'][q][1], out['supp_store 0'][q][1]):.2e} of the max-norm")))
    t.close()


def _general(eng, nn, cond):
    eng.set_params(nn, cond)
    f = eng.forward(want_sse=True)
    one = eng.loss_grad()
    assert eng.n_failed() == 0
    sets = eng.multistart_loss_grad(nn[None, :], cond[None, :])
    eng.close()
    return f, one, sets


def test_cpeptide_general_activation_kernels_on_live_biases():
    """cpep_kernel over CpepNetG<NIN, W, D, HA, OA>: the 3 shapes x 5 activation pairs x both state counts (no time-split
    kernels for these).  With an identity output the output bias cancels in the production term (network minus its
    baseline value), so that one entry of the gradient is exactly zero in oracle and kernel alike."""
    t = _Tally("c-peptide, other activation functions")
    with _device(t.who):
        for shape in ac.CPEP_GENERAL_SHAPES:
            c, nn_sets, beta_sets = fc.cpep_fixed_case(fc.CPEP_SHAPES.index(shape))
            for acts in ac.GENERAL_ACTS:
                ref = fc.cpep_general_ref(shape, acts)
                for n_state in (2, 3):
                    eng = _cpep_engine(c, n_state, hidden_activation=acts[0], output_activation=acts[1])
                    f, one, sets = _general(eng, nn_sets[0], beta_sets[0])
                    route = f"{shape} {acts[0]} / {acts[1]}, {n_state} states"
                    t.forward(f"{route} forward", f, ref)
                    t.grad(f"{route} loss_grad", one, ref)
                    t.same_bits(f"{route} multistart_loss_grad of one set against loss_grad", _set(sets, 0), one)
    t.close()


def test_suppression_general_activation_kernels_on_live_biases():
    """supp_kernel<W, D, GRAD, false, false, HA, OA>: the 2 shapes x 5 activation pairs."""
    t = _Tally("suppression, other activation functions")
    with _device(t.who):
        for shape in ac.SUPP_GENERAL_SHAPES:
            s, nn_sets, theta_sets = fc.supp_fixed_case(fc.SUPP_SHAPES.index(shape))
            for acts in ac.GENERAL_ACTS:
                ref = fc.supp_general_ref(shape, acts)
                eng = _supp_engine(s, hidden_activation=acts[0], output_activation=acts[1])
                f, one, sets = _general(eng, nn_sets[0], theta_sets[0])
                route = f"{shape} {acts[0]} / {acts[1]}"
                t.forward(f"{route} forward", f, ref)
                t.grad(f"{route} loss_grad", one, ref)
                t.same_bits(f"{route} multistart_loss_grad of one set against loss_grad", _set(sets, 0), one)
    t.close()
