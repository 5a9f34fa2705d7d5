"""Thin object wrapper over the C ABI: one Engine = one cude_ctx = one GPU.

Holds no numerics: every number comes from libcude_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import COND_LOG, COND_RAW, MODEL_CPEP, MODEL_CPEP_SYM, MODEL_SUPP, CudeError, check


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def n_params(nn_in, width, depth):
    return check(_lib.load().cude_n_params(nn_in, width, depth))


_OBJECTIVE = C.CFUNCTYPE(C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                         C.c_void_p)


def lbfgs_minimize(fg, x0, maxiters=1000):
    """The library's host-side L-BFGS + BackTracking (cude_lbfgs_minimize; needs no GPU) on a Python objective
    fg(x) -> (f, g).  Returns dict(x, f, iterations, f_calls, converged) like cude.lbfgs.lbfgs."""
    x0 = _f64(x0).reshape(-1)
    n = x0.size

    err = []

    def thunk(xp, nn, fp, gp, _user):
        try:
            f, g = fg(np.ctypeslib.as_array(xp, shape=(nn,)).copy())
            fp[0] = float(f)
            np.ctypeslib.as_array(gp, shape=(nn,))[:] = g
            return 0
        except BaseException as e:      # a ctypes callback must not raise: hand the error back through the status
            err.append(e)
            return -1
    cb = _OBJECTIVE(thunk)
    x = np.empty(n)
    f, it, calls, conv = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.load().cude_lbfgs_minimize(n, _ptr(x0), int(maxiters), C.cast(cb, C.c_void_p), None, _ptr(x),
                                         C.byref(f), C.byref(it), C.byref(calls), C.byref(conv))
    if err:
        raise err[0]
    check(rc)
    return dict(x=x, f=f.value, iterations=it.value, f_calls=calls.value, converged=bool(conv.value))


_CANDIDATES = C.CFUNCTYPE(C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
_REDUCE = C.CFUNCTYPE(C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_void_p)

# status codes of Engine.refine_conditional (CUDE_REFINE_* of include/cude.h)
REFINE_CONVERGED, REFINE_AT_BOUND, REFINE_MAX_EVALS, REFINE_FLAT, REFINE_FAILED = range(5)
# status bits of Engine.npde (CUDE_NPDE_* of include/cude.h)
NPDE_SINGULAR, NPDE_FEW, NPDE_FAILED_SIMS, NPDE_BAD_OBS = 1, 2, 4, 8
# status bits of Engine.vpc (CUDE_VPC_* of include/cude.h)
VPC_NO_GROUP, VPC_FAILED_SIMS, VPC_BAD_OBS = 1, 2, 4
# status bits of Engine.profile_intervals (CUDE_CI_* of include/cude.h)
CI_LOWER_OPEN, CI_UPPER_OPEN, CI_DISCONNECTED, CI_EMPTY, CI_CENTER_FAILED, CI_BELOW_CENTER = 1, 2, 4, 8, 16, 32


def lbfgs_minimize_sharded(fg, x0, n_shared, reduce, maxiters=1000):
    """cude_lbfgs_minimize_sharded: x = [shared (n_shared, replicated); local]; fg(x) -> (global f, local g);
    reduce(values: ndarray, op) -> ndarray sums (op 0) / maximises (op 1) over the ranks."""
    x0 = _f64(x0).reshape(-1)
    n = x0.size

    err = []

    # A callback that raised would leave this rank on a different L-BFGS path from its peers, which then block in the
    # next collective: the error goes back through the status (rc < 0 -> CUDE_ERR_ARG / CUDE_ERR_COMM) and is re-raised
    # here once the library has returned.
    def thunk(xp, nn, fp, gp, _user):
        try:
            f, g = fg(np.ctypeslib.as_array(xp, shape=(nn,)).copy())
            fp[0] = float(f)
            np.ctypeslib.as_array(gp, shape=(nn,))[:] = g
            return 0
        except BaseException as e:
            err.append(e)
            return -1

    def red(vp, count, op, _user):
        try:
            v = np.ctypeslib.as_array(vp, shape=(count,))
            v[:] = reduce(v.copy(), int(op))
            return 0
        except BaseException as e:
            err.append(e)
            return -1
    cb, rcb = _OBJECTIVE(thunk), _REDUCE(red)
    x = np.empty(n)
    f, it, calls, conv = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.load().cude_lbfgs_minimize_sharded(n, int(n_shared), _ptr(x0), int(maxiters), C.cast(cb, C.c_void_p),
                                                 C.cast(rcb, C.c_void_p), None, _ptr(x), C.byref(f), C.byref(it),
                                                 C.byref(calls), C.byref(conv))
    if err:
        raise err[0]
    check(rc)
    return dict(x=x, f=f.value, iterations=it.value, f_calls=calls.value, converged=bool(conv.value))


def device_count():
    n = C.c_int32(0)
    check(_lib.load().cude_device_count(C.byref(n)))
    return n.value


class Engine:
    """model: 'cpep' | 'supp' | 'cpep_sym'.  arch = (nn_in, width, depth); (1, 0, 0) for 'cpep_sym' (the analytic
    production p0*dG/(dG+k): parameters [p0], conditional k or log k according to cond_space = 'raw' | 'log')."""

    def __init__(self, model, arch=(1, 0, 0), n_steps=30, n_state=None, lam=0.0, device=0, cond_space="log"):
        self._lib = _lib.load()
        self.model = {"cpep": MODEL_CPEP, "supp": MODEL_SUPP, "cpep_sym": MODEL_CPEP_SYM}[model]
        # the general form `chain(widths, activation_functions; input_dims, output_activation)`: arch = (nn_in, [widths],
        # [one activation per hidden layer], output activation), names as in ACTIVATIONS (cude_set_network)
        general = None
        if len(arch) >= 2 and isinstance(arch[1], (list, tuple)):
            widths = [int(w) for w in arch[1]]
            hidden = arch[2] if len(arch) > 2 else "tanh"
            hidden = [hidden] * len(widths) if isinstance(hidden, str) else list(hidden)
            if len(hidden) != len(widths):
                raise ValueError("The number of widths must match the number of activation functions.")
            general = (widths, hidden + [arch[3] if len(arch) > 3 else "softplus"])
            arch = (arch[0], max(widths), len(widths))
        self.arch = tuple(int(v) for v in arch[:3])
        if n_state is None:
            n_state = 3 if self.model == MODEL_SUPP else 2
        space = {"log": COND_LOG, "raw": COND_RAW}[cond_space]
        cfg = _lib.Config(self.model, n_state, self.arch[0], self.arch[1], self.arch[2], int(n_steps), int(device),
                          space, float(lam))
        h = C.c_void_p()
        check(self._lib.cude_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.n_state = n_state
        self.lam = float(lam)
        self.N = 0
        self.T = 0
        if general is not None:
            self.set_network(*general)
        self.P, self.fallback_kernel = self.network_info()

    ACTIVATIONS = {"tanh": 0, "relu": 1, "sigmoid": 2, "softplus": 3, "identity": 4}

    def set_network(self, widths, activations):
        """cude_set_network: per-layer widths and activation names (hidden layers, then the output layer's).  Before the
        population is uploaded.  Shapes without a tuned kernel run on the fallback kernel (csrc/cude_generic.hip)."""
        w = (C.c_int32 * len(widths))(*[int(v) for v in widths])
        a = (C.c_int32 * len(activations))(*[self.ACTIVATIONS[str(v)] for v in activations])
        if len(activations) != len(widths) + 1:
            raise ValueError("one activation per hidden layer and one for the output layer")
        check(self._lib.cude_set_network(self._h, len(widths), w, a))
        self.P, self.fallback_kernel = self.network_info()

    def network_info(self):
        """(number of shared parameters, True if the network runs on the fallback kernel)."""
        p, g = C.c_int32(), C.c_int32()
        check(self._lib.cude_network_info(self._h, C.byref(p), C.byref(g)))
        return p.value, bool(g.value)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.cude_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tolerances(self, abstol=1e-6, reltol=1e-3):
        """Tolerances of the adaptive mode (n_steps = 0)."""
        check(self._lib.cude_set_tolerances(self._h, float(abstol), float(reltol)))

    def adaptive_steps(self, subject):
        """(t_n, dt_n) of the steps `subject` accepted in the last gradient evaluation (adaptive mode): `sol.t`."""
        n = C.c_int32(0)
        check(self._lib.cude_adaptive_steps(self._h, int(subject), 0, None, None, C.byref(n)))
        t, dt = np.empty(n.value), np.empty(n.value)
        check(self._lib.cude_adaptive_steps(self._h, int(subject), n.value, _ptr(t), _ptr(dt), C.byref(n)))
        return t, dt

    # -- population
    def set_population_cpep(self, timepoints, glucose, cpeptide, age, t2dm):
        """glucose, cpeptide: (N, T) arrays (any strides are honoured without a host copy when
        they are element-strided float64)."""
        tp = _f64(timepoints)
        g = np.asarray(glucose, dtype=np.float64)
        cp = np.asarray(cpeptide, dtype=np.float64)
        if g.shape != cp.shape or g.ndim != 2 or g.shape[1] != tp.size:
            raise ValueError("glucose/cpeptide must be (N, T) with T = len(timepoints)")
        if g.strides != cp.strides or g.strides[0] % 8 or g.strides[1] % 8:
            g, cp = np.ascontiguousarray(g), np.ascontiguousarray(cp)
        N, T = g.shape
        age = _f64(age)
        t2 = np.ascontiguousarray(t2dm, dtype=np.uint8)
        if age.size != N or t2.size != N:
            raise ValueError("age/t2dm must have N entries")
        check(self._lib.cude_set_population_cpep(self._h, N, T, _ptr(tp), _ptr(g), _ptr(cp), g.strides[0] // 8,
                                                 g.strides[1] // 8, _ptr(age), _ptr(t2)))
        self.N, self.T = N, T

    def set_population_supp(self, timepoints, data):
        """data: (3, T, N) array (Julia individual_data); passed in Julia column-major order."""
        tp = _f64(timepoints)
        d = np.asarray(data, dtype=np.float64)
        if d.ndim != 3 or d.shape[0] != 3 or d.shape[1] != tp.size:
            raise ValueError("data must be (3, T, N)")
        dcol = np.ascontiguousarray(d.transpose(2, 1, 0))
        N, T = d.shape[2], d.shape[1]
        check(self._lib.cude_set_population_supp(self._h, N, T, _ptr(tp), _ptr(dcol)))
        self.N, self.T = N, T

    # -- parameters
    def set_params(self, nn=None, cond=None):
        nn_a = None if nn is None else _f64(nn)
        cd_a = None if cond is None else _f64(cond).reshape(-1)
        if nn_a is not None and nn_a.size != self.P:
            raise ValueError(f"expected {self.P} network parameters, got {nn_a.size}")
        if cd_a is not None and cd_a.size != self.N:
            raise ValueError(f"expected {self.N} conditional parameters, got {cd_a.size}")
        check(self._lib.cude_set_params(self._h, _ptr(nn_a), _ptr(cd_a)))

    def get_params(self):
        nn = np.empty(self.P)
        cond = np.empty(self.N)
        check(self._lib.cude_get_params(self._h, _ptr(nn), _ptr(cond)))
        return nn, cond

    # -- evaluation
    def forward(self, want_sse=False, want_traj=False):
        loss = C.c_double()
        sse = np.empty(self.N) if want_sse else None
        traj = np.empty((self.N, self.T, self.n_state)) if want_traj else None
        check(self._lib.cude_forward(self._h, C.byref(loss), _ptr(sse), _ptr(traj)))
        out = {"loss": loss.value}
        if want_sse:
            out["sse"] = sse
        if want_traj:
            out["traj"] = traj.transpose(2, 1, 0)     # -> (n_state, T, N), the Julia Array(sol) shape
        return out

    def simulate(self, times):
        """States of every subject at arbitrary non-decreasing times inside the population's time span (dense
        output of the same solve, fixed-step or adaptive) -> array (n_state, len(times), N).  Entries a subject's failed
        adaptive solve does not reach are NaN."""
        t = _f64(times).reshape(-1)
        out = np.empty((self.N, t.size, self.n_state))
        check(self._lib.cude_simulate(self._h, t.size, _ptr(t), _ptr(out)))
        return np.ascontiguousarray(out.transpose(2, 1, 0))

    def sensitivity(self, want_sens=True):
        """cude_sensitivity at the context's parameters: dict(sens (n_state, T, N) = d u / d cond_i (None unless
        want_sens), info (N,), score (N,), sse (N,)); failed subjects are NaN."""
        sens = np.empty((self.N, self.T, self.n_state)) if want_sens else None
        info, score, sse = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        check(self._lib.cude_sensitivity(self._h, _ptr(sens), _ptr(info), _ptr(score), _ptr(sse)))
        return {"sens": None if sens is None else sens.transpose(2, 1, 0), "info": info, "score": score, "sse": sse}

    def curvature(self, want_sens2=True):
        """cude_curvature at the context's parameters: dict(sens2 (n_state, T, N) = d^2 u / d cond_i^2 (None unless
        want_sens2), curv (N,) = (1/2) d^2 SSE_i / d cond_i^2 (may be <= 0), info (N,), score (N,), sse (N,)); failed
        subjects are NaN."""
        sens2 = np.empty((self.N, self.T, self.n_state)) if want_sens2 else None
        curv, info, score, sse = np.empty(self.N), np.empty(self.N), np.empty(self.N), np.empty(self.N)
        check(self._lib.cude_curvature(self._h, _ptr(sens2), _ptr(curv), _ptr(info), _ptr(score), _ptr(sse)))
        return {"sens2": None if sens2 is None else sens2.transpose(2, 1, 0), "curv": curv, "info": info, "score": score,
                "sse": sse}

    def multistart_forward(self, nn_sets, cond_sets):
        """Losses of K candidate (network, conditional) parameter sets in one launch.
        nn_sets: (K, P); cond_sets: (K, N)."""
        nn = _f64(nn_sets)
        cd = _f64(cond_sets)
        if nn.ndim != 2 or nn.shape[1] != self.P or cd.shape != (nn.shape[0], self.N):
            raise ValueError(f"expected nn_sets (K, {self.P}) and cond_sets (K, {self.N})")
        losses = np.empty(nn.shape[0])
        check(self._lib.cude_multistart_forward(self._h, nn.shape[0], _ptr(nn), _ptr(cd), _ptr(losses)))
        return losses

    def screen_candidates(self, n_candidates, n_keep, gen):
        """Screening with the selection on the device: gen(first, count) -> (nn (count, P), cond (count, N)) is asked
        for one chunk at a time; returns (indices, losses, nn (n_keep, P), cond (n_keep, N)) of the n_keep best
        candidates in increasing order of loss (ties: lower index first, as partialsortperm)."""
        P, N = self.P, self.N

        def thunk(first, count, nn_p, cond_p, _user):
            try:
                nn, cond = gen(int(first), int(count))
                np.ctypeslib.as_array(nn_p, shape=(count, P))[:] = nn
                np.ctypeslib.as_array(cond_p, shape=(count, N))[:] = cond
                return 0
            except Exception:      # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1
        cb = _CANDIDATES(thunk)
        n_keep = min(int(n_keep), int(n_candidates))
        idx, loss = np.empty(n_keep, dtype=np.int64), np.empty(n_keep)
        nn_out, cond_out = np.empty((n_keep, P)), np.empty((n_keep, N))
        check(self._lib.cude_screen_candidates(self._h, int(n_candidates), n_keep, C.cast(cb, C.c_void_p), None,
                                               _ptr(idx), _ptr(loss), _ptr(nn_out), _ptr(cond_out)))
        return idx, loss, nn_out, cond_out

    def multistart_loss_grad(self, nn_sets, cond_sets):
        """Loss and gradient of K parameter sets in one launch (restarts trained side by side).
        nn_sets: (K, P); cond_sets: (K, N) -> losses (K,), g_nn (K, P), g_cond (K, N)."""
        nn = _f64(nn_sets)
        cd = _f64(cond_sets)
        if nn.ndim != 2 or nn.shape[1] != self.P or cd.shape != (nn.shape[0], self.N):
            raise ValueError(f"expected nn_sets (K, {self.P}) and cond_sets (K, {self.N})")
        K = nn.shape[0]
        losses, g_nn, g_cond = np.empty(K), np.empty((K, self.P)), np.empty((K, self.N))
        check(self._lib.cude_multistart_loss_grad(self._h, K, _ptr(nn), _ptr(cd), _ptr(losses), _ptr(g_nn),
                                                  _ptr(g_cond)))
        return losses, g_nn, g_cond

    def mh_estep(self, normals, uniforms, sigma, prior_mean, prior_sd, proposal_std, temperature=1.0, gamma=1.0,
                 n_mc=None):
        """n_mc Metropolis-Hastings steps for every subject on the device (chain state = the context's
        conditional parameters, updated in place).  normals/uniforms: (n_mc, N) host draws, or both None with n_mc
        given: the draws come from the device-side generator (set_rng).  Returns acceptance counts."""
        acc = np.zeros(self.N, dtype=np.int64)
        if normals is None and uniforms is None:
            if n_mc is None:
                raise ValueError("n_mc is required when the draws are generated on the device")
            z = u = None
            steps = int(n_mc)
        else:
            z = _f64(normals)
            u = _f64(uniforms)
            if z.ndim != 2 or z.shape[1] != self.N or u.shape != z.shape:
                raise ValueError(f"expected draws of shape (n_mc, {self.N})")
            steps = z.shape[0]
        check(self._lib.cude_mh_estep(self._h, steps, _ptr(z), _ptr(u), float(sigma), float(prior_mean),
                                      float(prior_sd), float(proposal_std), float(temperature), float(gamma),
                                      _ptr(acc)))
        return acc

    def set_param_mask(self, mask):
        """Freeze shared parameters: network-gradient entries are multiplied by mask (P entries of 0 / 1; None lifts
        it), so frozen entries keep their value under every optimiser of the library."""
        m = None if mask is None else _f64(mask).reshape(-1)
        if m is not None and m.size != self.P:
            raise ValueError(f"expected a mask of {self.P} entries")
        check(self._lib.cude_set_param_mask(self._h, _ptr(m)))

    def set_rng(self, seed, subject_offset=0):
        """Seed / rewind the device-side draws of mh_estep / mh_chain; subject_offset = global index of this
        context's first subject (draws do not depend on the sharding)."""
        check(self._lib.cude_set_rng(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(subject_offset)))

    def rng_draws(self, first_step, n_steps):
        """(normals, uniforms), each (n_steps, N): the draws steps first_step ... of the device stream use."""
        z = np.empty((int(n_steps), self.N))
        u = np.empty((int(n_steps), self.N))
        check(self._lib.cude_rng_draws(self._h, int(first_step), int(n_steps), _ptr(z), _ptr(u)))
        return z, u

    def train_restarts(self, nn_sets, cond_sets, adam_iters, learning_rate, lbfgs_iters, want_trace=False):
        """K restarts trained side by side inside the library (Adam, then L-BFGS + BackTracking in lock step):
        nn_sets (K, P), cond_sets (K, N) -> trained (nn (K, P), cond (K, N), objective (K,); +Inf = dropped)
        [, loss trace (K, adam_iters + lbfgs_iters), NaN after a run stopped]."""
        nn = _f64(nn_sets)
        cd = _f64(cond_sets)
        if nn.ndim != 2 or nn.shape[1] != self.P or cd.shape != (nn.shape[0], self.N):
            raise ValueError(f"expected nn_sets (K, {self.P}) and cond_sets (K, {self.N})")
        K = nn.shape[0]
        nn_out, cond_out, obj = np.empty_like(nn), np.empty_like(cd), np.empty(K)
        trace = np.empty((K, int(adam_iters) + int(lbfgs_iters))) if want_trace else None
        check(self._lib.cude_train_restarts(self._h, K, _ptr(nn), _ptr(cd), int(adam_iters), float(learning_rate),
                                            int(lbfgs_iters), _ptr(nn_out), _ptr(cond_out), _ptr(obj), _ptr(trace)))
        return (nn_out, cond_out, obj, trace) if want_trace else (nn_out, cond_out, obj)

    def profile_conditional(self, values):
        """SSE of every subject at every scan value of the conditional parameter (shared parameters frozen), all in
        one launch: values (K,) -> (K, N)."""
        v = _f64(values).reshape(-1)
        out = np.empty((v.size, self.N))
        check(self._lib.cude_profile_conditional(self._h, v.size, _ptr(v), _ptr(out)))
        return out

    def profile_intervals(self, values, center=None, delta=0.0, *, delta_per_subject=None, penalty_weight=0.0,
                          penalty_center=0.0, rounds=0, sections=3, argmin_only=False):
        """Per-subject profile-likelihood intervals with the profile kept on the device (cude_profile_intervals): the scan
        over `values` (K,) is reduced there chunk by chunk, `rounds` sectioning rounds with `sections` interior points
        per end then tighten both ends.  center (N,) -- None: the context's conditional parameters; the threshold of
        subject i is F_i(center_i) + delta (or delta_per_subject[i]), in SSE units.  Returns dict(lower, upper, argmin,
        min, center_objective (N,) doubles; n_inside, status (N,) int32, status = CI_* bits).  argmin_only: dict(argmin,
        min) of the scan alone -- no centre solve, no threshold."""
        v = _f64(values).reshape(-1)
        cen = None if center is None else np.ascontiguousarray(np.broadcast_to(_f64(center), (self.N,)))
        dps = None if delta_per_subject is None else np.ascontiguousarray(np.broadcast_to(_f64(delta_per_subject), (self.N,)))
        out = {k: np.empty(self.N) for k in (("argmin", "min") if argmin_only else
                                             ("lower", "upper", "argmin", "min", "center_objective"))}
        if not argmin_only:
            out["n_inside"], out["status"] = np.empty(self.N, dtype=np.int32), np.empty(self.N, dtype=np.int32)
        check(self._lib.cude_profile_intervals(
            self._h, v.size, _ptr(v), _ptr(cen), float(delta), _ptr(dps), float(penalty_weight), float(penalty_center),
            int(rounds), int(sections), _ptr(out.get("lower")), _ptr(out.get("upper")), _ptr(out["argmin"]),
            _ptr(out["min"]), _ptr(out.get("center_objective")), _ptr(out.get("n_inside")), _ptr(out.get("status"))))
        return out

    def predictive_bands(self, cond_sets, times, ranks, state=0, want_mean=True):
        """Posterior-predictive bands on the device (cude_predictive_bands): cond_sets (K, N) -- the rows of mh_chain's
        samples -- are solved as simulate(times) solves the context's own conditional parameters, and every (subject,
        time) column of state `state` is reduced there to its order statistics `ranks` (strictly increasing, 0-based) and
        its mean over the sets in set order.  Returns dict(order (N, n_times, n_ranks) -- None without ranks --, mean
        (N, n_times) -- None unless want_mean --, bad_sets (N,) int32: sets with a non-finite value).  A column with a
        non-finite value is NaN throughout; n_failed() afterwards counts the subjects with bad_sets > 0."""
        cd = _f64(cond_sets)
        if cd.ndim != 2 or cd.shape[1] != self.N:
            raise ValueError(f"expected cond_sets (K, {self.N})")
        t = _f64(times).reshape(-1)
        rk = np.ascontiguousarray(np.asarray(ranks, dtype=np.int32).reshape(-1))
        order = np.empty((self.N, t.size, rk.size)) if rk.size else None
        mean = np.empty((self.N, t.size)) if want_mean else None
        bad = np.empty(self.N, dtype=np.int32)
        check(self._lib.cude_predictive_bands(self._h, cd.shape[0], _ptr(cd), t.size, _ptr(t), int(state), rk.size,
                                              _ptr(rk) if rk.size else None, _ptr(order), _ptr(mean), _ptr(bad)))
        return {"order": order, "mean": mean, "bad_sets": bad}

    def evaluate_conditional_sets(self, cond_sets, penalty_weight=0.0, penalty_center=0.0, want_sse=False):
        """SSE_i(cond_sets[k, i]) + penalty_weight (cond_sets[k, i] - penalty_center)^2 for every set and subject
        (cude_evaluate_conditional_sets; cond_sets (K, N)), reduced on the device to the per-subject minimum: dict(index (N,)
        int32 = the first set that attains it, objective (N,) -- +Inf and index 0 with no finite value --, sse (K, N) -- None
        unless want_sse)."""
        cd = _f64(cond_sets)
        if cd.ndim != 2 or cd.shape[1] != self.N:
            raise ValueError(f"expected cond_sets (K, {self.N})")
        sse = np.empty(cd.shape) if want_sse else None
        idx, obj = np.empty(self.N, dtype=np.int32), np.empty(self.N)
        check(self._lib.cude_evaluate_conditional_sets(self._h, cd.shape[0], _ptr(cd), float(penalty_weight),
                                                       float(penalty_center), _ptr(sse), _ptr(idx), _ptr(obj)))
        return {"index": idx, "objective": obj, "sse": sse}

    def marginal_likelihood(self, sigma, prior_mean=0.0, prior_sd=np.inf, *, nodes=None, log_weights=None, n_draws=None,
                            first_step=0, center=None, scale=None, want_points=False, want_terms=False):
        """Per-subject marginal log-likelihoods on the device (cude_marginal_likelihood): log of the integral over the
        random effect of exp(log-likelihood + log prior), by the rule (nodes, log_weights) (K,) at x = center + scale *
        nodes, or -- nodes and log_weights None, n_draws = K -- by self-normalised importance sampling from
        Normal(center, scale^2) with the device stream's normals of steps first_step ... (rng_draws' bits; the stream
        position is left alone).  center (N,) -- None: the context's conditional parameters; scale (N,) -- None: 1.
        Returns dict(logml, post_mean, post_var, post_sse, ess (N,) doubles; n_bad (N,) int32; points, terms (K, N) --
        None unless wanted).  A subject with no finite term: logml -Inf, the moments NaN, counted by n_failed()."""
        z = None if nodes is None else _f64(nodes).reshape(-1)
        a = None if log_weights is None else _f64(log_weights).reshape(-1)
        if z is None and a is None:
            if n_draws is None:
                raise ValueError("n_draws is required when the points are drawn on the device")
            K = int(n_draws)
        else:                                   # (one of the two alone: the library's CUDE_ERR_ARG)
            if z is not None and a is not None and z.size != a.size:
                raise ValueError("nodes and log_weights differ in length")
            K = (z if z is not None else a).size
        cen = None if center is None else np.ascontiguousarray(np.broadcast_to(_f64(center), (self.N,)))
        scl = None if scale is None else np.ascontiguousarray(np.broadcast_to(_f64(scale), (self.N,)))
        out = {k: np.empty(self.N) for k in ("logml", "post_mean", "post_var", "post_sse", "ess")}
        out["n_bad"] = np.empty(self.N, dtype=np.int32)
        rows = max(K, 0)
        out["points"] = np.empty((rows, self.N)) if want_points else None
        out["terms"] = np.empty((rows, self.N)) if want_terms else None
        check(self._lib.cude_marginal_likelihood(
            self._h, K, _ptr(z), _ptr(a), int(first_step), _ptr(cen), _ptr(scl), float(sigma), float(prior_mean),
            float(prior_sd), _ptr(out["logml"]), _ptr(out["post_mean"]), _ptr(out["post_var"]), _ptr(out["post_sse"]),
            _ptr(out["ess"]), _ptr(out["n_bad"]), _ptr(out["points"]), _ptr(out["terms"])))
        return out

    def subject_scores(self, cond_sets=None, weights=None, want=("scores", "wsse", "bad", "sum", "cross")):
        """Per-subject scores of the shared parameters on the device (cude_subject_scores): s_i = sum_k w_ik d SSE_i(x_ik) /
        d theta in set order, with cond_sets (K, N) -- None: the context's conditional parameters, one set -- and weights
        (K, N) -- None: 1; a set with weight 0 is skipped for that subject.  Returns dict(scores (N, P), wsse (N,), bad
        (N,) int32 = sets with weight whose SSE or row was not finite, sum (P,), cross (P, P)), None for what `want`
        leaves out.  A failed subject (bad > 0) has a NaN row and wsse, is left out of sum and cross, and is counted by
        n_failed() afterwards."""
        cd = None if cond_sets is None else _f64(cond_sets)
        w = None if weights is None else _f64(weights)
        if cd is not None and (cd.ndim != 2 or cd.shape[1] != self.N):
            raise ValueError(f"expected cond_sets (K, {self.N})")
        K = cd.shape[0] if cd is not None else (w.shape[0] if w is not None and w.ndim == 2 else 1)
        if w is not None and w.shape != (K, self.N):
            raise ValueError(f"expected weights ({K}, {self.N})")
        unknown = set(want) - {"scores", "wsse", "bad", "sum", "cross"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        P = self.P
        out = {"scores": np.empty((self.N, P)) if "scores" in want else None,
               "wsse": np.empty(self.N) if "wsse" in want else None,
               "bad": np.empty(self.N, dtype=np.int32) if "bad" in want else None,
               "sum": np.empty(P) if "sum" in want else None,
               "cross": np.empty((P, P)) if "cross" in want else None}
        check(self._lib.cude_subject_scores(self._h, K, _ptr(cd), _ptr(w), _ptr(out["scores"]), _ptr(out["wsse"]),
                                            _ptr(out["bad"]), _ptr(out["sum"]), _ptr(out["cross"])))
        return out

    @property
    def n_outputs(self):
        """Outputs per subject of network_information (cude_n_outputs): T for the c-peptide models, 3 T for suppression."""
        n = C.c_int32()
        check(self._lib.cude_n_outputs(self._h, C.byref(n)))
        return n.value

    INFO_OUTPUTS = ("jac", "jcond", "gn", "coupling", "dcond", "schur", "qform", "status")

    def network_information(self, cond=None, penalty_weight=0.0, cov=None, profiled=False,
                            want=("gn", "coupling", "dcond", "schur", "status")):
        """Output Jacobians with respect to the shared parameters and the expected-information matrices on the device
        (cude_network_information): cond (N,) -- None: the context's conditional parameters.  Returns dict(jac (N, n_out, P)
        = d yhat_io / d theta, jcond (N, n_out) = d yhat_io / d cond_i, gn (P, P) = A, coupling (N, P) = b_i, dcond (N,) =
        d_i, schur (P, P) = A - sum_i b_i b_i^T / (d_i + penalty_weight), qform (N, n_out) = z cov z^T (needs cov; z = J_io
        - jc_io / (d_i + pw) b_i when profiled, J_io otherwise), status (N,) int32: bit 1 failed, bit 2 flat), None for
        what `want` leaves out.  A failed subject has NaN rows, is left out of gn and schur, and is counted by n_failed()
        afterwards."""
        unknown = set(want) - set(self.INFO_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        cd = None if cond is None else _f64(cond).reshape(-1)
        if cd is not None and cd.size != self.N:
            raise ValueError(f"expected cond ({self.N},)")
        P, N = self.P, self.N
        cv = None if cov is None else _f64(cov)
        if cv is not None and cv.shape != (P, P):
            raise ValueError(f"expected cov ({P}, {P})")
        n_out = self.n_outputs
        shapes = {"jac": (N, n_out, P), "jcond": (N, n_out), "gn": (P, P), "coupling": (N, P), "dcond": (N,),
                  "schur": (P, P), "qform": (N, n_out), "status": (N,)}
        out = {k: (np.empty(shapes[k], dtype=np.int32 if k == "status" else np.float64) if k in want else None)
               for k in self.INFO_OUTPUTS}
        check(self._lib.cude_network_information(self._h, _ptr(cd), float(penalty_weight), _ptr(cv), 1 if profiled else 0,
                                                 _ptr(out["jac"]), _ptr(out["jcond"]), _ptr(out["gn"]),
                                                 _ptr(out["coupling"]), _ptr(out["dcond"]), _ptr(out["schur"]),
                                                 _ptr(out["qform"]), _ptr(out["status"])))
        return out

    def lm_candidates(self, mu):
        """Levenberg-Marquardt steps at the context's parameters for the dampings mu (1 ... 8 of them) and their trial
        losses in one multi-set forward launch (cude_lm_candidates): dict(nn (K, P) = theta + dtheta_k, cond (K, N) = c +
        dc^k, pred (K,) the predicted reduction of N loss, loss (K,) = multistart_forward at those sets, dnn (K, P) and dcond
        (K, N) the steps themselves).  An invalid
        candidate (a pivot of the damped Schur complement not > 0, a failed subject) is NaN throughout.  The context's
        parameters are untouched."""
        m = _f64(mu).reshape(-1)
        K = m.size
        nn, cond, pred, loss = np.empty((K, self.P)), np.empty((K, self.N)), np.empty(K), np.empty(K)
        dnn, dcond = np.empty((K, self.P)), np.empty((K, self.N))
        check(self._lib.cude_lm_candidates(self._h, K, _ptr(m), _ptr(nn), _ptr(cond), _ptr(pred), _ptr(loss), _ptr(dnn),
                                           _ptr(dcond)))
        return {"nn": nn, "cond": cond, "pred": pred, "loss": loss, "dnn": dnn, "dcond": dcond}

    def train_lm(self, max_iters=50, n_trials=4, mu0=1e-2, gtol=0.0, ftol=0.0):
        """Levenberg-Marquardt on the context's parameters (cude_train_lm), which hold the result afterwards: dict(trace
        (n_iters + 1,) = forward()'s loss at the start and after every iteration, mu (n_iters + 1,), n_iters, status =
        LM_GRAD | LM_DECREASE | LM_STALLED | LM_MAX_ITERS | LM_FAILED)."""
        trace, mus = np.full(int(max_iters) + 1, np.nan), np.full(int(max_iters) + 1, np.nan)
        n, st = C.c_int32(), C.c_int32()
        check(self._lib.cude_train_lm(self._h, int(max_iters), int(n_trials), float(mu0), float(gtol), float(ftol),
                                      _ptr(trace), _ptr(mus), C.byref(n), C.byref(st)))
        return {"trace": trace[:n.value + 1], "mu": mus[:n.value + 1], "n_iters": n.value, "status": st.value}

    def fit_conditional(self, lower, upper, n_grid=41, n_iters=48, penalty_weight=0.0, penalty_center=0.0):
        """All subjects' 1-D fits of the conditional parameter with the shared parameters frozen, on the device:
        argmin_x SSE_i(x) + penalty_weight (x - penalty_center)^2 over [lower, upper] -> (x[N], objective[N], sse[N])."""
        x, obj, sse = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        check(self._lib.cude_fit_conditional(self._h, float(lower), float(upper), int(n_grid), int(n_iters),
                                             float(penalty_weight), float(penalty_center), _ptr(x), _ptr(obj),
                                             _ptr(sse)))
        return x, obj, sse

    def refine_conditional(self, x0=None, lower=-4.0, upper=3.0, max_evals=40, xtol=1e-7, max_step=0.5,
                           penalty_weight=0.0, penalty_center=0.0):
        """The same problems by the Newton-type iteration of cude_refine_conditional from the starts x0 (N,) -- None:
        the context's conditional parameters -- in one launch (fixed-step mode): dict(x, objective, sse, info (N,)
        doubles; evals, status (N,) int32, status = REFINE_*).  A failed subject keeps its clamped start, objective +Inf."""
        if x0 is not None:
            x0 = np.ascontiguousarray(np.broadcast_to(_f64(x0), (self.N,)))
        x, obj, sse, info = np.empty(self.N), np.empty(self.N), np.empty(self.N), np.empty(self.N)
        evals, status = np.empty(self.N, dtype=np.int32), np.empty(self.N, dtype=np.int32)
        check(self._lib.cude_refine_conditional(self._h, _ptr(x0), float(lower), float(upper), int(max_evals),
                                                float(xtol), float(max_step), float(penalty_weight),
                                                float(penalty_center), _ptr(x), _ptr(obj), _ptr(sse), _ptr(info),
                                                _ptr(evals), _ptr(status)))
        return {"x": x, "objective": obj, "sse": sse, "info": info, "evals": evals, "status": status}

    def _residual_rows(self):
        return self.T if self.model != MODEL_SUPP else 3 * self.T

    def bootstrap_conditional(self, sigma, n_reps, center=None, *, ranks=(), noise=None, first_rep=0, lower=-4.0, upper=3.0,
                              max_evals=40, xtol=1e-7, max_step=0.5, penalty_weight=0.0, penalty_center=0.0,
                              want_replicates=False):
        """Parametric bootstrap of the per-subject fits on the device (cude_bootstrap_conditional): n_reps replicate data
        sets per subject -- forward(want_traj=True) at `center` (N,; None: the context's conditional parameters) plus
        sigma (N,) times the state's scale times standard normals -- each refitted by refine_conditional's rule from the
        centre.  noise (n_reps, rows, N), rows = T (c-peptide models) or 3 T in (3, T, N) order (suppression); None: the
        device stream of set_rng at replicates first_rep ... (bootstrap_noise returns those draws).  Returns dict(order
        (len(ranks), N) -- None without ranks --, mean, sd (N,), n_used (N,) int32 [, replicates (n_reps, N), status
        (n_reps, N) int32 = REFINE_*]): summaries over a subject's non-FAILED replicates, NaN where there are too few."""
        B = int(n_reps)
        sg = np.ascontiguousarray(np.broadcast_to(_f64(sigma), (self.N,)))
        cen = None if center is None else np.ascontiguousarray(np.broadcast_to(_f64(center), (self.N,)))
        nz = None
        if noise is not None:
            nz = _f64(noise)
            if nz.shape != (B, self._residual_rows(), self.N):
                raise ValueError(f"expected noise ({B}, {self._residual_rows()}, {self.N})")
        rk = np.ascontiguousarray(np.asarray(ranks, dtype=np.int32).reshape(-1))
        order = np.empty((rk.size, self.N)) if rk.size else None
        mean, sd, used = np.empty(self.N), np.empty(self.N), np.empty(self.N, dtype=np.int32)
        reps = np.empty((B, self.N)) if want_replicates else None
        status = np.empty((B, self.N), dtype=np.int32) if want_replicates else None
        check(self._lib.cude_bootstrap_conditional(
            self._h, _ptr(cen), _ptr(sg), int(first_rep), B, _ptr(nz), float(lower), float(upper), int(max_evals),
            float(xtol), float(max_step), float(penalty_weight), float(penalty_center), rk.size,
            _ptr(rk) if rk.size else None, _ptr(order), _ptr(mean), _ptr(sd), _ptr(used), _ptr(reps), _ptr(status)))
        out = {"order": order, "mean": mean, "sd": sd, "n_used": used}
        if want_replicates:
            out["replicates"], out["status"] = reps, status
        return out

    def bootstrap_noise(self, first_rep, n_reps):
        """The standard normals bootstrap_conditional(noise=None, first_rep=first_rep) draws: (n_reps, rows, N), +0.0 in the
        rows of t_0."""
        z = np.empty((int(n_reps), self._residual_rows(), self.N))
        check(self._lib.cude_bootstrap_noise(self._h, int(first_rep), int(n_reps), _ptr(z)))
        return z

    def npde(self, sigma, n_sims, cond_sets=None, *, prior_mean=0.0, prior_sd=1.0, noise=None, first_rep=0, state=0,
             want_decorrelated=True, want_sims=False):
        """Prediction discrepancies and npde per subject on the device (cude_npde): n_sims simulated data sets per subject --
        simulate(timepoints) at cond_sets (n_sims, N), or at prior_mean + prior_sd z with z of the device stream of set_rng
        (None), plus sigma (N,) times the state's scale times standard normals -- against the population's observations of
        state `state` at the R = T - 1 data times after t_0.  noise (n_sims, R, N), or None: the device stream at replicates
        first_rep ... (npde_draws returns both kinds of draws).  Returns dict(pred_mean, pred_var, pd (R, N), below (R, N)
        int32, n_used, status (N,) int32 = NPDE_* bits [, npde (R, N), below_decorr (R, N) int32] [, sims (n_sims, R, N)])."""
        K, R = int(n_sims), self.T - 1
        sg = np.ascontiguousarray(np.broadcast_to(_f64(sigma), (self.N,)))
        cd = None
        if cond_sets is not None:
            cd = _f64(cond_sets)
            if cd.shape != (K, self.N):
                raise ValueError(f"expected cond_sets ({K}, {self.N})")
        nz = None
        if noise is not None:
            nz = _f64(noise)
            if nz.shape != (K, R, self.N):
                raise ValueError(f"expected noise ({K}, {R}, {self.N})")
        out = {"pred_mean": np.empty((R, self.N)), "pred_var": np.empty((R, self.N)), "pd": np.empty((R, self.N)),
               "below": np.empty((R, self.N), dtype=np.int32), "n_used": np.empty(self.N, dtype=np.int32),
               "status": np.empty(self.N, dtype=np.int32)}
        if want_decorrelated:
            out["npde"], out["below_decorr"] = np.empty((R, self.N)), np.empty((R, self.N), dtype=np.int32)
        if want_sims:
            out["sims"] = np.empty((K, R, self.N))
        check(self._lib.cude_npde(
            self._h, K, _ptr(cd), float(prior_mean), float(prior_sd), _ptr(sg), int(first_rep), _ptr(nz), int(state),
            _ptr(out["pred_mean"]), _ptr(out["pred_var"]), _ptr(out["below"]), _ptr(out.get("below_decorr")), _ptr(out["pd"]),
            _ptr(out.get("npde")), _ptr(out["n_used"]), _ptr(out["status"]), _ptr(out.get("sims"))))
        return out

    def npde_draws(self, first_rep, n_sims):
        """The standard normals npde(cond_sets=None, noise=None, first_rep=first_rep) draws: (eta_normals (n_sims, N), noise
        (n_sims, T - 1, N))."""
        z, eps = np.empty((int(n_sims), self.N)), np.empty((int(n_sims), self.T - 1, self.N))
        check(self._lib.cude_npde_draws(self._h, int(first_rep), int(n_sims), _ptr(z), _ptr(eps)))
        return z, eps

    def vpc(self, sigma, n_sims, cond_sets=None, *, prior_mean=0.0, prior_sd=1.0, noise=None, first_rep=0, state=0,
            groups=None, n_groups=None, levels=(0.05, 0.5, 0.95), ci_levels=(0.025, 0.5, 0.975), want_sim_q=True):
        """Visual predictive check by subject group on the device (cude_vpc): n_sims data sets simulated as npde simulates
        them (the same arguments, the same bits); inside each group (groups (N,) int ids in [0, n_groups), negative = left
        out; None: one group) the type-7 quantiles across subjects at `levels` of every simulated data set and of the
        observations at every data time after t_0, then the quantiles at `ci_levels` across the simulations.  Returns
        dict(observed (G, R, L), simulated_ci (G, R, L, C) [, simulated_q (n_sims, G, R, L)], n_members, n_sims_used (G,)
        int32, status (N,) int32 = VPC_* bits)."""
        K, R = int(n_sims), self.T - 1
        sg = np.ascontiguousarray(np.broadcast_to(_f64(sigma), (self.N,)))
        cd = None
        if cond_sets is not None:
            cd = _f64(cond_sets)
            if cd.shape != (K, self.N):
                raise ValueError(f"expected cond_sets ({K}, {self.N})")
        nz = None
        if noise is not None:
            nz = _f64(noise)
            if nz.shape != (K, R, self.N):
                raise ValueError(f"expected noise ({K}, {R}, {self.N})")
        gr = None
        if groups is not None:
            gr = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(-1))
            if gr.shape != (self.N,):
                raise ValueError(f"expected groups ({self.N},)")
        G = int(n_groups) if n_groups is not None else (1 if gr is None else max(1, int(gr.max()) + 1))
        lv, cv = _f64(levels).reshape(-1), _f64(ci_levels).reshape(-1)
        L, C_ = lv.size, cv.size
        out = {"observed": np.empty((G, R, L)), "simulated_ci": np.empty((G, R, L, C_)),
               "n_members": np.empty(G, dtype=np.int32), "n_sims_used": np.empty(G, dtype=np.int32),
               "status": np.empty(self.N, dtype=np.int32)}
        if want_sim_q:
            out["simulated_q"] = np.empty((K, G, R, L))
        check(self._lib.cude_vpc(
            self._h, K, _ptr(cd), float(prior_mean), float(prior_sd), _ptr(sg), int(first_rep), _ptr(nz), int(state),
            G, _ptr(gr), L, _ptr(lv), C_, _ptr(cv), _ptr(out["observed"]), _ptr(out["simulated_ci"]),
            _ptr(out.get("simulated_q")), _ptr(out["n_members"]), _ptr(out["n_sims_used"]), _ptr(out["status"])))
        return out

    def mh_chain(self, normals, uniforms, sigma, prior_mean, prior_sd, proposal_std, temperature=1.0, gamma=1.0,
                 n_mc=None):
        """mh_estep that also returns every state of the chain: (accepted (N,), samples (n_mc, N)).  normals =
        uniforms = None with n_mc given: device-side draws."""
        if normals is None and uniforms is None:
            if n_mc is None:
                raise ValueError("n_mc is required when the draws are generated on the device")
            z = u = None
            shape = (int(n_mc), self.N)
        else:
            z = _f64(normals)
            u = _f64(uniforms)
            if z.ndim != 2 or z.shape[1] != self.N or u.shape != z.shape:
                raise ValueError(f"expected draws of shape (n_mc, {self.N})")
            shape = z.shape
        acc = np.zeros(self.N, dtype=np.int64)
        samples = np.empty(shape)
        check(self._lib.cude_mh_chain(self._h, shape[0], _ptr(z), _ptr(u), float(sigma), float(prior_mean),
                                      float(prior_sd), float(proposal_std), float(temperature), float(gamma),
                                      _ptr(acc), _ptr(samples)))
        return acc, samples

    def loss_grad(self, want_cond_grad=True):
        loss = C.c_double()
        g_nn = np.empty(self.P)
        g_cond = np.empty(self.N) if want_cond_grad else None
        check(self._lib.cude_loss_grad(self._h, C.byref(loss), _ptr(g_nn), _ptr(g_cond)))
        return loss.value, g_nn, g_cond

    def n_failed(self):
        n = C.c_int64()
        check(self._lib.cude_n_failed(self._h, C.byref(n)))
        return n.value

    # -- optimiser
    def adam_init(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        check(self._lib.cude_adam_init(self._h, lr, beta1, beta2, eps))

    def adam_step(self, want_loss=True):
        if want_loss:
            loss = C.c_double()
            check(self._lib.cude_adam_step(self._h, C.byref(loss)))
            return loss.value
        check(self._lib.cude_adam_step(self._h, None))
        return None

    def adam_run(self, n_iters):
        """n_iters fused optimiser iterations with one synchronisation (hipGraph replay); returns the loss
        before each update."""
        losses = np.empty(int(n_iters))
        check(self._lib.cude_adam_run(self._h, int(n_iters), _ptr(losses)))
        return losses

    # -- bring-your-own collective
    def set_global_subjects(self, n_global, scale=None):
        sc = None if scale is None else _f64(scale)
        check(self._lib.cude_set_global_subjects(self._h, float(n_global), _ptr(sc)))

    def get_scale(self):
        sc = np.empty(3)
        n = C.c_double()
        check(self._lib.cude_get_scale(self._h, _ptr(sc), C.byref(n)))
        return sc, n.value

    def loss_grad_partial(self, want_cond_grad=False):
        """This rank's un-reduced [g_nn; sum sse; n_failed] (and optionally dL/dcond of its subjects)."""
        part = np.empty(self.P + 2)
        g_cond = np.empty(self.N) if want_cond_grad else None
        check(self._lib.cude_loss_grad_partial(self._h, _ptr(part), _ptr(g_cond)))
        return part, g_cond

    def adam_apply(self, reduced):
        r = _f64(reduced)
        loss = C.c_double()
        check(self._lib.cude_adam_apply(self._h, _ptr(r), C.byref(loss)))
        return loss.value

    # -- the same exchange without the host round trip (a collective that reduces device memory in place)
    def partial_buffer(self):
        """(device address, count = P + 2) of the context's [g_nn; sum sse; n_failed] vector."""
        ptr, n = C.c_void_p(), C.c_int32()
        check(self._lib.cude_partial_buffer(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def partial_tensor(self, torch, device):
        """A torch tensor ALIASING that vector (no copy): torch.distributed.all_reduce on it reduces in place."""
        ptr, n = self.partial_buffer()

        class _Alias:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 3,
                                        "strides": None}
        return torch.as_tensor(_Alias(), device=device)

    def loss_grad_partial_device(self):
        check(self._lib.cude_loss_grad_partial_device(self._h))

    def adam_apply_device(self):
        loss = C.c_double()
        check(self._lib.cude_adam_apply_device(self._h, C.byref(loss)))
        return loss.value

    def synchronize(self):
        check(self._lib.cude_synchronize(self._h))

    def adaptive_regroup(self):
        """Adaptive mode: order the launch by the accepted-step counts of the last gradient evaluation so that a wave's
        lanes finish together.  Returns (mean max - min steps within a wave before, after)."""
        b, a = C.c_int32(), C.c_int32()
        check(self._lib.cude_adaptive_regroup(self._h, C.byref(b), C.byref(a)))
        return b.value, a.value

    def grad_occupancy(self):
        """Resident waves per CU the runtime grants the one-lane gradient kernel of this context."""
        n = C.c_int32()
        check(self._lib.cude_grad_occupancy(self._h, C.byref(n)))
        return n.value

    def set_kernel_timing(self, enabled):
        """True / 1: HIP events around every ensemble launch; n > 1: around every n-th; False / 0: off."""
        check(self._lib.cude_set_kernel_timing(self._h, int(enabled)))

    def kernel_time_ms(self):
        ms = C.c_double()
        n = C.c_int64()
        check(self._lib.cude_kernel_time_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_time_stats(self):
        """(mean, median, minimum in ms, launches timed) of the dominant kernel since the last query (cude_kernel_time_stats)."""
        ms, med, mn = C.c_double(), C.c_double(), C.c_double()
        n = C.c_int64()
        check(self._lib.cude_kernel_time_stats(self._h, C.byref(ms), C.byref(med), C.byref(mn), C.byref(n)))
        return ms.value, med.value, mn.value, n.value

    # -- communicator
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES)()
        check(_lib.load().cude_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, n_ranks, rank, unique_id):
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        check(self._lib.cude_comm_init(self._h, n_ranks, rank, buf))

    def comm_info(self):
        """(ranks, rank, rccl version) as the attached communicator reports them; (1, 0, 0) without one."""
        n, r, v = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._lib.cude_comm_info(self._h, C.byref(n), C.byref(r), C.byref(v)))
        return n.value, r.value, v.value

    def allreduce_host(self, values):
        v = _f64(values).copy()
        check(self._lib.cude_comm_allreduce_host(self._h, _ptr(v), v.size))
        return v

    # -- the peer-write exchange (cude_xchg_*): multi-GPU without a collective library
    def xchg_export(self, n_ranks, rank):
        """This rank's mailbox as 128 bytes for its peers (cude_xchg_export)."""
        buf = (C.c_uint8 * _lib.XCHG_HANDLE_BYTES)()
        check(self._lib.cude_xchg_export(self._h, int(n_ranks), int(rank), buf))
        return bytes(buf)

    def xchg_attach(self, handles, timeout_s=20.0):
        """handles: the n_ranks exported handles in rank order (bytes each).  Collective: ends with a self-test."""
        blob = b"".join(handles)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        check(self._lib.cude_xchg_attach(self._h, buf, float(timeout_s)))

    def xchg_detach(self):
        """Releases the exported / attached exchange; the next xchg_export offers the next kind of mailbox memory."""
        check(self._lib.cude_xchg_detach(self._h))

    def xchg_enable(self, enabled=True):
        check(self._lib.cude_xchg_enable(self._h, 1 if enabled else 0))

    def xchg_info(self):
        """(ranks, rank, memory kind of the mailbox: 3 uncached / 1 fine-grained / 0 plain, timed-out waits so far)."""
        n, r, k, t = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self._lib.cude_xchg_info(self._h, C.byref(n), C.byref(r), C.byref(k), C.byref(t)))
        return n.value, r.value, k.value, t.value

    def set_option(self, name, value):
        """cude_set_option: run-time options of the context (include/cude.h lists them)."""
        check(self._lib.cude_set_option(self._h, str(name).encode(), str(value).encode()))


__all__ = ["Engine", "CudeError", "n_params", "device_count"]
