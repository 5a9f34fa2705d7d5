"""cude_profile_intervals restated in numpy from the rule's text (include/cude.h), over an evaluator ev(x (N,)) -> SSE (N,)
-- the yardstick the device path is held to bit for bit (tests/test_gpu_profile_intervals.py, where ev is the device's own
forward solve) and which tests/test_profile_intervals_host.py holds against api.find_confidence_intervals on the C oracle.

  1. F_i(x) = SSE_i(x) + pw (x - pc)^2, every operation rounded on its own; a non-finite F is above every threshold.
  2. thr_i = F_i(center_i) + d_i.  A centre whose F is not finite: CENTER_FAILED, nothing lies within the threshold.
  3. Scan over `values` (strictly increasing): minimum of F and its index (first minimum; none finite: index 0, +Inf),
     first and last index with F <= thr, their count -- chunk by chunk into a running state.
  4. lower = values[first] or -Inf if first == 0; upper = values[last] or +Inf if last == n_points - 1.
  5. `rounds` rounds of m interior points per closed end: p_j = out + (in - out) j / (m + 1); in <- the p_j nearest to out
     with F <= thr (none: in stays), out <- that point's neighbour on the out side.  Other ends ride along at values[argmin].
  6. argmin_only: minimum and argmin of the scan alone.

No quantity crosses subjects, so all subjects advance together."""
import numpy as np

LOWER_OPEN, UPPER_OPEN, DISCONNECTED, EMPTY, CENTER_FAILED, BELOW_CENTER = 1, 2, 4, 8, 16, 32


def objective(sse, x, pw=0.0, pc=0.0):
    """Rule 1, with +Inf for every non-finite value."""
    with np.errstate(all="ignore"):
        f = np.asarray(sse, dtype=np.float64) + pw * (np.asarray(x, dtype=np.float64) - pc) ** 2
    return np.where(np.isfinite(f), f, np.inf)


def empty_state(N, n_points):
    return dict(fmin=np.full(N, np.inf), imin=np.zeros(N, dtype=np.int64), first=np.full(N, n_points, dtype=np.int64),
                last=np.full(N, -1, dtype=np.int64), cnt=np.zeros(N, dtype=np.int64))


def reduce_chunk(state, F, thr, k0):
    """Rows k0 ... of the scan (F (kn, N), +Inf where not finite) behind the running state; thr None: minimum only."""
    kn, N = F.shape
    k = np.argmin(F, axis=0)                                     # first minimum of the chunk; all +Inf: 0
    f = F[k, np.arange(N)]
    better = f < state["fmin"]                                   # strict: an earlier chunk keeps a tie
    state["fmin"] = np.where(better, f, state["fmin"])
    state["imin"] = np.where(better, k0 + k, state["imin"])
    if thr is not None:
        inside = F <= thr[None, :]
        any_in = inside.any(axis=0)
        first = np.where(any_in, k0 + np.argmax(inside, axis=0), state["first"])
        last = np.where(any_in, k0 + kn - 1 - np.argmax(inside[::-1], axis=0), state["last"])
        state["first"] = np.minimum(state["first"], first)
        state["last"] = np.maximum(state["last"], last)
        state["cnt"] = state["cnt"] + inside.sum(axis=0)
    return state


def scan(values, profile, thr, pw=0.0, pc=0.0, chunk=None):
    """Rule 3 over a profile of SSEs (n_points, N), `chunk` rows at a time (None: all at once)."""
    values = np.asarray(values, dtype=np.float64)
    K, N = profile.shape
    chunk = K if not chunk else int(chunk)
    state = empty_state(N, K)
    for k0 in range(0, K, chunk):
        F = objective(profile[k0:k0 + chunk], values[k0:k0 + chunk, None], pw, pc)
        state = reduce_chunk(state, F, thr, k0)
    return state


def grid_result(values, state, fcen):
    """Rule 4 and the status bits: (lower, upper, status, brackets (lo_out, lo_in, hi_in, hi_out), NaN = no bracket)."""
    values = np.asarray(values, dtype=np.float64)
    K, N = values.size, state["fmin"].size
    first, last, cnt = state["first"], state["last"], state["cnt"]
    failed = ~(fcen < np.inf)
    some = ~failed & (cnt > 0)
    status = np.zeros(N, dtype=np.int32)
    status[failed] = CENTER_FAILED
    status[~failed & (cnt == 0)] = EMPTY
    lo_open, hi_open = some & (first == 0), some & (last == K - 1)
    status[lo_open] |= LOWER_OPEN
    status[hi_open] |= UPPER_OPEN
    status[some & (cnt != last - first + 1)] |= DISCONNECTED
    status[~failed & (state["fmin"] < fcen)] |= BELOW_CENTER
    nan = np.full(N, np.nan)
    lo_closed, hi_closed = some & ~lo_open, some & ~hi_open
    f_c, l_c = np.clip(first, 1, K - 1), np.clip(last, 0, K - 2)
    lo_in = np.where(lo_closed, values[f_c], np.where(lo_open, -np.inf, nan))
    lo_out = np.where(lo_closed, values[f_c - 1], nan)
    hi_in = np.where(hi_closed, values[l_c], np.where(hi_open, np.inf, nan))
    hi_out = np.where(hi_closed, values[l_c + 1], nan)
    return status, [lo_out, lo_in, hi_in, hi_out]


def section_round(ev, out, inn, dummy, thr, m, pw, pc):
    """One round of rule 5 for one end of every subject: the new (out, in)."""
    active = ~np.isnan(out)
    new_out, new_in, found = out.copy(), inn.copy(), np.zeros(out.size, dtype=bool)
    for j in range(1, m + 1):
        with np.errstate(all="ignore"):
            p = np.where(active, out + (inn - out) * j / (m + 1), dummy)
        F = objective(ev(p), p, pw, pc)
        hit = active & ~found & (F <= thr)
        new_in = np.where(hit, p, new_in)
        found |= hit
        new_out = np.where(active & ~found, p, new_out)
    return new_out, new_in


def intervals(ev, values, center, delta, pw=0.0, pc=0.0, rounds=0, sections=3, chunk=None, profile=None, sse_center=None,
              argmin_only=False):
    """The whole rule.  profile (n_points, N) / sse_center (N,): SSEs already evaluated (else through ev).  delta: scalar or
    (N,).  Returns dict(lower, upper, argmin, min, center_objective, n_inside, status, brackets)."""
    values = np.asarray(values, dtype=np.float64)
    if profile is None:
        N = np.asarray(center).size
        profile = np.stack([ev(np.full(N, v)) for v in values])
    N = profile.shape[1]
    if argmin_only:
        st = scan(values, profile, None, pw, pc, chunk)
        return dict(argmin=values[st["imin"]], min=st["fmin"])
    center = np.broadcast_to(np.asarray(center, dtype=np.float64), (N,))
    fcen = objective(ev(center) if sse_center is None else sse_center, center, pw, pc)
    with np.errstate(all="ignore"):
        thr = np.where(fcen < np.inf, fcen + np.broadcast_to(np.asarray(delta, dtype=np.float64), (N,)), np.nan)
    st = scan(values, profile, thr, pw, pc, chunk)
    status, (lo_out, lo_in, hi_in, hi_out) = grid_result(values, st, fcen)
    dummy = values[st["imin"]]
    for _ in range(int(rounds)):
        lo_out, lo_in = section_round(ev, lo_out, lo_in, dummy, thr, sections, pw, pc)
        hi_out, hi_in = section_round(ev, hi_out, hi_in, dummy, thr, sections, pw, pc)
    return dict(lower=lo_in, upper=hi_in, argmin=dummy, min=st["fmin"], center_objective=fcen,
                n_inside=st["cnt"].astype(np.int32), status=status, brackets=(lo_out, lo_in, hi_in, hi_out), thr=thr)


# ----------------------------------------------------------------------------- evaluations on the C oracle
def cpep_evaluator(c, n_steps=30, n_state=2, nn=None):
    """c: a case of conftest.make_cpep_case -> ev(x) = per-subject SSE of the C oracle's fixed-step solve."""
    import c_oracle as co
    nn = c["nn"] if nn is None else nn

    def ev(x):
        return co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], c["arch"], nn, np.asarray(x, dtype=np.float64),
                       n_steps, n_state, want_grad=False, covariate=(c["arch"][0] == 3))["sse"]
    return ev


def supp_evaluator(c, n_steps=30):
    import c_oracle as co

    def ev(x):
        return co.supp(c["tp"], c["data"], c["arch"], c["nn"], np.asarray(x, dtype=np.float64), 0.0, n_steps,
                       want_grad=False)["sse"]
    return ev
