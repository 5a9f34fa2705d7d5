"""The rules of cude_predictive_bands and cude_evaluate_conditional_sets (include/cude.h) restated in numpy, fed by
whatever solves the caller has: v[K, n_times, N] for the bands, sse[K, N] and x[K, N] for the best set."""
import numpy as np


def sequential_mean(v):
    """(((v[0] + v[1]) + v[2]) + ...) / K along axis 0: plain adds in set order."""
    v = np.asarray(v, dtype=np.float64)
    acc = v[0].copy()
    for k in range(1, v.shape[0]):
        acc = acc + v[k]
    return acc / v.shape[0]


def bands(v, ranks):
    """v (K, n_times, N) -> dict(order (N, n_times, n_ranks), mean (N, n_times), bad_sets (N,)): rule 2's order statistics by a
    full sort, rule 3's mean, rule 4: a column with any non-finite value is NaN throughout (decided on the values), and
    bad_sets counts the sets with a non-finite value at any time."""
    v = np.asarray(v, dtype=np.float64)
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    finite = np.isfinite(v)
    bad_col = ~finite.all(axis=0)                                   # (n_times, N)
    with np.errstate(invalid="ignore"):
        srt = np.sort(np.where(finite, v, np.inf), axis=0)
        order = srt[ranks] if ranks.size else np.empty((0,) + v.shape[1:])
        mean = sequential_mean(v)
    order = np.where(bad_col[None], np.nan, order)
    mean = np.where(bad_col, np.nan, mean)
    bad_sets = (~finite.all(axis=1)).sum(axis=0).astype(np.int32)   # (N,)
    return {"order": np.ascontiguousarray(order.transpose(2, 1, 0)), "mean": np.ascontiguousarray(mean.T),
            "bad_sets": bad_sets}


def objective(sse, x, pw=0.0, pc=0.0):
    """cude_profile_intervals rule 1: every operation rounded on its own; a non-finite F is +Inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(x, dtype=np.float64) - pc
        f = np.asarray(sse, dtype=np.float64) + pw * (t * t)
    return np.where(np.isfinite(f), f, np.inf)


def best_of_sets(sse, x, pw=0.0, pc=0.0):
    """(index (N,) int32, objective (N,)): per subject the first set (strict <) with the smallest F; no finite value:
    index 0 and +Inf."""
    f = objective(sse, x, pw, pc)
    K, N = f.shape
    best, idx = np.full(N, np.inf), np.zeros(N, dtype=np.int32)
    for k in range(K):
        better = f[k] < best
        best = np.where(better, f[k], best)
        idx = np.where(better, k, idx).astype(np.int32)
    return idx, best
