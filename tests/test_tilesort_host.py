"""The sorting network of csrc/cude_tilesort.h without a GPU: tile_sort_ascending's pass arithmetic -- `lo`, `up`, `ia` /
`ib` and the `x > y` exchange -- restated in numpy, one vectorised pass per (k, j) over the index space the 256 threads
cover (idx = tid + u * kTileSortThreads, u < kTileSortPairs, idx < n_pair), against np.sort at every tile geometry.

    K      1   2   3   64   65  129  257   513  1025  2049  4096
    Kp     1   2   4   64  128  256  512  1024  2048  4096  4096
    C     64  64  64   64   64   32   16     8     4     2     2        C = min(kTileSortMaxCols, kTileSortDoubles / Kp)

tile_geometry() takes the three constants from the header by regular expression; tests/test_gpu_set_reductions.py states
the same table and is held to it here, so the table the device tests walk cannot drift from the header.

Columns hold ties, both zeros, +Inf holes (a FAILED replicate's estimate in cude_bootstrap.hip) and the +Inf padding behind
K.  The comparison is on values: np.array_equal with np.sort of the column.  -0.0 == +0.0, so where both zeros stand the
result is a permutation that the values alone do not fix: there the multiset is compared (as many of each zero as went in).

When a device test of tests/test_gpu_set_reductions.py fails and this file passes, the network's index arithmetic is not the
cause: look at the kernel around it (launch attributes, barriers, the load and read-off loops)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "conditional-ude_amd", "csrc", "cude_tilesort.h")
TABLE = {1: (1, 64), 2: (2, 64), 3: (4, 64), 64: (64, 64), 65: (128, 64), 129: (256, 32), 257: (512, 16), 513: (1024, 8),
         1025: (2048, 4), 2049: (4096, 2), 4096: (4096, 2)}


def tile_constants():
    """(kTileSortThreads, kTileSortDoubles, kTileSortMaxCols) as the header states them."""
    src = open(HEADER).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
                 for name in ("kTileSortThreads", "kTileSortDoubles", "kTileSortMaxCols"))


def tile_geometry(K):
    """tile_geometry restated: (Kp, C) of a tile of K values per column."""
    _, doubles, max_cols = tile_constants()
    Kp = 1
    while Kp < K:
        Kp <<= 1
    return Kp, min(max_cols, doubles // Kp)


def tile_sort_ascending(s_v, lgC, Kp):
    """The device function on a flat tile [Kp][C] (element e of column c at e * C + c), in place."""
    threads, doubles, _ = tile_constants()
    pairs = doubles // 2 // threads                           # kTileSortPairs
    C = 1 << lgC
    n_pair = (Kp << lgC) >> 1
    idx = (np.arange(threads)[None, :] + np.arange(pairs)[:, None] * threads).ravel()
    idx = idx[idx < n_pair]
    assert idx.size == n_pair                                 # the threads' 16 pairs cover every pair of the pass
    cc, p = idx & (C - 1), idx >> lgC
    k = 2
    while k <= Kp:
        j = k >> 1
        while j >= 1:
            lo = ((p & ~(j - 1)) << 1) | (p & (j - 1))
            up = (lo & k) == 0
            ia, ib = (lo << lgC) + cc, ((lo | j) << lgC) + cc
            assert np.unique(np.concatenate([ia, ib])).size == 2 * n_pair      # a pass's pairs are disjoint
            x, y = s_v[np.where(up, ia, ib)], s_v[np.where(up, ib, ia)]
            ia, ib = np.where(up, ia, ib), np.where(up, ib, ia)
            ex = x > y
            s_v[ia[ex]], s_v[ib[ex]] = y[ex], x[ex]
            j >>= 1
        k <<= 1
    return s_v


def _tile(K, Kp, C, rng, extremes):
    """(Kp, C) doubles: K own values per column -- one decimal, so that ties abound, both zeros, +Inf holes -- and the
    +Inf padding; extremes: columns 0 and 1 (every geometry has them) are all holes and all one value."""
    v = np.round(rng.standard_normal((Kp, C)), 1)
    v[rng.random((Kp, C)) < 0.1] = 0.0
    v[rng.random((Kp, C)) < 0.1] = -0.0
    v[rng.random((Kp, C)) < 0.15] = np.inf
    if extremes:
        v[:, 0] = np.inf
        v[:, 1] = 0.5
    v[K:] = np.inf
    return v


@pytest.mark.parametrize("K", sorted(TABLE))
def test_network_sorts_every_geometry(K):
    Kp, C = tile_geometry(K)
    assert (Kp, C) == TABLE[K]
    lgC = C.bit_length() - 1
    assert 1 << lgC == C and Kp * C <= tile_constants()[1]
    rng = np.random.default_rng(K)
    for trial in range(3):
        v = _tile(K, Kp, C, rng, trial == 0)
        got = tile_sort_ascending(v.ravel().copy(), lgC, Kp).reshape(Kp, C)
        assert np.array_equal(got, np.sort(v, axis=0))
        # the zeros: a permutation, so as many -0.0 (and +0.0) per column as went in
        neg = lambda a: np.count_nonzero((a == 0.0) & np.signbit(a), axis=0)         # noqa: E731
        assert np.array_equal(neg(got), neg(v)) and np.array_equal(np.count_nonzero(got == 0.0, axis=0), np.count_nonzero(v == 0.0, axis=0))
        # what the reductions read: the first n of a column are its own finite values, +Inf behind them
        n = np.count_nonzero(np.isfinite(v), axis=0)
        assert all(np.all(np.isfinite(got[:n[c], c])) and np.all(got[n[c]:, c] == np.inf) for c in range(C))
    if K >= 3:
        assert np.count_nonzero((v[:K] == 0.0) & np.signbit(v[:K])) > 0 and np.count_nonzero(np.isinf(v[:K])) > 0


def test_restatement_is_the_headers_text():
    """The lines restated above, as the header writes them: an edit of the device function fails here until the
    restatement follows it."""
    src = open(HEADER).read()
    for line in ("const int n_pair = (Kp << lgC) >> 1;", "for (int k = 2; k <= Kp; k <<= 1) {", "for (int j = k >> 1; j >= 1; j >>= 1) {",
                 "const int idx = tid + u * kTileSortThreads;", "const int cc = idx & (C - 1), p = idx >> lgC;",
                 "const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));", "const bool up = (lo & k) == 0;",
                 "ia[u] = (lo << lgC) + cc;", "ib[u] = ((lo | j) << lgC) + cc;", "x[u] = s_v[up ? ia[u] : ib[u]];",
                 "y[u] = s_v[up ? ib[u] : ia[u]];", "if (!up) { const int t = ia[u]; ia[u] = ib[u]; ib[u] = t; }",
                 "x[u] > y[u]) { s_v[ia[u]] = y[u]; s_v[ib[u]] = x[u]; }",
                 "constexpr int kTileSortPairs = kTileSortDoubles / 2 / kTileSortThreads;",
                 "const int C = kTileSortDoubles / Kp < kTileSortMaxCols ? kTileSortDoubles / Kp : kTileSortMaxCols;"):
        assert line in src, line
    assert tile_constants() == (256, 8192, 64)


def test_read_off_index_is_the_tiles_own_width():
    """Both reductions read rank r of column cc at (r << lgC) + cc.  With the widest tile's shift (r << 6) instead, every
    narrower tile answers with another column's element or leaves the tile -- which tests/test_gpu_set_reductions.py sees at
    every K above 128 through either entry point; shown here on the sorted tile itself."""
    csrc = os.path.dirname(HEADER)
    for name in ("cude_bootstrap.hip", "cude_predictive.hip"):
        assert "s_v[(ranks[r] << lgC) + cc]" in open(os.path.join(csrc, name)).read(), name
    for K, (Kp, C) in TABLE.items():
        lgC = C.bit_length() - 1
        v = np.sort(_tile(K, Kp, C, np.random.default_rng(K), False), axis=0).ravel()
        ranks = np.unique([0, min(1, K - 1), K // 2, K - 1])
        for cc in (0, C - 1):
            right = (ranks << lgC) + cc
            assert np.array_equal(v[right], v.reshape(Kp, C)[ranks, cc])
            wrong = (ranks << 6) + cc
            assert (C == 64) == np.array_equal(wrong, right)
            if C < 64 and K > 1:
                assert wrong[-1] >= v.size or not np.array_equal(v[wrong], v[right])


def test_the_device_tests_walk_this_table():
    import test_gpu_set_reductions as sr
    assert sr.GEOMETRY == {K: tile_geometry(K) for K in sr.GEOMETRY} == TABLE
    assert {C for _, C in TABLE.values()} == {64, 32, 16, 8, 4, 2}
