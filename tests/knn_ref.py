"""Brute-force reference for the k nearest neighbours (nb_knn), numpy only.

`lattice_knn`: integer coordinates, int64 arithmetic -- every distance is exact, so the engine's rows must EQUAL it: the k smallest
candidates under (d2 ascending, then j ascending), 0xffffffff / +inf behind them.  A STABLE sort on d2 alone gives that order: equal
distances keep their ascending j.  It runs chunked over the points as neighbors_ref.py does."""
import numpy as np

from neighbors_ref import NONE, _blocks


def lattice_knn(bodies, points, k, skip0=None):
    """bodies (n, >=3), points (m, >=3): integer-valued.  skip0: point r leaves body skip0 + r out.
    Returns (index (m, k) uint32, d2 (m, k) float64)."""
    x = np.asarray(bodies)[:, :3].astype(np.int64)
    p = np.asarray(points)[:, :3].astype(np.int64)
    n, m = len(x), len(p)
    big = np.iinfo(np.int64).max
    index = np.full((m, k), NONE, np.uint32)
    d2 = np.full((m, k), np.inf)
    w = min(k, n)
    for k0, k1 in _blocks(m, n):
        d = x[None, :, :] - p[k0:k1, None, :]
        q = (d * d).sum(2)
        if skip0 is not None:
            kk = np.arange(k0, k1)
            q[kk - k0, skip0 + kk] = big
        order = np.argsort(q, axis=1, kind="stable")[:, :w]
        best = np.take_along_axis(q, order, axis=1)
        have = best != big
        index[k0:k1, :w] = np.where(have, order, NONE)
        d2[k0:k1, :w] = np.where(have, best.astype(np.float64), np.inf)
    return index, d2


def naive_knn(bodies, points, k, skip0=None):
    """The same by a plain Python loop per point (for checking lattice_knn itself at small n)."""
    index = np.full((len(points), k), NONE, np.uint32)
    d2 = np.full((len(points), k), np.inf)
    for r, p in enumerate(points):
        cand = []
        for j, b in enumerate(bodies):
            if skip0 is not None and j == skip0 + r:
                continue
            cand.append((sum((int(b[c]) - int(p[c])) ** 2 for c in range(3)), j))
        cand.sort()                                            # tuples: d2, then j
        for t, (q, j) in enumerate(cand[:k]):
            index[r, t] = j
            d2[r, t] = q
    return index, d2
