"""Brute-force references for the neighbour query (nb_neighbors), numpy only.

`lattice_ref`: integer coordinates, int64 arithmetic -- every distance is exact, so the engine's answer must EQUAL it, the smallest
index among equal distances included.  `float_ref`: float64 distances of the stored rows, for the bounds of the real distributions.
Both run chunked over the points, so the (points x bodies) block never grows past a few million entries."""
import numpy as np

NONE = 0xffffffff


def _blocks(m, n):
    step = max(1, 4000000 // max(1, n))
    for k0 in range(0, m, step):
        yield k0, min(m, k0 + step)


def lattice_ref(bodies, points, radii=None, skip0=None):
    """bodies (n, >=3), points (m, >=3): integer-valued.  radii: (m,) integers or None.  skip0: point k leaves body skip0 + k out.
    Returns (index uint32, d2 float64 (+inf where there is no candidate), count uint32 | None)."""
    x = np.asarray(bodies)[:, :3].astype(np.int64)
    p = np.asarray(points)[:, :3].astype(np.int64)
    n, m = len(x), len(p)
    big = np.iinfo(np.int64).max
    index = np.full(m, NONE, np.uint32)
    d2 = np.full(m, np.inf)
    count = None if radii is None else np.zeros(m, np.uint32)
    h2 = None if radii is None else np.asarray(radii).astype(np.int64) ** 2
    for k0, k1 in _blocks(m, n):
        d = x[None, :, :] - p[k0:k1, None, :]
        q = (d * d).sum(2)
        if skip0 is not None:
            kk = np.arange(k0, k1)
            q[kk - k0, skip0 + kk] = big
        j = q.argmin(1)                                   # the first of equal minima: the smallest j
        best = q[np.arange(k1 - k0), j]
        have = best != big
        index[k0:k1] = np.where(have, j, NONE)
        d2[k0:k1] = np.where(have, best.astype(np.float64), np.inf)
        if count is not None:
            count[k0:k1] = ((q < h2[k0:k1, None]) & (q != big)).sum(1)
    return index, d2, count


def float_ref(bodies, points, skip0=None):
    """float64 squared distances of the rows as stored.  Returns a function block(k0, k1) -> (k1 - k0, n) array with the own row of
    a skip0 point at +inf, and the point-block iterator to use with it."""
    x = np.asarray(bodies)[:, :3].astype(np.float64)
    p = np.asarray(points)[:, :3].astype(np.float64)

    def block(k0, k1):
        d = x[None, :, :] - p[k0:k1, None, :]
        q = (d * d).sum(2)
        if skip0 is not None:
            kk = np.arange(k0, k1)
            q[kk - k0, skip0 + kk] = np.inf
        return q

    return block, list(_blocks(len(p), len(x)))


def check_float(bodies, points, index, dist2, count, radii, tol, skip0=None):
    """The three bounds of the real-distribution tests; returns the worst figures (excess of d2(j*) over the minimum, error of dist2,
    and how far outside its bracket a count lies -- 0 when inside)."""
    block, blocks = float_ref(bodies, points, skip0)
    worst_nn = worst_d2 = 0.0
    worst_cnt = 0
    h2 = None if radii is None else np.asarray(radii, np.float64) ** 2
    for k0, k1 in blocks:
        q = block(k0, k1)
        rows = np.arange(k1 - k0)
        jstar = index[k0:k1].astype(np.int64)
        assert np.all(jstar < q.shape[1]), "an index past the last body"
        dmin = q.min(1)
        dstar = q[rows, jstar]
        scale = np.where(dmin > 0, dmin, 1.0)
        worst_nn = max(worst_nn, float(((dstar - dmin) / scale).max()))
        sc2 = np.where(dstar > 0, dstar, 1.0)
        worst_d2 = max(worst_d2, float((np.abs(dist2[k0:k1].astype(np.float64) - dstar) / sc2).max()))
        if count is not None:
            lo = (q < (h2[k0:k1] * (1 - tol))[:, None]).sum(1)
            hi = (q < (h2[k0:k1] * (1 + tol))[:, None]).sum(1)
            c = count[k0:k1].astype(np.int64)
            worst_cnt = max(worst_cnt, int(np.maximum(lo - c, c - hi).max()), 0)
    return worst_nn, worst_d2, worst_cnt
