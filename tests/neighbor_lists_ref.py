"""Brute-force reference for the neighbour lists (nb_neighbor_lists), numpy only.

`lattice_lists`: integer coordinates, int64 arithmetic -- every distance is exact, so the engine's rows must EQUAL it: the members in
ascending index, the `cap` smallest of them when there are more, 0xffffffff behind them, and the true count.  It runs chunked over the
points as neighbors_ref.py does, so the (points x bodies) block never grows past a few million entries."""
import numpy as np

from neighbors_ref import NONE, _blocks


def lattice_lists(bodies, points, radii, cap, skip0=None):
    """bodies (n, >=3), points (m, >=3): integer-valued.  radii: (m,) integers.  skip0: point k leaves body skip0 + k out.
    Returns (lists (m, cap) uint32, count (m,) uint32)."""
    x = np.asarray(bodies)[:, :3].astype(np.int64)
    p = np.asarray(points)[:, :3].astype(np.int64)
    n, m = len(x), len(p)
    h2 = np.asarray(radii).astype(np.int64) ** 2
    lists = np.full((m, cap), NONE, np.uint32)
    count = np.zeros(m, np.uint32)
    for k0, k1 in _blocks(m, n):
        d = x[None, :, :] - p[k0:k1, None, :]
        inside = (d * d).sum(2) < h2[k0:k1, None]
        if skip0 is not None:
            kk = np.arange(k0, k1)
            inside[kk - k0, skip0 + kk] = False
        count[k0:k1] = inside.sum(1)
        rank = np.cumsum(inside, axis=1) - 1                   # position of a member in its row: ascending j
        k, j = np.nonzero(inside & (rank < cap))
        lists[k0 + k, rank[k, j]] = j
    return lists, count


def naive_lists(bodies, points, radii, cap, skip0=None):
    """The same by a plain Python loop per point (for checking lattice_lists itself at small n)."""
    lists = np.full((len(points), cap), NONE, np.uint32)
    count = np.zeros(len(points), np.uint32)
    for k, p in enumerate(points):
        row = []
        for j, b in enumerate(bodies):
            if skip0 is not None and j == skip0 + k:
                continue
            d2 = sum((int(b[c]) - int(p[c])) ** 2 for c in range(3))
            if d2 < int(radii[k]) ** 2:
                row.append(j)
        count[k] = len(row)
        lists[k, :min(cap, len(row))] = row[:cap]
    return lists, count
