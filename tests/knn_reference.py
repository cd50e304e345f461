"""Brute-force k nearest neighbours in numpy float32: the oracle of gs_knn3d / knn.

The squared distance is `(dx * dx + dy * dy) + dz * dz` with d = p_j - p_i, every operation a float32 operation in
this order (numpy rounds each one, and has no fused multiply-add), which is the kernel's contract: results compare
with `==`.  Row i lists the k points j != i with the smallest (dist2, j) in lexicographic order; the point itself is
removed by index; a point with a non-finite coordinate is nobody's neighbour and its own row is empty; missing entries
are +inf / -1."""
import numpy as np


def reference_knn(points, k):
    """points (N,3) float32 -> (dist2 (N,k) float32, index (N,k) int64)"""
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float32)
    assert p.ndim == 2 and p.shape[1] == 3
    n = p.shape[0]
    dist2 = np.full((n, k), np.inf, dtype=np.float32)
    index = np.full((n, k), -1, dtype=np.int64)
    usable = np.isfinite(p).all(axis=1)
    all_rows = np.arange(n)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            if not usable[i]:
                continue
            d = p - p[i]  # float32 - float32
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d2.dtype == np.float32
            keep = usable & (all_rows != i)
            j, d2 = all_rows[keep], d2[keep]
            order = np.lexsort((j, d2))[:k]
            dist2[i, :len(order)] = d2[order]
            index[i, :len(order)] = j[order]
    return dist2, index
