"""Float64 NumPy restatement of the error distribution (DESIGN.md "Error distribution"; dbm_track_error_quantiles and
dbm_track_error_histogram in include/dbm.h): which errors take part, the quantile rule on exact order statistics, the uniform-bin rule.

Not collected by pytest (no test_ prefix): the CPU tests check it against np.quantile, pandas' describe() and np.histogram, the GPU
tests check the kernels against it.  Every product and sum below is one NumPy operation, so each is rounded on its own.
"""
import numpy as np


def errors(points, z_interpolated):
    """The errors that take part: e = z_interpolated - z where that is finite, -0.0 as +0.0; in the points' order."""
    e = np.asarray(z_interpolated, dtype=np.float64) - np.asarray(points, dtype=np.float64).reshape(-1, 3)[:, 2]
    e = e[np.isfinite(e)]
    return np.where(e == 0.0, 0.0, e)


def keys(e):
    """The order-preserving 64-bit keys the select works on: sign bit set -> all bits flipped, else the sign bit set."""
    b = np.ascontiguousarray(e, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def quantiles(e, probabilities):
    """NumPy's method="linear" on the sorted errors: h = (m - 1) q, j = floor(h), g = h - j, neighbours a = e[j], b = e[j + 1] (both
    the maximum where h >= m - 1), d = b - a, a + d g or, where g >= 0.5, b - d (1 - g).  m = 0: NaN."""
    e = np.sort(np.asarray(e, dtype=np.float64))
    q = np.atleast_1d(np.asarray(probabilities, dtype=np.float64))
    m = e.size
    if m == 0:
        return np.full(q.shape, np.nan)
    top = np.float64(m - 1)
    h = top * q
    j = np.floor(h)
    g = h - j
    above = h >= top
    lo = np.where(above, m - 1, j).astype(np.int64)
    hi = np.where(above, m - 1, j + 1).astype(np.int64)
    a, b = e[lo], e[np.minimum(hi, m - 1)]
    d = b - a
    low = a + d * g
    high = b - d * (1.0 - g)
    return np.where(above, b, np.where(g >= 0.5, high, low))


def histogram(e, edges):
    """np.histogram's uniform-bin rule with the given bins + 1 edges: int64 counts."""
    e = np.asarray(e, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    B = edges.size - 1
    first, last = edges[0], edges[B]
    e = e[(e >= first) & (e <= last)]
    i = (((e - first) / (last - first)) * B).astype(np.int64)
    i[i == B] -= 1
    i[e < edges[i]] -= 1
    i[(e >= edges[i + 1]) & (i != B - 1)] += 1
    return np.bincount(i, minlength=B).astype(np.int64)


def describe(e, percentiles=(0.25, 0.5, 0.75)):
    """`Series(e).describe(percentiles)` as a dict in its order (std with ddof 1; an empty series: count 0, the rest NaN)."""
    e = np.asarray(e, dtype=np.float64)
    nan = float("nan")
    d = {"count": e.size, "mean": e.mean() if e.size else nan, "std": e.std(ddof=1) if e.size > 1 else nan,
         "min": e.min() if e.size else nan}
    for p, v in sorted(zip(percentiles, quantiles(e, percentiles))):
        d[f"{round(100.0 * p, 9):g}%"] = v
    d["max"] = e.max() if e.size else nan
    return d
