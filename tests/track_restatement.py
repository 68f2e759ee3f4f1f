"""Float64 NumPy restatement of the track sampling semantics (DESIGN.md "Track sampling"; dbm_grid_track in include/dbm.h).

Not collected by pytest (no test_ prefix): the CPU tests check it against known answers, the GPU tests check the kernel against it.
`node` may be given a callable (r, c) -> float32 values instead of an array, so that a plane too large for the host can be restated
from the stencil nodes alone.
"""
import numpy as np

INTERP = {"nearest": 0, "bilinear": 1, "bicubic": 2}


def weights(u, k):
    if k == 2:
        return [1.0 - u, u]
    return [u * (u * (-0.5 * u + 1.0) - 0.5), u * u * (1.5 * u - 2.5) + 1.0, u * (u * (-1.5 * u + 2.0) + 0.5), u * u * (0.5 * u - 0.5)]


def _values(grid):
    if callable(grid):
        return grid
    g = np.asarray(grid, dtype=np.float32)
    return lambda r, c: g[r, c]


def _row_node(val, W, r, c):
    """(possibly ghost) column c in [-2, W+1] of grid row r."""
    v = val(r, np.clip(c, 0, W - 1)).astype(np.float64)
    lo, hi = c < 0, c > W - 1
    if lo.any():
        a, b = val(r[lo], 0).astype(np.float64), val(r[lo], 1).astype(np.float64)
        v[lo] = a + (-c[lo]).astype(np.float64) * (a - b)
    if hi.any():
        a, b = val(r[hi], W - 1).astype(np.float64), val(r[hi], W - 2).astype(np.float64)
        v[hi] = a + (c[hi] - (W - 1)).astype(np.float64) * (a - b)
    return v


def node(val, H, W, r, c):
    """(possibly ghost) node (r, c), r in [-2, H+1], c in [-2, W+1]: linear extrapolation, columns first, then rows."""
    v = _row_node(val, W, np.clip(r, 0, H - 1), c)
    lo, hi = r < 0, r > H - 1
    if lo.any():
        a = _row_node(val, W, np.zeros(lo.sum(), np.int64), c[lo])
        b = _row_node(val, W, np.ones(lo.sum(), np.int64), c[lo])
        v[lo] = a + (-r[lo]).astype(np.float64) * (a - b)
    if hi.any():
        a = _row_node(val, W, np.full(hi.sum(), H - 1, np.int64), c[hi])
        b = _row_node(val, W, np.full(hi.sum(), H - 2, np.int64), c[hi])
        v[hi] = a + (r[hi] - (H - 1)).astype(np.float64) * (a - b)
    return v


def sample(grid, shape, geom, xs, ys, interpolation="bicubic", threshold=0.5):
    """z_interpolated at (xs, ys): grid is an (H, W) float32 array or a callable; shape = (H, W); geom = (x0, y0, dx, dy,
    registration 0 gridline / 1 pixel)."""
    H, W = shape
    x0, y0, dx, dy, reg = geom
    val = _values(grid)
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    t, s = (xs - x0) / dx, (ys - y0) / dy
    half = 0.5 if reg == 1 else 0.0
    with np.errstate(invalid="ignore"):
        inside = (t >= -half) & (t <= W - 1 + half) & (s >= -half) & (s <= H - 1 + half)
    out = np.full(xs.shape, np.nan)
    t, s = t[inside], s[inside]
    if interpolation == "nearest":
        r = np.clip(np.floor(s + 0.5), 0, H - 1).astype(np.int64)
        c = np.clip(np.floor(t + 0.5), 0, W - 1).astype(np.int64)
        out[inside] = val(r, c).astype(np.float64)
        return out
    k = 2 if interpolation == "bilinear" else 4
    cf, rf = np.floor(t), np.floor(s)
    wc, wr = weights(t - cf, k), weights(s - rf, k)
    c0 = cf.astype(np.int64) - (1 if k == 4 else 0)
    r0 = rf.astype(np.int64) - (1 if k == 4 else 0)
    acc = np.zeros(t.shape)
    wsum = np.zeros(t.shape)
    holes = np.zeros(t.shape, bool)
    for j in range(k):
        for i in range(k):
            w = wr[j] * wc[i]
            z = node(val, H, W, r0 + j, c0 + i)
            ok = ~np.isnan(z)
            acc[ok] += w[ok] * z[ok]
            wsum[ok] += w[ok]
            holes |= ~ok
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.where(holes, np.where(wsum + 1e-9 >= threshold, acc / wsum, np.nan), acc)
    out[inside] = res
    return out


def sample_chunked(grid, shape, geom, xs, ys, interpolation="bicubic", threshold=0.5, chunk=1 << 20):
    out = np.empty(len(xs))
    for a in range(0, len(xs), chunk):
        out[a:a + chunk] = sample(grid, shape, geom, xs[a:a + chunk], ys[a:a + chunk], interpolation, threshold)
    return out


def stats(z_interpolated, z):
    """count, mean, std (ddof 1), min, max, rmse of the finite errors."""
    e = np.asarray(z_interpolated, np.float64) - np.asarray(z, np.float64)
    e = e[np.isfinite(e)]
    n = e.size
    nan = float("nan")
    if n == 0:
        return dict(count=0, mean=nan, std=nan, min=nan, max=nan, rmse=nan)
    return dict(count=n, mean=float(e.mean()), std=float(e.std(ddof=1)) if n > 1 else nan, min=float(e.min()), max=float(e.max()),
                rmse=float(np.sqrt(np.sum(e * e) / n)))
