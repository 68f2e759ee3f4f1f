"""Float64 NumPy restatement of the tiling semantics (DESIGN.md "Tiling"; dbm_grid_tile and dbm_grid_filled_windows in include/dbm.h).

Not collected by pytest (no test_ prefix): the CPU tests check it against scipy.interpolate.interpn, numpy.ma.masked_values and the
reference's doctest answers; the GPU tests check the kernels against it.  Written from the rules, not from the kernel.  `grid` may be
a callable (r, c) -> float32 values instead of an array, so that a plane too large for the host is restated from the nodes it needs.
"""
import numpy as np


def _values(grid):
    if callable(grid):
        return grid
    g = np.asarray(grid, dtype=np.float32)
    return lambda r, c: g[r, c]


def pad_windows(window_bounds, padding=0):
    """(n, 4) left, bottom, right, top (data_prep.py:660-665)."""
    w = np.asarray(window_bounds, dtype=np.float64)
    return np.stack([w[:, 0] - padding, w[:, 1] - padding, w[:, 2] + padding, w[:, 3] + padding], axis=1)


def tile_shape(padded, res):
    left, bottom, right, top = (float(v) for v in padded[0])
    return int((top - bottom) / res), int((right - left) / res)


def window_coords(window, res, out_h, out_w):
    """new_y (top to bottom), new_x of one padded window (data_prep.py:695-696)."""
    left, bottom, right, top = (float(v) for v in window)
    half = res / 2
    return np.linspace(top - half, bottom + half, num=out_h), np.linspace(left + half, right - half, num=out_w)


def axis(x0, dx, n):
    """The axis sorted ascending and the raster index of each of its nodes."""
    g = np.arange(n, dtype=np.float64) * dx + x0     # multiply, then add
    j = np.arange(n)
    return (g, j) if dx > 0 else (g[::-1], j[::-1])


def cells(c, g):
    """scipy's rule on the ascending axis g: i with g[i] <= c < g[i+1] (last node: i = n - 2), t, and the outside / NaN flag."""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(c) | (c < g[0]) | (c > g[-1])
    i = np.clip(np.searchsorted(g, np.where(bad, g[0], c), side="right") - 1, 0, len(g) - 2)
    t = (c - g[i]) / (g[i + 1] - g[i])
    return i, t, bad


def bilinear(grid, shape, geom, ys, xs):
    """The float64 (len(ys), len(xs)) interpolant at the outer product of the coordinates ys, xs."""
    H, W = shape
    x0, y0, dx, dy = geom[:4]
    val = _values(grid)
    gy, jy = axis(y0, dy, H)
    gx, jx = axis(x0, dx, W)
    iy, ty, bady = cells(ys, gy)
    ix, tx, badx = cells(xs, gx)
    r0, r1 = jy[iy][:, None], jy[iy + 1][:, None]
    c0, c1 = jx[ix][None, :], jx[ix + 1][None, :]
    ty, tx = ty[:, None], tx[None, :]
    r0, r1, c0, c1 = (np.broadcast_to(a, (len(ys), len(xs))) for a in (r0, r1, c0, c1))
    z = [val(r, c).astype(np.float64) for r, c in ((r0, c0), (r0, c1), (r1, c0), (r1, c1))]
    with np.errstate(invalid="ignore"):
        v = 0.0 + z[0] * ((1 - ty) * (1 - tx))
        v = v + z[1] * ((1 - ty) * tx)
        v = v + z[2] * (ty * (1 - tx))
        v = v + z[3] * (ty * tx)
    v[bady, :] = np.nan
    v[:, badx] = np.nan
    return v


def nodes_of(coords, x0, dx, n):
    """Raster indices of the nodes whose coordinate EQUALS each of coords; KeyError if there is none (sel, tolerance 0)."""
    g = np.arange(n, dtype=np.float64) * dx + x0
    out = []
    for c in coords:
        hit = np.flatnonzero(g == c)
        if hit.size == 0:
            raise KeyError(float(c))
        out.append(int(hit[0]))
    return np.array(out)


def mask_rule(v, nodata):
    """numpy.ma.masked_values(v, nodata): |v - nodata| <= 1e-8 + 1e-5 |nodata|; NaN or no nodata masks nothing, NaN values are never masked."""
    v = np.asarray(v, dtype=np.float64)
    if nodata is None or np.isnan(nodata):
        return np.zeros(v.shape, bool)
    with np.errstate(invalid="ignore"):
        return np.abs(v - nodata) <= 1e-8 + 1e-5 * abs(nodata)


def tile(grid, shape, geom, window_bounds, padding=0, resolution=None, nodata=None, gapfiller=None, interpolate=True, fill_nan=False):
    """selective_tile: (tiles float32 (n, 1, h, w), masked counts int (n,))."""
    H, W = shape
    x0, y0, dx, dy = geom[:4]
    assert abs(dx) == abs(dy)
    res = abs(dx) if resolution is None else float(resolution)
    padded = pad_windows(window_bounds, padding)
    out_h, out_w = tile_shape(padded, res)
    assert out_h >= 1 and out_w >= 1
    val = _values(grid)
    tiles = np.empty((len(padded), 1, out_h, out_w), dtype=np.float32)
    counts = np.zeros(len(padded), dtype=np.int64)
    for k, wb in enumerate(padded):
        ys, xs = window_coords(wb, res, out_h, out_w)
        if interpolate:
            v = bilinear(val, shape, geom, ys, xs)
        else:
            assert res == abs(dx)
            rr, cc = nodes_of(ys, y0, dy, H), nodes_of(xs, x0, dx, W)
            v = val(np.broadcast_to(rr[:, None], (out_h, out_w)), np.broadcast_to(cc[None, :], (out_h, out_w))).astype(np.float64)
        m = mask_rule(v, nodata)
        if fill_nan:
            m |= np.isnan(v)
        o = v.astype(np.float32)
        if gapfiller is not None:
            o[m] = np.float32(gapfiller)
        tiles[k, 0] = o
        counts[k] = m.sum()
    return tiles, counts


def filled_windows(grid, geom, size, step):
    """flags (ny, nx) uint8: 1 iff the size x size window (uly step, ulx step), counted from the north-west corner, holds no NaN."""
    g = np.asarray(grid, dtype=np.float32)
    x0, y0, dx, dy = geom[:4]
    mask = np.isnan(g)
    if dy > 0:
        mask = mask[::-1]
    if dx < 0:
        mask = mask[:, ::-1]
    H, W = mask.shape
    ny, nx = (H - size) // step + 1, (W - size) // step + 1
    views = np.lib.stride_tricks.sliding_window_view(mask, (size, size))[::step, ::step]
    assert views.shape[:2] == (ny, nx)
    return (~views.any(axis=(-2, -1))).astype(np.uint8)
