"""Scoring a grid against radar survey tracks (reference srgan_train.py:1422-1466, deepbedmap.py:505-626).

The reference samples a predicted bed elevation grid at the survey points with `gmt.grdtrack` and reduces the
along-track error to its RMSE: `rmse_test`, the number that picks the keep-best checkpoint (srgan_train.py:1655-1666)
and is the Optuna objective (:1721).  Here the grid is sampled on the GPU (dbm_grid_track, include/dbm.h) where it
lives -- a DeviceArray canvas of `predict_tiled_resident(download=False)` is read in place -- with GMT's three standard
interpolants (`grdtrack -nn / -nl / -nc`, NaN threshold +t 0.5), and the errors are reduced there too (count, mean,
std, min, max, rmse; deterministic).  Semantics: DESIGN.md "Track sampling".  The rest of the reference's error table and
its error histogram (deepbedmap.py:550-563, 575-608) -- the quartiles of `describe()`, `hist(bins=25)` -- come from
`describe_errors` and `error_histogram`, which read z_interpolated where dbm_grid_track left it (dbm_track_error_quantiles,
dbm_track_error_histogram; DESIGN.md "Error distribution").  No CPU fallback: without a GPU every call raises DbmError.
"""
import dataclasses

import numpy as np

from . import _lib
from .resident import (REGISTRATIONS, DeviceArray, DevicePoints, GridGeometry, devptr, f64ptr, plane_shape, points_table,  # noqa: F401
                       resident_plane, to_device)   # (re-exported: evaluation.GridGeometry is resident.GridGeometry)
from .srgan import using_config

INTERPOLATIONS = {"nearest": 0, "bilinear": 1, "bicubic": 2}
MAX_QUANTILES, MAX_BINS, DIST_WORKSPACE = 16, 4096, 69632   # DBM_TRACK_MAX_QUANTILES, _MAX_BINS, _DIST_WORKSPACE (include/dbm.h)


@dataclasses.dataclass(frozen=True)
class TrackStats:
    """Summary of the finite along-track errors e = z_interpolated - z: the count, mean, std (ddof 1), min and max rows of
    `DataFrame.describe()`, and rmse = sqrt(sum e^2 / count).  The 25 %, 50 % and 75 % rows are in `TrackDescription`
    (`describe_errors`).  count 0: every other value NaN; std NaN for count < 2.  All NaN without a z column."""
    count: int
    mean: float
    std: float
    min: float
    max: float
    rmse: float

    @classmethod
    def from_array(cls, s):
        return cls(int(s[0]), float(s[1]), float(s[2]), float(s[3]), float(s[4]), float(s[5]))


def percentile_label(p):
    """0.25 -> "25%", 0.125 -> "12.5%": the row labels of `describe()`"""
    return f"{round(100.0 * float(p), 9):g}%"


@dataclasses.dataclass(frozen=True)
class TrackDescription:
    """The error table of deepbedmap.py:550-563 for one grid: `stats` (TrackStats) and `quantiles[k]` = the `percentiles[k]` quantile
    of the finite errors (`np.quantile(e, p, method="linear")`, what `describe()` computes; NaN for count 0).  `histogram`: (counts
    int64, edges float64) when bins were asked for, else None."""
    stats: TrackStats
    percentiles: tuple
    quantiles: tuple
    histogram: tuple = dataclasses.field(default=None, compare=False)

    def as_dict(self):
        """`describe()`'s rows in its order: count, mean, std, min, the percentiles (ascending, "25%" ...), max"""
        d = {"count": self.stats.count, "mean": self.stats.mean, "std": self.stats.std, "min": self.stats.min}
        for p, q in sorted(zip(self.percentiles, self.quantiles), key=lambda pq: pq[0]):
            d[percentile_label(p)] = q
        d["max"] = self.stats.max
        return d


_NO_STATS = TrackStats(0, float("nan"), float("nan"), float("nan"), float("nan"), float("nan"))


def _check(interpolation, threshold, H, W):
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {sorted(INTERPOLATIONS)}, got {interpolation!r}")
    if not (0.0 < float(threshold) <= 1.0):
        raise ValueError(f"threshold must lie in (0, 1], got {threshold}")
    if H < 1 or W < 1:
        raise ValueError(f"empty grid ({H} x {W})")
    if interpolation != "nearest" and (H < 2 or W < 2):
        raise ValueError(f"{interpolation} needs at least 2 x 2 nodes, the grid is {H} x {W}")


def grdtrack(points, grid, geometry, interpolation="bicubic", threshold=0.5, return_values=True, ctx=None):
    """`gmt.grdtrack(points=points, grid=grid, newcolname="z_interpolated")` (srgan_train.py:1458) plus the error
    statistics of srgan_train.py:1461-1464 / deepbedmap.py:530-574, on the GPU.

    points: (n, 2) / (n, 3) array or DataFrame of x, y[, z], or DevicePoints (already resident); grid: NumPy array or
    DeviceArray of shape (H, W), (1, H, W) or (1, 1, H, W) (a DeviceArray is read in place); geometry: GridGeometry.
    Returns (z_interpolated float64 (n,) or None, TrackStats; the statistics are NaN without a z column)."""
    return _grdtrack(points, grid, geometry, interpolation, threshold, return_values, ctx)


def _grdtrack(points, grid, geometry, interpolation, threshold, return_values, ctx, resident_values=False):
    """grdtrack; resident_values: a DevicePoints' z_interpolated is written to `points.outputs()[0]` also when it is not returned"""
    H, W = plane_shape(grid)
    _check(interpolation, threshold, H, W)
    if not isinstance(geometry, GridGeometry):
        raise TypeError("geometry must be a GridGeometry")
    if isinstance(points, DevicePoints):
        dpts, pts = points, None
    else:
        dpts, pts = None, points_table(points)
    dgrid, ctx = resident_plane(grid, ctx or (dpts.ctx if dpts is not None else None))
    stats = np.empty(6, dtype=np.float64)
    if dpts is not None:
        if dpts.ctx is not ctx:
            raise ValueError("grdtrack: the points and the grid live on different contexts")
        n, ncol = dpts.n, dpts.ncol
        zdev, sdev = dpts.outputs()
        src, zout, sout, flags = dpts, (zdev if return_values or resident_values else None), sdev, _lib.DEVICE_PTRS
    else:
        n, ncol = pts.shape
        z = np.empty(n if return_values else 0, dtype=np.float64)
        src, zout, sout, flags = pts, (z if return_values else None), stats, 0
    ctx.call("dbm_grid_track", devptr(dgrid), H, W, f64ptr(geometry.as_array()), devptr(src), n, ncol, INTERPOLATIONS[interpolation],
             float(threshold), devptr(zout), devptr(sout), flags)
    if dpts is not None:
        z = ctx.download(zdev, np.float64, n if return_values else 0)
        ctx.download(sdev, out=stats)
    return (z if return_values else None), (TrackStats.from_array(stats) if ncol == 3 else _NO_STATS)


def _probabilities(percentiles):
    q = np.atleast_1d(np.asarray(percentiles, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= MAX_QUANTILES:
        raise ValueError(f"percentiles: 1..{MAX_QUANTILES} probabilities, got shape {q.shape}")
    if not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f"percentiles must lie in [0, 1], got {percentiles!r}")
    return np.ascontiguousarray(q)


def _bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
        raise TypeError(f"bins must be an integer (uniform bins), got {bins!r}")
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must lie in 1..{MAX_BINS}, got {bins}")
    return int(bins)


def histogram_edges(stats, bins, range=None):
    """The bins + 1 edges `np.histogram(e, bins, range)` uses for errors with the extremes of `stats` (NumPy's own rule, by
    NumPy: range None -> (min, max), (0, 1) for count 0; first == last -> -+ 0.5; then np.linspace)."""
    seen = np.array([stats.min, stats.max] if stats.count > 0 else [], dtype=np.float64)
    return np.histogram_bin_edges(seen, bins=_bins(bins), range=range).astype(np.float64, copy=False)


def distribution_arguments(percentiles, bins=None, range=None):
    """The probabilities as a float64 array; ValueError / TypeError for percentiles, bins or a range that will not do"""
    q = _probabilities(percentiles)
    if bins is not None:
        histogram_edges(_NO_STATS, bins, range)
    return q


def _sampled(who, points, grid, geometry, interpolation, threshold, ctx):
    """grdtrack on a DevicePoints (a host table is uploaded once, to the grid's context), z_interpolated left on the device"""
    if not isinstance(points, DevicePoints):
        points = DevicePoints(points, ctx or (grid.ctx if isinstance(grid, DeviceArray) else None))
    if points.ncol != 3:
        raise ValueError(f"{who}: the points need a z column")
    _, stats = _grdtrack(points, grid, geometry, interpolation, threshold, False, ctx, resident_values=True)
    return points, stats


def _quantiles(dpts, q):
    ctx, out = dpts.ctx, np.empty(q.size, dtype=np.float64)
    with ctx.scratch(DIST_WORKSPACE + out.nbytes) as ws:   # the workspace, then the result
        ctx.call("dbm_track_error_quantiles", devptr(dpts), devptr(dpts.outputs()[0]), dpts.n, f64ptr(q), q.size,
                 devptr(ws + DIST_WORKSPACE), devptr(ws), _lib.DEVICE_PTRS)
        ctx.download(ws + DIST_WORKSPACE, out=out)
    return tuple(float(v) for v in out)


def _histogram(dpts, edges):
    ctx, out = dpts.ctx, np.empty(edges.size - 1, dtype=np.int64)
    with ctx.scratch(DIST_WORKSPACE + out.nbytes) as ws:
        ctx.call("dbm_track_error_histogram", devptr(dpts), devptr(dpts.outputs()[0]), dpts.n, f64ptr(edges), out.size,
                 devptr(ws + DIST_WORKSPACE), devptr(ws), _lib.DEVICE_PTRS)
        ctx.download(ws + DIST_WORKSPACE, out=out)
    return out


def describe_errors(points, grid, geometry, interpolation="bicubic", threshold=0.5, percentiles=(0.25, 0.5, 0.75), ctx=None, bins=None,
                    range=None):
    """The error table of deepbedmap.py:550-563 for one grid, on the GPU: `grdtrack` at the points (x, y, z), then
    `(z_interpolated - z).describe(percentiles)` of the finite errors -- TrackStats plus exact quantiles (NumPy's / pandas' linear
    rule on exact order statistics, dbm_track_error_quantiles).  points: array / DataFrame (uploaded once) or DevicePoints;
    z_interpolated stays on the device and only the table comes back.  percentiles: 1..16 probabilities in [0, 1].  With `bins`,
    the description also carries `error_histogram`'s (counts, edges) of the same sampling.  Returns TrackDescription."""
    q = distribution_arguments(percentiles, bins, range)   # (argument errors before any work)
    dpts, stats = _sampled("describe_errors", points, grid, geometry, interpolation, threshold, ctx)
    hist = None
    if bins is not None:
        edges = histogram_edges(stats, bins, range)
        hist = (_histogram(dpts, edges), edges)
    return TrackDescription(stats, tuple(float(v) for v in q), _quantiles(dpts, q), hist)


def error_histogram(points, grid, geometry, bins=25, range=None, interpolation="bicubic", threshold=0.5, ctx=None):
    """`df.hist(column="error", bins=25)`'s numbers (deepbedmap.py:575-608) on the GPU: `np.histogram(e, bins=bins, range=range)` of
    the finite errors e = z_interpolated - z of `grdtrack` at the points.  bins: 1..4096 uniform bins; range None: the errors'
    (min, max), from the statistics of the same sampling.  Returns (counts int64 (bins,), edges float64 (bins + 1,))."""
    distribution_arguments((0.5,), bins, range)   # (argument errors before any work)
    dpts, stats = _sampled("error_histogram", points, grid, geometry, interpolation, threshold, ctx)
    edges = histogram_edges(stats, bins, range)
    return _histogram(dpts, edges), edges


def _forward(model, X_tile, W1_tile, W2_tile, W3_tile, dtype):
    with using_config(name="enable_backprop", value=False), using_config(name="dtype", value=dtype):
        return model.forward(x=X_tile, w1=W1_tile, w2=W2_tile, w3=W3_tile).array


def _test_area_geometry(x, y, H, W):
    """The reference puts np.flipud(Y_hat[0, 0]) on the ground truth's coordinates (srgan_train.py:1451-1455): the
    unflipped output is the same grid with its rows in reverse order."""
    if len(x) != W or len(y) != H:
        raise ValueError(f"coordinates ({len(y)} y, {len(x)} x) do not match the prediction ({H} x {W})")
    return GridGeometry.from_coords(x, y).flipped_rows(H)


def get_deepbedmap_test_result(model, X_tile, W1_tile, W2_tile, W3_tile, points, x, y, interpolation="bicubic",
                               dtype="float32"):
    """srgan_train.py:1422-1466 with the test area's inputs passed in (get_fixed_test_inputs reads files): the generator's
    forward on the area (enable_backprop False), the prediction on the ground truth's coordinates x, y (np.flipud, as the
    reference does), sampled at the survey points (x, y, z) and scored.  Returns (rmse, np.flipud(Y_hat[0, 0]))."""
    if not isinstance(points, DevicePoints) and points_table(points).shape[1] != 3:
        raise ValueError("get_deepbedmap_test_result: the points need a z column")
    ins = [a if isinstance(a, DeviceArray) else to_device(a, model.ctx) for a in (X_tile, W1_tile, W2_tile, W3_tile)]
    Y_hat = _forward(model, *ins, dtype)   # (1, 1, H, W) DeviceArray (model.xp.asarray inputs, srgan_train.py:1442-1448)
    H, W = Y_hat.shape[-2:]
    _, stats = grdtrack(points, Y_hat, _test_area_geometry(x, y, H, W), interpolation=interpolation, return_values=False)
    return stats.rmse, np.flipud(Y_hat.get()[0, 0])


def make_test_area_score(X_tile, W1_tile, W2_tile, W3_tile, points, x, y, interpolation="bicubic", dtype="float32", ctx=None):
    """score_fn(g_model) -> rmse for `train_epochs(score_fn=...)`: get_deepbedmap_test_result's number, with the inputs and
    the points uploaded ONCE here and reused every epoch (the forward's output is sampled where it lies)."""
    ctx = ctx or _lib.default_context()
    _, _, h, w = X_tile.shape
    H, W = 4 * (h - 2), 4 * (w - 2)
    geom = _test_area_geometry(x, y, H, W)
    ins = [a if isinstance(a, DeviceArray) else to_device(a, ctx) for a in (X_tile, W1_tile, W2_tile, W3_tile)]
    dpts = points if isinstance(points, DevicePoints) else DevicePoints(points, ctx)
    if dpts.ncol != 3:
        raise ValueError("make_test_area_score: the points need a z column")
    _check(interpolation, 0.5, H, W)

    def score_fn(g_model):
        Y_hat = _forward(g_model, *ins, dtype)
        return grdtrack(dpts, Y_hat, geom, interpolation=interpolation, return_values=False)[1].rmse

    return score_fn
