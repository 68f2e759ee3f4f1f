"""Scoring a grid against radar survey tracks (reference srgan_train.py:1422-1466, deepbedmap.py:505-626).

The reference samples a predicted bed elevation grid at the survey points with `gmt.grdtrack` and reduces the
along-track error to its RMSE: `rmse_test`, the number that picks the keep-best checkpoint (srgan_train.py:1655-1666)
and is the Optuna objective (:1721).  Here the grid is sampled on the GPU (dbm_grid_track, include/dbm.h) where it
lives -- a DeviceArray canvas of `predict_tiled_resident(download=False)` is read in place -- with GMT's three standard
interpolants (`grdtrack -nn / -nl / -nc`, NaN threshold +t 0.5), and the errors are reduced there too (count, mean,
std, min, max, rmse; deterministic).  Semantics: DESIGN.md "Track sampling".  No CPU fallback: without a GPU every
call raises DbmError.
"""
import dataclasses

import numpy as np

from . import _lib
from .resident import (REGISTRATIONS, DeviceArray, DevicePoints, GridGeometry, devptr, f64ptr, plane_shape, points_table,  # noqa: F401
                       resident_plane, to_device)   # (re-exported: evaluation.GridGeometry is resident.GridGeometry)
from .srgan import using_config

INTERPOLATIONS = {"nearest": 0, "bilinear": 1, "bicubic": 2}


@dataclasses.dataclass(frozen=True)
class TrackStats:
    """Summary of the finite along-track errors e = z_interpolated - z (`DataFrame.describe()` columns, std with ddof 1) and
    rmse = sqrt(sum e^2 / count).  count 0: every other value NaN; std NaN for count < 2.  All NaN without a z column."""
    count: int
    mean: float
    std: float
    min: float
    max: float
    rmse: float

    @classmethod
    def from_array(cls, s):
        return cls(int(s[0]), float(s[1]), float(s[2]), float(s[3]), float(s[4]), float(s[5]))


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
        src, zout, sout, flags = dpts, (zdev if return_values else None), sdev, _lib.DEVICE_PTRS
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
