"""Scoring a grid against radar survey tracks (reference srgan_train.py:1422-1466, deepbedmap.py:505-626).

The reference samples a predicted bed elevation grid at the survey points with `gmt.grdtrack` and reduces the
along-track error to its RMSE: `rmse_test`, the number that picks the keep-best checkpoint (srgan_train.py:1655-1666)
and is the Optuna objective (:1721).  Here the grid is sampled on the GPU (dbm_grid_track, include/dbm.h) where it
lives -- a DeviceArray canvas of `predict_tiled_resident(download=False)` is read in place -- with GMT's three standard
interpolants (`grdtrack -nn / -nl / -nc`, NaN threshold +t 0.5), and the errors are reduced there too (count, mean,
std, min, max, rmse; deterministic).  Semantics: DESIGN.md "Track sampling".  No CPU fallback: without a GPU every
call raises DbmError.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .srgan import DeviceArray, to_device, using_config

INTERPOLATIONS = {"nearest": 0, "bilinear": 1, "bicubic": 2}
REGISTRATIONS = {"gridline": 0, "pixel": 1}


@dataclasses.dataclass(frozen=True)
class GridGeometry:
    """Node (r, c) of a grid sits at (x0 + c dx, y0 + r dy); dx, dy non-zero, either sign (north-up: dy < 0).
    registration "gridline": nodes are the grid's extent (domain [0, W-1] x [0, H-1] in node units); "pixel": nodes are the
    centres of pixels (domain [-1/2, W-1/2] x [-1/2, H-1/2])."""
    x0: float
    y0: float
    dx: float
    dy: float
    registration: str = "gridline"

    def __post_init__(self):
        if self.registration not in REGISTRATIONS:
            raise ValueError(f"registration must be one of {sorted(REGISTRATIONS)}, got {self.registration!r}")
        for name in ("x0", "y0", "dx", "dy"):
            if not np.isfinite(getattr(self, name)):
                raise ValueError(f"GridGeometry.{name} must be finite")
        if self.dx == 0 or self.dy == 0:
            raise ValueError("GridGeometry: dx and dy must be non-zero")

    @classmethod
    def from_bounds(cls, window_bound, height, width):
        """The geometry `save_array_to_grid(window_bound=...)` writes for a (height, width) array: pixel registration,
        north-up, tiepoint (minx, maxy), pixel scale ((maxx - minx) / width, (maxy - miny) / height)."""
        minx, miny, maxx, maxy = (float(v) for v in window_bound)
        px, py = (maxx - minx) / int(width), (maxy - miny) / int(height)
        return cls(x0=minx + px / 2, y0=maxy - py / 2, dx=px, dy=-py, registration="pixel")

    @classmethod
    def from_coords(cls, x, y, registration="gridline"):
        """From evenly spaced 1-D coordinate vectors (xarray-style: x[c], y[r] are the nodes' coordinates)."""
        def spacing(v, name):
            v = np.asarray(v, dtype=np.float64).ravel()
            if v.size < 2:
                raise ValueError(f"from_coords: {name} needs at least two coordinates to define a spacing")
            d = (v[-1] - v[0]) / (v.size - 1)
            if d == 0 or not np.isfinite(d) or np.abs(np.diff(v) - d).max() > 1e-6 * abs(d):
                raise ValueError(f"from_coords: {name} is not evenly spaced")
            return float(v[0]), float(d)

        x0, dx = spacing(x, "x")
        y0, dy = spacing(y, "y")
        return cls(x0=x0, y0=y0, dx=dx, dy=dy, registration=registration)

    def flipped_rows(self, height):
        """The same nodes with the row order reversed (row r becomes row height - 1 - r)."""
        return dataclasses.replace(self, y0=self.y0 + (int(height) - 1) * self.dy, dy=-self.dy)

    def as_array(self):
        return np.array([self.x0, self.y0, self.dx, self.dy, REGISTRATIONS[self.registration]], dtype=np.float64)


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


class DevicePoints:
    """Survey points (x, y[, z]) resident in HBM as float64 (n, ncol): upload once, sample many grids (make_test_area_score).
    Holds its own output buffer (z_interpolated + statistics), reused from call to call."""

    def __init__(self, points, ctx=None):
        pts = _points_array(points)
        self.ctx = ctx or _lib.default_context()
        self.n, self.ncol = pts.shape
        self.ptr = self.ctx.malloc(max(pts.nbytes, 8))
        if pts.nbytes:
            _lib.check(_lib.lib().dbm_memcpy_h2d(self.ctx.handle, C.c_void_p(self.ptr), pts.ctypes.data_as(C.c_void_p), pts.nbytes),
                       self.ctx.handle)
        self._out = None   # device: z_interpolated (n doubles), then 8 doubles of statistics

    @classmethod
    def adopt(cls, ptr, n, ncol, ctx):
        """A table that is resident already (what `ascii_to_xyz(download=False)` parsed): `ptr` -- from ctx.malloc, at least 8 n ncol
        bytes, float64 (n, ncol) -- becomes the object's own and is freed with it.  Nothing is uploaded."""
        self = cls.__new__(cls)
        self.ctx, self.n, self.ncol, self.ptr, self._out = ctx, int(n), int(ncol), ptr, None
        return self

    def outputs(self):
        if self._out is None:
            self._out = self.ctx.malloc(8 * (self.n + 8))
        return self._out, self._out + 8 * self.n

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            for p in (self.ptr, self._out):
                if p:
                    self.ctx.free(p)
            self.ptr = self._out = 0
        except Exception:
            pass


def _points_array(points):
    """(n, 2) / (n, 3) float64 C-contiguous: x, y[, z] -- a NumPy array or a DataFrame with columns x, y[, z]."""
    if hasattr(points, "columns"):   # pandas.DataFrame (the reference's `points` table, data_prep.ascii_to_xyz)
        cols = ["x", "y", "z"] if "z" in points.columns else ["x", "y"]
        points = points[cols].to_numpy()
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] not in (2, 3):
        raise ValueError(f"points must be (n, 2) x, y or (n, 3) x, y, z; got shape {pts.shape}")
    return pts


def _grid_plane(grid):
    shape = tuple(int(s) for s in grid.shape)
    if len(shape) == 2 or (len(shape) == 3 and shape[0] == 1) or (len(shape) == 4 and shape[:2] == (1, 1)):
        return shape[-2], shape[-1]
    raise ValueError(f"grid must be (H, W), (1, H, W) or (1, 1, H, W); got {shape}")


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
    H, W = _grid_plane(grid)
    _check(interpolation, threshold, H, W)
    if not isinstance(geometry, GridGeometry):
        raise TypeError("geometry must be a GridGeometry")
    if isinstance(points, DevicePoints):
        dpts, pts = points, None
    else:
        dpts, pts = None, _points_array(points)
    if isinstance(grid, DeviceArray):
        ctx = grid.ctx
        dgrid = grid
    else:
        ctx = ctx or (dpts.ctx if dpts is not None else _lib.default_context())
        dgrid = to_device(np.asarray(grid, dtype=np.float32).reshape(H, W), ctx)
    lib = _lib.lib()
    geom = geometry.as_array()
    args = (ctx.handle, C.c_void_p(dgrid.ptr), H, W, geom.ctypes.data_as(C.POINTER(C.c_double)))
    interp = INTERPOLATIONS[interpolation]
    if dpts is not None:
        if dpts.ctx is not ctx:
            raise ValueError("grdtrack: the points and the grid live on different contexts")
        n, ncol = dpts.n, dpts.ncol
        zdev, sdev = dpts.outputs()
        _lib.check(lib.dbm_grid_track(*args, C.c_void_p(dpts.ptr), n, ncol, interp, float(threshold),
                                      C.c_void_p(zdev) if return_values else None, C.c_void_p(sdev), _lib.DEVICE_PTRS), ctx.handle)
        z = np.empty(n if return_values else 0, dtype=np.float64)
        stats = np.empty(6, dtype=np.float64)
        if z.size:
            _lib.check(lib.dbm_memcpy_d2h(ctx.handle, z.ctypes.data_as(C.c_void_p), C.c_void_p(zdev), z.nbytes), ctx.handle)
        _lib.check(lib.dbm_memcpy_d2h(ctx.handle, stats.ctypes.data_as(C.c_void_p), C.c_void_p(sdev), stats.nbytes), ctx.handle)
    else:
        n, ncol = pts.shape
        z = np.empty(n if return_values else 0, dtype=np.float64)
        stats = np.empty(6, dtype=np.float64)
        _lib.check(lib.dbm_grid_track(*args, pts.ctypes.data_as(C.c_void_p), n, ncol, interp, float(threshold),
                                      z.ctypes.data_as(C.c_void_p) if return_values else None, stats.ctypes.data_as(C.c_void_p), 0),
                   ctx.handle)
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
    if not isinstance(points, DevicePoints) and _points_array(points).shape[1] != 3:
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
