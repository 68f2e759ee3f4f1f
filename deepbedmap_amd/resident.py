"""What lives in HBM between the stages of the data layer, and how a stage hands it to libdbm.

`DeviceArray` (a plane, a canvas, a batch of tiles, a mask), `DevicePoints` (a survey's point table) and `GridGeometry` (where a
plane's nodes lie) are what the data-preparation and scoring modules pass to one another; the helpers below turn what a caller may
give in their place -- a NumPy array, a DataFrame -- into them, and any of them into the pointer a library call takes
(`ctx.call(name, devptr(a), ...)`, _lib.Context).  In this module "array" means a NumPy array or a DeviceArray.  No CPU fallback:
creating a resident object without a GPU raises DbmError.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _lib

REGISTRATIONS = {"gridline": 0, "pixel": 1}
WORKSPACE_DEFAULT = 1 << 30   # bytes of block staging per batch of a resident read (block_reads.py) or write (block_writes.py)


class DeviceArray:
    """float32 C-contiguous array resident in HBM (owned unless wrapping foreign memory); `dtype` makes it a float64, int32 or uint8
    array instead."""

    def __init__(self, shape, ctx=None, ptr=None, owner=None, dtype=np.float32):
        self.ctx = ctx or _lib.default_context()
        self.shape = tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape)) if self.shape else 1
        self.dtype = np.dtype(dtype)
        self._own = ptr is None
        self.ptr = self.ctx.malloc(self.dtype.itemsize * max(self.size, 1)) if ptr is None else int(ptr)
        self._owner = owner
        self._gen = 0  # content version: bumped by every write through this object

    @property
    def nbytes(self):
        return self.dtype.itemsize * self.size

    def __len__(self):
        return self.shape[0]

    def data_ptr(self):
        return self.ptr

    def set(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.size == self.size, (host.shape, self.shape)
        self._gen += 1
        self.ctx.upload(self.ptr, host)
        return self

    def get(self):
        return self.ctx.download(self.ptr, self.dtype, self.shape)

    def written(self):
        """To be called after the library has written into the array: moves its content version, which decides whether a forward
        computed ahead from the array may still be consumed (training._content_token).  Returns the array."""
        self._gen += 1
        return self

    def __array__(self, dtype=None, copy=None):
        a = self.get()
        return a.astype(dtype) if dtype is not None else a

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self._own and self.ptr:
                self.ctx.free(self.ptr)
                self.ptr = 0
        except Exception:
            pass


def to_device(a, ctx=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return DeviceArray(a.shape, ctx).set(a)


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


def points_table(points, ncols=lambda c: c in (2, 3), what="points must be (n, 2) x, y or (n, 3) x, y, z"):
    """float64 C-contiguous (n, ncol) from a NumPy array or a DataFrame with columns x, y[, z] (the reference's `points` table,
    data_prep.ascii_to_xyz; no pandas import).  `ncols(ncol)` says whether the number of columns will do; `what` opens the ValueError
    otherwise."""
    if hasattr(points, "columns"):
        cols = ["x", "y", "z"] if "z" in points.columns else ["x", "y"]
        points = points[cols].to_numpy()
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or not ncols(pts.shape[1]):
        raise ValueError(f"{what}; got shape {pts.shape}")
    return pts


class DevicePoints:
    """Survey points (x, y[, z]) resident in HBM as float64 (n, ncol): upload once, sample many grids (make_test_area_score).
    Holds its own output buffer (z_interpolated + statistics), reused from call to call."""

    def __init__(self, points, ctx=None):
        pts = points_table(points)
        self.ctx = ctx or _lib.default_context()
        self.n, self.ncol = pts.shape
        self.ptr = self.ctx.malloc(max(pts.nbytes, 8))
        self.ctx.upload(self.ptr, pts)
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


def shape_of(x):
    """The shape of an array, or of anything NumPy can make one of."""
    return x.shape if isinstance(x, DeviceArray) else np.shape(x)


def plane_shape(grid):
    """(H, W) of an array of shape (H, W), (1, H, W) or (1, 1, H, W)."""
    shape = tuple(int(s) for s in grid.shape)
    if len(shape) == 2 or (len(shape) == 3 and shape[0] == 1) or (len(shape) == 4 and shape[:2] == (1, 1)):
        return shape[-2], shape[-1]
    raise ValueError(f"grid must be (H, W), (1, H, W) or (1, 1, H, W); got {shape}")


def resident_plane(grid, ctx=None, what=None):
    """(DeviceArray, its context) of one plane: a DeviceArray is used in place, anything else is uploaded to `ctx` (None: the default
    context) as a float32 (H, W) array.  With `what`, the caller's name for the message, the grid must be exactly (H, W); without it
    `plane_shape` decides, and (1, H, W) and (1, 1, H, W) will do too."""
    if not isinstance(grid, DeviceArray):
        grid = np.asarray(grid, dtype=np.float32)
    if what is None:
        shape = plane_shape(grid)
    elif len(grid.shape) != 2:
        raise ValueError(f"{what}: the grid must be (H, W); got {grid.shape}")
    else:
        shape = grid.shape
    if isinstance(grid, DeviceArray):
        return grid, grid.ctx
    ctx = ctx or _lib.default_context()
    return to_device(grid.reshape(shape), ctx), ctx


def devptr(x):
    """What a `void*` parameter of the library takes for `x`: a DeviceArray's or a DevicePoints' memory, a raw device pointer (an int),
    a NumPy array's own memory (for the entry points that also read and write host memory), or None for NULL."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(x) if isinstance(x, (int, np.integer)) else x.ptr)


def f64ptr(a):
    """The `double*` of a float64 NumPy array."""
    return a.ctypes.data_as(C.POINTER(C.c_double))
