"""Cutting training tiles and model inputs from rasters that live in HBM (reference data_prep.py:501-572 `get_window_bounds`,
:622-741 `selective_tile`, :757-771 and :880-911 the training set; deepbedmap.py:132-213 `get_deepbedmap_model_inputs`).

The reference opens each raster with xarray / rasterio, interpolates every window with `DataArray.interp(method="linear")`
(scipy.interpolate.interpn) under dask, and masks nodata with numpy.ma.masked_values.  Here the raster is a DeviceArray (the
continent's planes `predict_tiled_resident` already keeps resident), and the windows are cut where it lies by dbm_grid_tile /
dbm_grid_filled_windows (include/dbm.h).  Semantics: DESIGN.md "Tiling".  No CPU fallback: without a GPU every call that reaches
the library raises DbmError; argument errors are raised before that.
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from .geotiff import read_geotiff, read_geotiff_resident
from .resident import DeviceArray, GridGeometry, devptr, f64ptr, plane_shape, to_device


class Raster:
    """One band on its grid: `array` (H, W), (1, H, W) or (1, 1, H, W) -- a DeviceArray is used in place, a NumPy array is
    uploaded once, at its first use --, `geometry` a GridGeometry (node (r, c) at (x0 + c dx, y0 + r dy), square pixels for
    selective_tile), `nodata` the value that marks missing data (None or NaN: none)."""

    def __init__(self, array, geometry, nodata=None, ctx=None):
        if not isinstance(geometry, GridGeometry):
            raise TypeError("geometry must be a GridGeometry")
        self.H, self.W = plane_shape(array)
        if self.H < 1 or self.W < 1:
            raise ValueError(f"empty raster ({self.H} x {self.W})")
        if nodata is not None:
            nodata = float(nodata)
            if np.isinf(nodata):
                raise ValueError("nodata must be finite, NaN or None")
        self.geometry, self.nodata = geometry, nodata
        if isinstance(array, DeviceArray):
            self._dev, self._host, self.ctx = array, None, array.ctx
        else:
            self._dev, self._host, self.ctx = None, np.asarray(array, dtype=np.float32).reshape(self.H, self.W), ctx

    @classmethod
    def from_geotiff(cls, path, ctx=None):
        """A file `geotiff.read_geotiff` decodes (what save_array_to_grid writes): the geometry from the pixel scale and the
        tiepoint (nodes are pixel centres, north-up), nodata from the GDAL_NODATA tag."""
        array, info = read_geotiff(path)
        px, py, _ = info["pixel_scale"]
        i, j, _, x, y, _ = info["tiepoint"]
        geometry = GridGeometry(x0=x + (0.5 - i) * px, y0=y - (0.5 - j) * py, dx=px, dy=-py, registration="pixel")
        nodata = float(info["nodata"]) if info["nodata"] else None
        return cls(array[0].astype(np.float32), geometry, nodata=nodata, ctx=ctx)

    @classmethod
    def open(cls, path, window_bound=None, ctx=None, overview=0):
        """A GeoTIFF as GDAL and libtiff write them (`geotiff.open_geotiff`'s dialect), decoded on the GPU and resident from the
        start: the file's geometry (GTRasterTypeGeoKey honoured), shifted to the window (minx, miny, maxx, maxy) if one is given
        -- only its blocks are read --, and its GDAL_NODATA.  A file without georeference raises ValueError.  overview = k > 0: the
        file's k-th reduced-resolution image instead of the first one, on the same extent."""
        from .geotiff import open_geotiff

        if isinstance(path, str) and path.startswith("netcdf:"):   # the reference's GDAL subdataset names (data_prep.py:889-900)
            file, _, variable = path[len("netcdf:"):].rpartition(":")
            if not file or not variable:
                raise ValueError(f"{path}: a netCDF variable is named netcdf:FILE:VARIABLE")
            if overview:
                raise ValueError(f"{path}: overview {overview!r}: netCDF variables have no overviews")
            return cls.open_netcdf(file, variable, window_bound=window_bound, ctx=ctx)
        open_geotiff(path, overview).geometry   # (raises before any device work)
        array, info = read_geotiff_resident(path, window_bound=window_bound, ctx=ctx, overview=overview)
        try:
            nodata = float(info["nodata"]) if info["nodata"] else None
        except ValueError:
            raise ValueError(f"{path}: GDAL_NODATA (42113) = {info['nodata']!r} is not a number") from None
        if nodata is not None and np.isinf(nodata):
            nodata = None   # (GDAL writes "inf" / "-inf" too; a Raster's nodata is finite or NaN)
        return cls(array, info["geometry"], nodata=nodata)

    @classmethod
    def open_netcdf(cls, path, variable=None, window_bound=None, ctx=None):
        """A variable of a netCDF file (`netcdf.open_netcdf`'s dialect: netCDF-4 / HDF5 chunks with shuffle and deflate, classic
        CDF-1 / CDF-2), its chunks placed on the GPU and resident from the start, north-up, masked and scaled by the module's value
        rule; `variable` None: the file's only 2-D variable.  The geometry comes from the file's x / y coordinates (a file without
        them raises ValueError), shifted to the window if one is given -- only its chunks are read.  nodata is NaN when the variable
        has a fill (those samples ARE NaN), else None."""
        from .netcdf import open_netcdf, read_netcdf_resident

        if open_netcdf(path, variable).geometry is None:   # (raises before any device work)
            raise ValueError(f"{path}: no georeference: the coordinate variables x and y are missing")
        array, info = read_netcdf_resident(path, variable, window_bound=window_bound, ctx=ctx)
        return cls(array, info["geometry"], nodata=None if info["fill"] is None else float("nan"))

    @property
    def shape(self):
        return self.H, self.W

    def device(self):
        """The plane in HBM (uploads a NumPy raster once)."""
        if self._dev is None:
            self.ctx = self.ctx or _lib.default_context()
            self._dev = to_device(self._host, self.ctx)
            self._host = None
        return self._dev


def _windows_array(window_bounds):
    w = np.asarray(window_bounds, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != 4 or w.shape[0] < 1:
        raise ValueError(f"window_bounds must be a non-empty list of (minx, miny, maxx, maxy); got shape {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError("window_bounds must be finite")
    return w


def tile_shape(window_bounds, padding, resolution):
    """(y_length, x_length) of data_prep.py:679-680: from the FIRST window, for all of them."""
    x0, y0, x1, y1 = (float(v) for v in np.asarray(window_bounds, dtype=np.float64)[0])
    left, bottom, right, top = x0 - padding, y0 - padding, x1 + padding, y1 + padding
    return int((top - bottom) / resolution), int((right - left) / resolution)


def _axis_nodes(coords, x0, dx, n):
    """Raster indices j with x0 + j dx == coords, exactly (`sel(method="nearest", tolerance=0)`); -1 where there is none."""
    j = np.rint((coords - x0) / dx)
    j = np.where(np.isfinite(j), j, -1).astype(np.int64)
    ok = (j >= 0) & (j < n)
    ok &= (np.where(ok, j, 0).astype(np.float64) * dx + x0) == coords
    return np.where(ok, j, -1)


def _linspace_rows(start, stop, num):
    """Row k = np.linspace(start[k], stop[k], num): arange(num) * step + start, the end point stored exactly."""
    if num == 1:
        return start[:, None].copy()
    v = np.arange(num, dtype=np.float64)[None, :] * ((stop - start) / (num - 1))[:, None] + start[:, None]
    v[:, -1] = stop
    return v


def slice_windows(geometry, shape, padded, out_h, out_w, resolution):
    """The host side of interpolate=False: (n, 4) int64 (row0, col0, row step, column step) after checking that every output
    coordinate of every window EQUALS a node coordinate (the reference raises KeyError otherwise); ValueError names the first
    offending window."""
    H, W = shape
    half = resolution / 2
    new_y = _linspace_rows(padded[:, 3] - half, padded[:, 1] + half, out_h)   # (n, out_h), top to bottom
    new_x = _linspace_rows(padded[:, 0] + half, padded[:, 2] - half, out_w)
    rows = _axis_nodes(new_y, geometry.y0, geometry.dy, H)
    cols = _axis_nodes(new_x, geometry.x0, geometry.dx, W)
    rstep = -1 if geometry.dy > 0 else 1    # tile rows run north to south, tile columns west to east
    cstep = -1 if geometry.dx < 0 else 1
    good = (rows >= 0).all(axis=1) & (cols >= 0).all(axis=1)
    good &= (rows == rows[:, :1] + rstep * np.arange(out_h)).all(axis=1) & (cols == cols[:, :1] + cstep * np.arange(out_w)).all(axis=1)
    if not good.all():
        k = int(np.argmin(good))
        raise ValueError(f"selective_tile(interpolate=False): window {k} {tuple(padded[k, [0, 1, 2, 3]])} does not cut the grid "
                         "at its nodes (its pixel centres are not node coordinates)")
    out = np.empty((len(padded), 4), dtype=np.int64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = rows[:, 0], cols[:, 0], rstep, cstep
    return out


def _plan(raster, window_bounds, padding, resolution, gapfiller, interpolate):
    """Everything selective_tile decides on the host: (mode, windows (n, 4) float64 or int64, resolution, out_h, out_w)."""
    if not isinstance(raster, Raster):
        raise TypeError("raster must be a Raster")
    w = _windows_array(window_bounds)
    padding = float(padding)
    if not np.isfinite(padding):
        raise ValueError("padding must be finite")
    g = raster.geometry
    if abs(g.dx) != abs(g.dy):
        raise ValueError(f"selective_tile needs square pixels, the raster has {abs(g.dx)} x {abs(g.dy)}")
    if resolution is None:
        resolution = abs(g.dx)
    resolution = float(resolution)
    if not (np.isfinite(resolution) and resolution > 0):
        raise ValueError(f"resolution must be positive, got {resolution}")
    if gapfiller is not None and not np.isfinite(np.float32(gapfiller)):
        raise ValueError(f"gapfiller must be a finite float32 number, got {gapfiller}")
    padded = np.stack([w[:, 0] - padding, w[:, 1] - padding, w[:, 2] + padding, w[:, 3] + padding], axis=1)
    out_h, out_w = tile_shape(w, padding, resolution)
    if out_h < 1 or out_w < 1:
        raise ValueError(f"empty tiles ({out_h} x {out_w}): the first window {tuple(w[0])} is smaller than one pixel of {resolution}")
    if interpolate:
        if raster.H < 2 or raster.W < 2:
            raise ValueError(f"bilinear interpolation needs at least 2 x 2 nodes, the raster is {raster.H} x {raster.W}")
        return 1, np.ascontiguousarray(padded), resolution, out_h, out_w
    if resolution != abs(g.dx):
        raise ValueError(f"selective_tile(interpolate=False) cannot resample: resolution {resolution} is not the raster's {abs(g.dx)}")
    return 0, np.ascontiguousarray(slice_windows(g, raster.shape, padded, out_h, out_w, resolution)), resolution, out_h, out_w


def _cut(raster, plan, gapfiller, fill_nan, out_ptr, stride, want_counts):
    """dbm_grid_tile on a planned cut; returns the per-window counts of masked values (host) if asked for."""
    mode, windows, resolution, out_h, out_w = plan
    grid = raster.device()
    ctx = grid.ctx
    n = len(windows)
    nodata = None if raster.nodata is None else C.byref(C.c_double(raster.nodata))
    fill = None if gapfiller is None else C.byref(C.c_float(gapfiller))
    counts = DeviceArray((n,), ctx, dtype=np.int32) if want_counts else None
    ctx.call("dbm_grid_tile", devptr(grid), raster.H, raster.W, f64ptr(raster.geometry.as_array()), devptr(windows), n, mode, resolution,
             out_h, out_w, nodata, fill, int(bool(fill_nan)), devptr(out_ptr), stride, devptr(counts))
    return counts.get() if want_counts else None


def selective_tile(raster, window_bounds, padding=0, resolution=None, gapfiller=None, interpolate=True, fill_nan=False, out=None,
                   channel=0):
    """data_prep.py:622-741 on a resident raster.  window_bounds: list of (xmin, ymin, xmax, ymax), each extended by `padding`;
    the tile size comes from the first window and `resolution` (default: the raster's).  interpolate=True resamples bilinearly
    to the windows' pixel centres (scipy's interpn rule), interpolate=False slices and demands that the windows cut the grid at
    its nodes (ValueError otherwise).  Values equal to the raster's nodata (numpy.ma.masked_values' band) become `gapfiller`;
    without one they stay and a warning lists the affected tiles.  fill_nan (an extension, not in the reference) treats NaN
    results -- outside the raster, a NaN node -- as missing too.  Returns a DeviceArray (n, 1, h, w), or fills channel
    `channel` of `out` (n, channels, h, w) and returns it."""
    plan = _plan(raster, window_bounds, padding, resolution, gapfiller, interpolate)
    n, (out_h, out_w) = len(plan[1]), plan[3:5]
    if out is None:
        if channel != 0:
            raise ValueError("channel needs an `out` array to select from")
        channels = 1
    else:
        if not isinstance(out, DeviceArray):
            raise TypeError("out must be a DeviceArray")
        if len(out.shape) != 4 or out.shape[0] != n or tuple(out.shape[2:]) != (out_h, out_w):
            raise ValueError(f"out has shape {out.shape}, the tiles need ({n}, channels, {out_h}, {out_w})")
        channels = out.shape[1]
        if not 0 <= int(channel) < channels:
            raise ValueError(f"channel {channel} outside out's {channels} channels")
    grid = raster.device()
    if out is None:
        out = DeviceArray((n, 1, out_h, out_w), grid.ctx)
    elif out.ctx is not grid.ctx:
        raise ValueError("selective_tile: out and the raster live on different contexts")
    can_mask = fill_nan or (raster.nodata is not None and not np.isnan(raster.nodata))
    counts = _cut(raster, plan, gapfiller, fill_nan, out.ptr + 4 * int(channel) * out_h * out_w, channels * out_h * out_w,
                  want_counts=can_mask and gapfiller is None)
    out.written()
    if counts is not None and counts.any():
        warnings.warn(f"selective_tile: tiles {np.flatnonzero(counts).tolist()} have missing data, try passing in a number to "
                      "'gapfiller'", stacklevel=2)
    return out


def bounds_from_flags(flags, geometry, shape, size, step):
    """data_prep.py:548-569 on the host: the (minx, miny, maxx, maxy) of every set flag, row-major (uly, ulx) from the north-west
    corner.  The raster's edges lie half a pixel outside its outermost nodes."""
    H, W = shape
    adx, ady = abs(geometry.dx), abs(geometry.dy)
    west = min(geometry.x0, geometry.x0 + (W - 1) * geometry.dx) - adx / 2
    north = max(geometry.y0, geometry.y0 + (H - 1) * geometry.dy) + ady / 2
    bounds = []
    for uly, ulx in np.argwhere(np.asarray(flags) != 0):
        left = west + int(ulx) * step * adx
        top = north - int(uly) * step * ady
        bounds.append((left, top - size * ady, left + size * adx, top))
    return bounds


def get_window_bounds(raster, height=36, width=36, step=3):
    """data_prep.py:501-572: the bounding boxes (minx, miny, maxx, maxy) of every height x width window, moved by `step`
    pixels from the north-west corner, that holds no NaN node."""
    if not isinstance(raster, Raster):
        raise TypeError("raster must be a Raster")
    height, width, step = int(height), int(width), int(step)
    if height != width:
        raise ValueError("get_window_bounds: the window must be square")
    if height % 2 != 0 or height < 2:
        raise ValueError("get_window_bounds: the window size must be an even number")
    if step < 1:
        raise ValueError("get_window_bounds: the step must be positive")
    if raster.H < height or raster.W < width:
        raise ValueError(f"get_window_bounds: the raster ({raster.H} x {raster.W}) is smaller than one window")
    grid = raster.device()
    ctx = grid.ctx
    ny, nx = (raster.H - height) // step + 1, (raster.W - width) // step + 1
    with ctx.scratch(ny * nx) as fdev:
        ctx.call("dbm_grid_filled_windows", devptr(grid), raster.H, raster.W, height, step, int(raster.geometry.dy > 0),
                 int(raster.geometry.dx < 0), devptr(fdev))
        flags = ctx.download(fdev, np.uint8, (ny, nx))
    return bounds_from_flags(flags, raster.geometry, raster.shape, height, step)


def _two_channels(velocity_x, velocity_y, window_bounds, padding, gapfiller):
    """W2: VX and VY at 500 m written through the window stride into the two channels of one (n, 2, h, w) array."""
    plan = _plan(velocity_x, window_bounds, padding, 500, gapfiller, True)
    ctx = velocity_x.device().ctx
    out = DeviceArray((len(plan[1]), 2, plan[3], plan[4]), ctx)
    selective_tile(velocity_x, window_bounds, padding=padding, resolution=500, gapfiller=gapfiller, out=out, channel=0)
    selective_tile(velocity_y, window_bounds, padding=padding, resolution=500, gapfiller=gapfiller, out=out, channel=1)
    return out


def get_deepbedmap_model_inputs(window_bound, bedmap2, rema, velocity_x, velocity_y, accumulation, padding=1000):
    """deepbedmap.py:164-200: one large tile each of BEDMAP2 (X, gaps -> -5000), REMA (W1), MEaSUREs ice velocity (W2: VX, VY
    at 500 m, gaps -> 0) and snow accumulation (W3, gaps -> 0) for the area (xmin, ymin, xmax, ymax), as DeviceArrays -- what
    get_deepbedmap_test_result, make_test_area_score and predict_tiled_resident take."""
    wb = [tuple(float(v) for v in window_bound)]
    if len(wb[0]) != 4:
        raise ValueError("window_bound must be (xmin, ymin, xmax, ymax)")
    for name, r in (("bedmap2", bedmap2), ("rema", rema), ("velocity_x", velocity_x), ("velocity_y", velocity_y), ("accumulation", accumulation)):
        if not isinstance(r, Raster):
            raise TypeError(f"{name} must be a Raster")
    X_tile = selective_tile(bedmap2, wb, padding=padding, gapfiller=-5000.0)
    W3_tile = selective_tile(accumulation, wb, padding=padding, gapfiller=0.0)
    W2_tile = _two_channels(velocity_x, velocity_y, wb, padding, 0.0)
    W1_tile = selective_tile(rema, wb, padding=padding)
    return X_tile, W1_tile, W2_tile, W3_tile


def tile_training_set(highres, bedmap2, rema, velocity_x, velocity_y, accumulation):
    """data_prep.py:757-771 and 880-911: `highres` is a list of (Raster, window_bounds) -- the groundtruth grids and the windows
    selected on each.  Y is sliced from them (interpolate=False, no padding); X, W1, W2 (500 m, VX and VY) and W3 are cut for
    the concatenated windows with 1000 m of padding.  Returns {"X", "W1", "W2", "W3", "Y"} of DeviceArrays, what
    get_train_dev_iterators takes."""
    if len(highres) < 1:
        raise ValueError("tile_training_set needs at least one (Raster, window_bounds) pair")
    plans = [_plan(r, w, 0, None, None, False) for r, w in highres]
    shapes = {(p[3], p[4]) for p in plans}
    if len(shapes) != 1:
        raise ValueError(f"the groundtruth grids give tiles of different shapes: {sorted(shapes)}")
    (h, w), = shapes
    for name, r in (("bedmap2", bedmap2), ("rema", rema), ("velocity_x", velocity_x), ("velocity_y", velocity_y), ("accumulation", accumulation)):
        if not isinstance(r, Raster):
            raise TypeError(f"{name} must be a Raster")
    windows = np.concatenate([_windows_array(wb) for _, wb in highres])
    ctx = highres[0][0].device().ctx
    Y = DeviceArray((len(windows), 1, h, w), ctx)
    done = 0
    for (raster, _), plan in zip(highres, plans):
        if raster.device().ctx is not ctx:
            raise ValueError("tile_training_set: the groundtruth grids live on different contexts")
        can_mask = raster.nodata is not None and not np.isnan(raster.nodata)
        counts = _cut(raster, plan, None, False, Y.ptr + 4 * done * h * w, h * w, want_counts=can_mask)
        if counts is not None and counts.any():
            warnings.warn(f"tile_training_set: groundtruth tiles {(done + np.flatnonzero(counts)).tolist()} have missing data", stacklevel=2)
        done += len(plan[1])
    Y.written()
    return {"X": selective_tile(bedmap2, windows, padding=1000),
            "W1": selective_tile(rema, windows, padding=1000),
            "W2": _two_channels(velocity_x, velocity_y, windows, 1000, None),
            "W3": selective_tile(accumulation, windows, padding=1000),
            "Y": Y}


def fill_gaps(fine, coarse, inplace=False):
    """data_prep.py:838-877 (REMA at 100 m patched from the 200 m mosaic) on resident rasters: every node of `fine` that is NaN or
    equal to `fine.nodata` takes the value `selective_tile(coarse, [bounds of fine], resolution=fine.dx)` has at that node -- this
    package's bilinear rule (scipy's interpn), NaN outside `coarse`, NOT GDAL's mask-renormalised resampler; nodes
    with data keep their bits.  `fine` must be north-up with square pixels.  Returns a Raster with fine's geometry and nodata: a new
    plane, or with inplace=True `fine` itself, patched where it lies."""
    if not isinstance(fine, Raster) or not isinstance(coarse, Raster):
        raise TypeError("fine and coarse must be Rasters")
    g = fine.geometry
    if not (g.dx > 0 and g.dy < 0 and g.dx == -g.dy):
        raise ValueError(f"fill_gaps needs a north-up fine raster with square pixels, it has dx {g.dx}, dy {g.dy}")
    if coarse.H < 2 or coarse.W < 2:
        raise ValueError(f"bilinear interpolation needs at least 2 x 2 nodes, the coarse raster is {coarse.H} x {coarse.W}")
    west, north = g.x0 - g.dx / 2, g.y0 + g.dx / 2   # the raster's edges lie half a pixel outside its outermost nodes
    bounds = (west, north - fine.H * g.dx, west + fine.W * g.dx, north)
    if tile_shape([bounds], 0, g.dx) != fine.shape:
        raise ValueError(f"fill_gaps: the bounds {bounds} of the fine raster do not give its shape {fine.shape} at resolution {g.dx}")
    src, cgrid = fine.device(), coarse.device()
    ctx = src.ctx
    if cgrid.ctx is not ctx:
        raise ValueError("fill_gaps: fine and coarse live on different contexts")
    out = src if inplace else DeviceArray(src.shape, ctx)
    nodata = None if fine.nodata is None else C.byref(C.c_double(fine.nodata))
    ctx.call("dbm_grid_fill_gaps", devptr(src), fine.H, fine.W, f64ptr(np.asarray(bounds, dtype=np.float64)), float(g.dx), nodata, devptr(cgrid),
             coarse.H, coarse.W, f64ptr(coarse.geometry.as_array()), devptr(out))
    out.written()
    return fine if inplace else Raster(out, g, nodata=fine.nodata)
