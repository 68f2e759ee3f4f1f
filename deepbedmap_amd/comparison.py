"""The grids DeepBedMap is compared against (reference deepbedmap.py:318-356, 505-626; paper_figures.py:847-931).

The reference's headline number is `rmse_deepbedmap3 - rmse_cubicbedmap` (deepbedmap.py:622-626): the along-track error of the
model's grid against that of BEDMAP2 upsampled x4 with `skimage.transform.rescale(order=3)`; its second comparison is terrain
roughness, a rolling-window standard deviation of each product grid (`standard_deviation_2d`).  Both are whole-plane passes over
grids that already lie in HBM and run there (dbm_grid_rescale, dbm_grid_rolling_std, include/dbm.h): a DeviceArray -- the canvas of
`predict_tiled_resident(download=False)`, a `Raster`'s grid -- is read in place and the result is a DeviceArray that `grdtrack`
samples in place.  Semantics: DESIGN.md "Comparison grids" (`rescale` is the scipy.ndimage chain of current scikit-image
releases; the reference's pinned 0.15 interpolates differently).  No CPU fallback: without a GPU every call raises DbmError.
"""
import numpy as np

from .evaluation import describe_errors, distribution_arguments, grdtrack
from .resident import DeviceArray, DevicePoints, GridGeometry, devptr, plane_shape, points_table, resident_plane
from .resident import to_device  # noqa: F401  (re-exported)


def rescale_output_shape(shape, scale):
    """(out_h, out_w) = round(scale * (H, W)) with NumPy's round; scale a number or one per axis"""
    try:
        s = np.asarray(scale, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f"scale must be a number or a pair of numbers, got {scale!r}")
    if s.shape not in ((), (2,)):
        raise ValueError(f"scale must be a number or one number per axis, got shape {s.shape}")
    s = np.broadcast_to(s, (2,))
    if not np.all(np.isfinite(s)) or np.any(s <= 0):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    out = np.round(s * np.asarray(shape, dtype=np.float64))
    if np.any(out < 1):
        raise ValueError(f"scale {scale!r} leaves no output node of a {shape[0]} x {shape[1]} grid")
    return int(out[0]), int(out[1])


def rescale(image, scale, order=1, anti_aliasing=True, clip=True, as_int=False, ctx=None):
    """`skimage.transform.rescale(image, scale, order=order, mode="reflect", anti_aliasing=anti_aliasing, clip=clip,
    preserve_range=True)` on the GPU, as current scikit-image computes it; as_int: the reference's `.astype(np.int32)` on the way
    in (deepbedmap.py:324, 349).  image: NumPy array or DeviceArray of shape (H, W), (1, H, W) or (1, 1, H, W); returns a
    DeviceArray of the same rank holding round(scale * (H, W)) nodes.  Orders 1 and 3; H, W >= 2; NaN nodes are outside the contract."""
    H, W = plane_shape(image)
    if order not in (1, 3):
        raise ValueError(f"order must be 1 (linear) or 3 (cubic), got {order!r}")
    if H < 2 or W < 2:
        raise ValueError(f"rescale needs at least 2 x 2 nodes, the grid is {H} x {W}")
    out_h, out_w = rescale_output_shape((H, W), scale)
    lead = tuple(image.shape)[:-2]
    src, ctx = resident_plane(image, ctx)
    out = DeviceArray(lead + (out_h, out_w), ctx)
    ctx.call("dbm_grid_rescale", devptr(src), H, W, out_h, out_w, int(order), int(bool(anti_aliasing)), int(bool(clip)), int(bool(as_int)),
             devptr(out))
    return out.written()


def standard_deviation_2d(grid, window_length, ctx=None):
    """paper_figures.py:847-867: the standard deviation (ddof 0) of each node's centred window_length x window_length neighbourhood,
    NaN nodes and nodes beyond the edges skipped, NaN where the window holds no valid node.  window_length odd, 1..63.  grid: NumPy
    array or DeviceArray of shape (H, W), (1, H, W) or (1, 1, H, W); returns a DeviceArray of the same shape."""
    H, W = plane_shape(grid)
    if isinstance(window_length, bool) or not isinstance(window_length, (int, np.integer)):
        raise TypeError(f"window_length must be an integer, got {window_length!r}")
    if window_length % 2 != 1 or not 1 <= window_length <= 63:
        raise ValueError(f"window_length must be odd and lie in 1..63, got {window_length}")
    if H < 1 or W < 1:
        raise ValueError(f"empty grid ({H} x {W})")
    src, ctx = resident_plane(grid, ctx)
    out = DeviceArray(tuple(grid.shape), ctx)
    ctx.call("dbm_grid_rolling_std", devptr(src), H, W, int(window_length), devptr(out))
    return out.written()


def cubic_bedmap(X_tile, ctx=None):
    """deepbedmap.py:323-332 in one call: the interior [1:-1, 1:-1] of the (1, 1, h, w) BEDMAP2 tile, cast to int32, upsampled x4 with
    order 3 -> DeviceArray (1, 1, 4 (h - 2), 4 (w - 2)): node for node the model's output for that tile, on the geometry
    `GridGeometry.from_bounds(window_bound, 4 (h - 2), 4 (w - 2))`."""
    shape = tuple(int(s) for s in X_tile.shape)
    if len(shape) != 4 or shape[:2] != (1, 1):
        raise ValueError(f"X_tile must be (1, 1, h, w), got {shape}")
    h, w = shape[2:]
    if h < 4 or w < 4:
        raise ValueError(f"X_tile needs an interior of at least 2 x 2 nodes, got {h} x {w}")
    if isinstance(X_tile, DeviceArray):
        ctx = X_tile.ctx
        inner = DeviceArray((h - 2, w - 2), ctx)
        ctx.call("dbm_memcpy2d_d2d", devptr(inner), 4 * (w - 2), devptr(X_tile.ptr + 4 * (w + 1)), 4 * w, 4 * (w - 2), h - 2)
        inner.written()
    else:
        inner = np.asarray(X_tile, dtype=np.float32)[0, 0, 1:-1, 1:-1]
    out = rescale(inner, 4, order=3, anti_aliasing=True, clip=True, as_int=True, ctx=ctx)
    out.shape = (1, 1) + out.shape
    return out


def _grids_and_points(who, points, grids, ctx):
    """[(name, grid, GridGeometry)] of a {name: (grid, GridGeometry)} mapping, and the points (x, y, z) as DevicePoints: a host table is
    uploaded once, to the context of the first resident grid"""
    if not hasattr(grids, "items"):
        raise TypeError("grids must map a name to (grid, GridGeometry)")
    entries = []
    for name, entry in grids.items():
        if not isinstance(entry, (tuple, list)) or len(entry) != 2 or not isinstance(entry[1], GridGeometry):
            raise TypeError(f"grids[{name!r}] must be (grid, GridGeometry)")
        plane_shape(entry[0])
        entries.append((name, entry[0], entry[1]))
    if (points.ncol if isinstance(points, DevicePoints) else points_table(points).shape[1]) != 3:
        raise ValueError(f"{who}: the points need a z column")
    if not isinstance(points, DevicePoints):
        for _, g, _ in entries:
            if ctx is None and isinstance(g, DeviceArray):
                ctx = g.ctx
        points = DevicePoints(points, ctx)   # uploaded once, sampled by every grid
    return entries, points


def compare_on_tracks(points, grids, interpolation="bicubic", threshold=0.5, ctx=None):
    """The table of deepbedmap.py:550-574, 622-626: every product grid sampled at the same survey points (x, y, z) and its
    along-track error summarised.  grids: {name: (grid, GridGeometry)}, grid a NumPy array or a DeviceArray (read in place);
    points: array / DataFrame (uploaded once) or DevicePoints.  Returns {name: TrackStats}; the reference's headline number is
    result["deepbedmap3"].rmse - result["cubicbedmap"].rmse.  The quartile rows of the table and the histograms: describe_on_tracks."""
    entries, points = _grids_and_points("compare_on_tracks", points, grids, ctx)
    return {name: grdtrack(points, g, geom, interpolation=interpolation, threshold=threshold, return_values=False, ctx=points.ctx)[1]
            for name, g, geom in entries}


def describe_on_tracks(points, grids, interpolation="bicubic", threshold=0.5, percentiles=(0.25, 0.5, 0.75), bins=None, range=None,
                       ctx=None):
    """compare_on_tracks with the whole table of deepbedmap.py:550-563 -- `describe()`'s eight rows per grid -- and, with `bins`, the
    error histograms of deepbedmap.py:575-608 (`hist(column="error", bins=25)`; range None: each grid's own (min, max), as pandas
    plots them).  The points are uploaded once for all grids; z_interpolated never leaves the device.  Returns {name:
    TrackDescription}; `.as_dict()` is `describe()`, `.histogram` (counts, edges) or None."""
    distribution_arguments(percentiles, bins, range)
    entries, points = _grids_and_points("describe_on_tracks", points, grids, ctx)
    return {name: describe_errors(points, g, geom, interpolation=interpolation, threshold=threshold, percentiles=percentiles,
                                  ctx=points.ctx, bins=bins, range=range)
            for name, g, geom in entries}
