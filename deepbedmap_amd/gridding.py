"""From a survey's point cloud to the `points` table and the 250 m ground-truth raster (reference data_prep.py:322-334, 353-378,
406-407).

The reference reprojects longitude / latitude with pyproj (`filters.reprojection` of ascii_to_xyz), takes the cloud's bounding box
with `gmt info -I` (get_region) and thins the cloud with `gmt.blockmedian` before gridding it (xyz_to_grid).  Those three passes over
the largest tables of the workflow -- tens of millions of float64 rows per survey -- run here on the GPU (dbm_points_polar_stereographic,
dbm_points_region, dbm_points_blockmedian, include/dbm.h); what they produce is what `grdtrack`, `DevicePoints`, `make_test_area_score`
(the table) and `Raster`, `tile_training_set` (the raster) take.  Semantics, the tie rule and what is unverified against GMT: DESIGN.md
"Gridding point clouds".

The second half of xyz_to_grid (data_prep.py:409-441: `gmt.surface(T=0.35, M="3c")`, then `grdsample -T`) runs on the GPU as well:
`tension_surface` interpolates the block-median raster with a tension spline (dbm_grid_tension_surface: float64 conjugate gradients on
the device), `mask_far_from_data` blanks nodes further than three cells from data (dbm_grid_distance_mask), `to_pixel_registration`
resamples gridline -> pixel (dbm_grid_to_pixel) and `xyz_to_grid` chains all four stages without leaving the device.  The surface is this
project's own, completely defined one -- constraints on nodes, natural edges, a residual stopping rule -- NOT a reproduction of GMT
`surface`: DESIGN.md "Tension surface" lists every difference.  NOT built: `gmt info -Is<inc>`.  (The CSV reading of
ascii_to_xyz, the step in front of these, is deepbedmap_amd/ascii_table.py.)  No CPU fallback: without a GPU every call that computes raises DbmError.
"""
import ctypes as C

import numpy as np

from . import _lib
from .resident import DeviceArray, DevicePoints, GridGeometry, devptr, f64ptr, points_table, resident_plane, shape_of
from .resident import to_device  # noqa: F401  (re-exported)

# EPSG method 9829 parameters {a, 1/f, latitude of true scale, longitude of origin, false easting, false northing}
EPSG3031 = (6378137.0, 298.257223563, -71.0, 0.0, 0.0, 0.0)
SRS_PAIRS = {("EPSG:4326", "EPSG:3031"): EPSG3031}   # (in_srs, out_srs), upper case, that `reproject` converts

# include/dbm.h: threads per workgroup of the point passes; the largest block population of each size class of the block medians'
# selection, in ascending order (8 lanes, 32 lanes, a wavefront, a workgroup sorting in LDS; larger blocks: selection out of global
# memory).  tests/test_gridding_host.py holds them to the header.
POINTS_THREADS = 256
BLOCKMEDIAN_SUB8 = 8
BLOCKMEDIAN_SUB32 = 32
BLOCKMEDIAN_WAVE = 64
BLOCKMEDIAN_LDS = 2048
BLOCKMEDIAN_CLASS_BOUNDARIES = (BLOCKMEDIAN_SUB8, BLOCKMEDIAN_SUB32, BLOCKMEDIAN_WAVE, BLOCKMEDIAN_LDS)


def _like(points, values):
    """`values` (n, ncol) as the kind of object `points` is: a DataFrame keeps its index and its other columns"""
    if hasattr(points, "columns"):
        out = points.copy()
        for k, name in enumerate(["x", "y", "z"][:values.shape[1]]):
            out[name] = values[:, k]
        return out
    return values


def _fmt(v):
    """a coordinate as GMT prints it (%.16g, negative zero as 0)"""
    return format(float(v) + 0.0, ".16g")


def parse_region(region):
    """'xmin/xmax/ymin/ymax' or a 4-sequence -> (xmin, xmax, ymin, ymax) floats; finite, max >= min"""
    if isinstance(region, str):
        parts = region.strip().split("/")
        if len(parts) != 4:
            raise ValueError(f"region must be 'xmin/xmax/ymin/ymax', got {region!r}")
        try:
            vals = tuple(float(p) for p in parts)
        except ValueError:
            raise ValueError(f"region must be 'xmin/xmax/ymin/ymax' with four numbers, got {region!r}") from None
    else:
        try:
            vals = tuple(float(v) for v in region)
        except (TypeError, ValueError):
            raise ValueError(f"region must be a string or four numbers, got {region!r}") from None
        if len(vals) != 4:
            raise ValueError(f"region must hold four numbers, got {len(vals)}")
    if not all(np.isfinite(v) for v in vals):
        raise ValueError(f"region must be finite, got {region!r}")
    if vals[1] < vals[0] or vals[3] < vals[2]:
        raise ValueError(f"region must have xmax >= xmin and ymax >= ymin, got {region!r}")
    return vals


def _spacing(spacing):
    try:
        s = float(spacing)
    except (TypeError, ValueError):
        raise ValueError(f"the spacing must be a positive number, got {spacing!r}") from None
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"the spacing must be positive and finite, got {spacing!r}")
    return s


def block_shape(region, spacing):
    """(H, W) of the gridline-registered blocks of `spacing` over `region`, the north / east edge fitted to the spacing (GMT's `+e`):
    round((max - min) / spacing) + 1 per axis"""
    xmin, xmax, ymin, ymax = parse_region(region)
    s = _spacing(spacing)
    H, W = int(np.rint((ymax - ymin) / s)) + 1, int(np.rint((xmax - xmin) / s)) + 1
    if H * W >= 2 ** 31:
        raise ValueError(f"{H} x {W} blocks: the grid must stay below 2^31 blocks")
    return H, W


def block_geometry(region, spacing):
    """GridGeometry of the block raster: node (0, 0) is the north-west node (xmin, ymax), rows run south"""
    xmin, _, ymin, ymax = parse_region(region)
    s = _spacing(spacing)
    H, _ = block_shape(region, spacing)
    span = float(H - 1) * s
    return GridGeometry(x0=xmin, y0=ymax if span == ymax - ymin else ymin + span, dx=s, dy=-s, registration="gridline")


def reproject(points, in_srs="EPSG:4326", out_srs="EPSG:3031", ctx=None):
    """The `filters.reprojection` step of ascii_to_xyz (data_prep.py:322-334): columns x, y = longitude, latitude in degrees become
    easting, northing in metres (polar stereographic, EPSG method 9829 variant B, south-pole case); further columns are kept.  Only
    EPSG:4326 -> EPSG:3031 is supported.  Returns the kind of object it was given: array -> array, DataFrame -> DataFrame; a DevicePoints
    is converted IN PLACE and returned.  A latitude outside [-90, 0] is refused with ValueError before anything is converted (a resident
    table is inspected on the device, over its rows whose x, y[, z] are all finite: the rows every later stage keeps)."""
    key = (str(in_srs).upper(), str(out_srs).upper())
    if key not in SRS_PAIRS:
        raise ValueError(f"reproject: only {sorted(SRS_PAIRS)} are supported, got {in_srs!r} -> {out_srs!r}")
    proj = f64ptr(np.array(SRS_PAIRS[key], dtype=np.float64))
    if isinstance(points, DevicePoints):
        # the latitudes' range, on the device: with an increment of 2^-20 degrees (-90 is a multiple) the outward rounding of
        # dbm_points_region moves ymin below -90 iff a latitude lies below it and ymax above 0 iff a latitude lies above it
        (_, _, lat_lo, lat_hi), count = region_of(points, 2.0 ** -20)
        if count and (lat_lo < -90.0 or lat_hi > 0.0):
            raise ValueError("reproject: latitudes must lie in [-90, 0] (the south-pole case of the polar stereographic projection)")
        points.ctx.call("dbm_points_polar_stereographic", devptr(points), points.n, points.ncol, proj, devptr(points), _lib.DEVICE_PTRS)
        return points
    pts = points_table(points, lambda c: c >= 2, "reproject: points must be (n, >= 2) longitude, latitude[, ...]")
    lat = pts[:, 1]
    if np.any(lat[np.isfinite(lat)] > 0.0) or np.any(lat[np.isfinite(lat)] < -90.0):
        raise ValueError("reproject: latitudes must lie in [-90, 0] (the south-pole case of the polar stereographic projection)")
    ctx = ctx or _lib.default_context()
    out = np.empty_like(pts)
    ctx.call("dbm_points_polar_stereographic", devptr(pts), pts.shape[0], pts.shape[1], proj, devptr(out), 0)
    return _like(points, out)


def region_of(xyz_data, round_increment=250, ctx=None):
    """((xmin, xmax, ymin, ymax) moved outward to multiples of round_increment, number of rows with finite x, y[, z]); four NaNs and 0
    without such a row"""
    inc = _spacing(round_increment)
    region, count = np.empty(4, dtype=np.float64), C.c_int64(0)
    if isinstance(xyz_data, DevicePoints):
        ctx = xyz_data.ctx
        with ctx.scratch(64) as out:
            ctx.call("dbm_points_region", devptr(xyz_data), xyz_data.n, xyz_data.ncol, inc, devptr(out), devptr(out + 32), _lib.DEVICE_PTRS)
            host = ctx.download(out, np.float64, 5)
        return tuple(float(v) for v in host[:4]), int(host[4:].view(np.int64)[0])
    pts = points_table(xyz_data, lambda c: c >= 2, "get_region: the table must be (n, >= 2) x, y[, z]")
    ctx = ctx or _lib.default_context()
    ctx.call("dbm_points_region", devptr(pts), pts.shape[0], pts.shape[1], inc, devptr(region), C.byref(count), 0)
    return tuple(float(v) for v in region), int(count.value)


def get_region(xyz_data, round_increment=250, ctx=None):
    """get_region (data_prep.py:353-378) as `gmt info -I<inc>` answers it -- NOT `-Is<inc>`, the variant the reference calls, which
    widens the box further to dimensions that suit GMT surface (not built; it only ever widens): the bounding box of the rows with
    finite x, y and z moved outward to multiples of round_increment, as the string 'xmin/xmax/ymin/ymax' that GMT prints and -R takes.
    xyz_data: array, DataFrame with columns x, y, z, or DevicePoints."""
    region, count = region_of(xyz_data, round_increment, ctx)
    if count == 0:
        raise ValueError("get_region: the table has no row with finite coordinates")
    return "/".join(_fmt(v) for v in region)


def _blockmedian(table, region, spacing, want_grid, want_counts, ctx):
    """(table (m, 3), grid DeviceArray or None, counts int32 (H, W) or None, geometry)"""
    r4 = np.array(parse_region(region), dtype=np.float64)
    s = _spacing(spacing)
    H, W = block_shape(r4, s)
    geometry = block_geometry(r4, s)
    if isinstance(table, DevicePoints):
        if table.ncol != 3:
            raise ValueError(f"blockmedian: the table must be (n, 3) x, y, z; got {table.ncol} columns")
        ctx, n, pts = table.ctx, table.n, None
    else:
        pts = points_table(table, lambda c: c == 3, "blockmedian: the table must be (n, 3) x, y, z")
        ctx, n = ctx or _lib.default_context(), pts.shape[0]
    grid = DeviceArray((H, W), ctx) if want_grid else None
    cdev = DeviceArray((H, W), ctx, dtype=np.int32) if want_counts else None
    cap = max(min(n, H * W), 1)
    m = C.c_int64(0)
    if pts is None:
        src, dst, flags = table, DeviceArray((cap, 3), ctx, dtype=np.float64), _lib.DEVICE_PTRS
    else:
        src, dst, flags = pts, np.empty((cap, 3), dtype=np.float64), 0
    ctx.call("dbm_points_blockmedian", devptr(src), n, f64ptr(r4), s, devptr(dst), cap, C.byref(m), devptr(grid), devptr(cdev), flags)
    out = ctx.download(dst.ptr, np.float64, (int(m.value), 3)) if pts is None else dst[:int(m.value)].copy()
    counts = cdev.get() if want_counts else None
    if grid is not None:
        grid.written()
    return out, grid, counts, geometry


def blockmedian(table, region, spacing=250, ctx=None):
    """`gmt.blockmedian(table=table, region=region, spacing=f"{spacing}+e")` (data_prep.py:406-407): per non-empty block of the
    gridline-registered grid over `region` the medians of x, of y and of z, in the order blockmedian prints (north row first, west to
    east).  table: (n, 3) array, DataFrame with columns x, y, z, or DevicePoints; region: 'xmin/xmax/ymin/ymax' or four numbers.
    Returns (m, 3) float64, or a DataFrame with columns x, y, z if given one."""
    out, _, _, _ = _blockmedian(table, region, spacing, False, False, ctx)
    if hasattr(table, "columns"):
        return type(table)({"x": out[:, 0], "y": out[:, 1], "z": out[:, 2]})
    return out


def blockmedian_grid(points, region, spacing=250, counts=False, download=True, ctx=None):
    """The block medians of z as a raster: (grid (H, W) float32 with NaN in empty blocks, GridGeometry[, counts (H, W) int32]).  With
    download=False the grid is a DeviceArray, used in place by `Raster`, `grdtrack`, `standard_deviation_2d` and `tension_surface`.
    This is the cloud binned, NOT interpolated: `tension_surface` / `xyz_to_grid` fill the empty blocks."""
    _, grid, cnt, geometry = _blockmedian(points, region, spacing, True, bool(counts), ctx)
    g = grid.get() if download else grid
    return (g, geometry, cnt) if counts else (g, geometry)


def _surface_arguments(shape, tension, tol, max_iter):
    H, W = (int(v) for v in shape)
    if H < 3 or W < 3:
        raise ValueError(f"tension_surface: the grid needs at least 3 x 3 nodes, got {H} x {W}")
    if H * W >= 2 ** 31:
        raise ValueError(f"tension_surface: {H} x {W} nodes: the grid must stay below 2^31 nodes")
    tension, tol = float(tension), float(tol)
    if not (0.0 < tension <= 1.0):
        raise ValueError(f"tension_surface: the tension must lie in (0, 1], got {tension}")
    if not (0.0 < tol < 1.0):
        raise ValueError(f"tension_surface: tol must lie in (0, 1), got {tol}")
    if int(max_iter) != max_iter or not (1 <= int(max_iter) <= 10 ** 6):
        raise ValueError(f"tension_surface: max_iter must be an integer in 1..10^6, got {max_iter!r}")
    return H, W, tension, tol, int(max_iter)


def tension_surface(grid, tension=0.35, tol=1e-9, max_iter=20000, download=True, ctx=None):
    """The `gmt.surface(T=tension)` step of xyz_to_grid (data_prep.py:410-419) as this project defines it (DESIGN.md "Tension surface",
    include/dbm.h dbm_grid_tension_surface): the minimiser of (1 - T) bending + T stretching energy of the differences that fit inside
    the grid, equal to `grid` on its non-NaN nodes (constraints ON nodes, natural edges; NOT GMT's off-node constraints and edge rows).
    grid: (H, W) array or DeviceArray with NaN in the free nodes -- what `blockmedian_grid` returns.  Returns (surface, info): surface
    a float32 array, or a DeviceArray with download=False; info = {"iterations", "residual" (final |r| / |b|), "constraints", "free"}.
    Raises ValueError for arguments out of range, DbmError (code 1) for a grid without data and DbmError (code 10) if the conjugate
    gradients have not reached tol within max_iter."""
    shape = shape_of(grid)
    if len(shape) != 2:
        raise ValueError(f"tension_surface: the grid must be (H, W); got {tuple(shape)}")
    H, W, tension, tol, max_iter = _surface_arguments(shape, tension, tol, max_iter)
    dgrid, ctx = resident_plane(grid, ctx, "tension_surface")
    out = DeviceArray((H, W), ctx)
    info = np.zeros(4, dtype=np.float64)
    ctx.call("dbm_grid_tension_surface", devptr(dgrid), H, W, tension, tol, max_iter, devptr(out), f64ptr(info))
    out.written()
    report = {"iterations": int(info[0]), "residual": float(info[1]), "constraints": int(info[2]), "free": int(info[3])}
    return (out.get() if download else out), report


def _mask_radius(radius):
    if int(radius) != radius or not (0 <= int(radius) <= 32):
        raise ValueError(f"mask_far_from_data: the radius must be an integer number of cells in 0..32, got {radius!r}")
    return int(radius)


def mask_far_from_data(surface, data, radius=3):
    """The `M="3c"` of `gmt.surface` (data_prep.py:416): NaN wherever no non-NaN node of `data` lies within `radius` cells (Euclidean
    node-to-node distance: this project's reading of GMT's `c` unit).  surface, data: (H, W) arrays or DeviceArrays.  A DeviceArray
    `surface` is masked IN PLACE and returned; an array is copied and a masked float32 array returned."""
    radius = _mask_radius(radius)
    sshape, dshape = shape_of(surface), shape_of(data)
    if len(sshape) != 2 or tuple(sshape) != tuple(dshape):
        raise ValueError(f"mask_far_from_data: surface and data must have the same (H, W) shape; got {tuple(sshape)} and {tuple(dshape)}")
    if surface is data:
        raise ValueError("mask_far_from_data: the surface must not be the data raster")
    ctx = surface.ctx if isinstance(surface, DeviceArray) else (data.ctx if isinstance(data, DeviceArray) else None)
    dsurf, ctx = resident_plane(surface, ctx, "mask_far_from_data")
    ddata, _ = resident_plane(data, ctx, "mask_far_from_data")
    if ddata.ctx is not dsurf.ctx:
        raise ValueError("mask_far_from_data: the surface and the data live on different contexts")
    H, W = (int(v) for v in sshape)
    ctx.call("dbm_grid_distance_mask", devptr(ddata), devptr(dsurf), H, W, radius)
    dsurf.written()
    return dsurf if isinstance(surface, DeviceArray) else dsurf.get()


def to_pixel_registration(grid, geometry, threshold=0.5, download=None, ctx=None):
    """`gmt grdsample -T` (data_prep.py:420-441): the gridline-registered (H, W) grid resampled at its cell centres with `grdtrack`'s
    bicubic interpolant (ghost nodes, NaN rule and threshold included).  Returns (grid (H - 1, W - 1), GridGeometry(x0 + dx / 2,
    y0 + dy / 2, dx, dy, "pixel")): a DeviceArray if given one (download=None) or with download=False, else a float32 array."""
    if not isinstance(geometry, GridGeometry):
        raise TypeError("geometry must be a GridGeometry")
    if geometry.registration != "gridline":
        raise ValueError("to_pixel_registration: the grid must be gridline-registered")
    if not (0.0 < float(threshold) <= 1.0):
        raise ValueError(f"threshold must lie in (0, 1], got {threshold}")
    shape = shape_of(grid)
    if len(shape) != 2 or shape[0] < 2 or shape[1] < 2:
        raise ValueError(f"to_pixel_registration: the grid must be (H, W) with at least 2 x 2 nodes; got {tuple(shape)}")
    if download is None:
        download = not isinstance(grid, DeviceArray)
    dgrid, ctx = resident_plane(grid, ctx, "to_pixel_registration")
    H, W = dgrid.shape
    out = DeviceArray((H - 1, W - 1), ctx)
    ctx.call("dbm_grid_to_pixel", devptr(dgrid), H, W, float(threshold), devptr(out))
    out.written()
    pixel = GridGeometry(x0=geometry.x0 + geometry.dx / 2, y0=geometry.y0 + geometry.dy / 2, dx=geometry.dx, dy=geometry.dy,
                         registration="pixel")
    return (out.get() if download else out), pixel


def xyz_to_grid(xyz_data, region, spacing=250, tension=0.35, mask_cell_radius=3, download=True, ctx=None, outfile=None):
    """xyz_to_grid (data_prep.py:381-441): block medians on the gridline grid of `spacing` over `region`
    (`blockmedian_grid`), the tension surface through them (`tension_surface`, its defaults for tol and max_iter), the distance mask
    (`mask_far_from_data`; mask_cell_radius=None skips it) and the pixel-registered resampling (`to_pixel_registration`).  Nothing
    leaves the device between the stages.  xyz_data: (n, 3) array, DataFrame with columns x, y, z, or DevicePoints.  Returns
    (grid (H - 1, W - 1), GridGeometry, pixel-registered): a float32 array, or a DeviceArray with download=False.  outfile
    (data_prep.py:410-441): the result is also written as a netCDF-4 grid of that path, from the device and before any download
    (`netcdf.write_netcdf_resident`: variable z, y ascending as GMT writes it, chunked, shuffled, deflated on the GPU); the return
    value is the same.  The result is this project's surface, not GMT's (DESIGN.md "Tension surface")."""
    if mask_cell_radius is not None:
        mask_cell_radius = _mask_radius(mask_cell_radius)
    _surface_arguments(block_shape(region, spacing), tension, 1e-9, 20000)
    medians, geometry = blockmedian_grid(xyz_data, region, spacing, download=False, ctx=ctx)
    surface, _ = tension_surface(medians, tension=tension, download=False)
    if mask_cell_radius is not None:
        mask_far_from_data(surface, medians, mask_cell_radius)
    if outfile is None:
        return to_pixel_registration(surface, geometry, download=download)
    from .netcdf import write_netcdf_resident

    grid, pixel = to_pixel_registration(surface, geometry, download=False)
    H, W = grid.shape
    west, north = pixel.x0 - pixel.dx / 2, pixel.y0 - pixel.dy / 2     # (dy < 0: the grid is north-up)
    write_netcdf_resident(outfile, (west, north + H * pixel.dy, west + W * pixel.dx, north), grid, y_ascending=True)
    return (grid.get() if download else grid), pixel
