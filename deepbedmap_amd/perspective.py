"""The 3-D perspective view of the DEM where it lies (reference deepbedmap.py:258-295, `plot_3d_view`: `fig.grdview(grid=..., surftype="sim",
plane=zmin, zscale=0.01, perspective=[202.5, 60])`; :465-501 the four-panel figure of every test-area run; paper_figures.py:624-660 and
:1126-1166).

The reference hands the grid to GMT's `grdview`.  Here the resident plane, draped with the image `relief_image` made of it, is rendered
by dbm_grid_perspective: a hidden-surface render of the height field under an orthographic view, one thread per pixel, and the image is
written by `write_png_resident`; only the compressed bytes cross PCIe.  Host side: the view's angles (`View`), the frame that holds the
scene (`perspective_frame`), the public calls (`perspective_image`, `plot_3d_view`) and the host entry of the same bytes
(`perspective_image_host`, dbm_grid_perspective_host: the kernel's own cell function under a plain traversal).

The rule is this project's own and is stated in DESIGN.md 6o; GMT's pixels are NOT claimed.  Mesh lines, axes, text and subplots stay
out of scope.  No CPU fallback: the device calls raise DbmError without a GPU; `perspective_image_host`, `View` and `perspective_frame`
need none.
"""
import dataclasses
import math
import os

import numpy as np

from . import _lib
from .resident import DeviceArray, GridGeometry, devptr, plane_shape, to_device

_QUADRANTS = ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))   # (sin, cos) at 0, 90, 180, 270 degrees


def sincos_degrees(angle):
    """(sin, cos) of an angle in degrees; at the multiples of 90 degrees exactly 0 and +-1, so that a ray along a grid axis has a ground
    component that IS zero."""
    d = math.fmod(float(angle), 360.0)
    if d < 0.0:
        d += 360.0
    q = d / 90.0
    if q == math.floor(q):
        return _QUADRANTS[int(q) % 4]
    return math.sin(math.radians(d)), math.cos(math.radians(d))


@dataclasses.dataclass(frozen=True)
class View:
    """Where the viewer stands and how heights are drawn (the reference's `perspective=[azimuth, elevation]`, `plane=zmin` and
    `zscale`): azimuth in degrees clockwise from north, elevation in degrees above the horizon, 1 <= elevation <= 89; `level` is the
    height that is drawn at 0 (the reference's plane); a sample z stands h = (z - level) * exaggeration / pixel_size grid steps above it
    (the reference's zscale = 0.01 is a tenfold exaggeration).  pixel_size: the grid step in the units of z; None: taken from the
    Raster that is rendered."""
    azimuth: float = 202.5
    elevation: float = 60.0
    level: float = -1400.0
    exaggeration: float = 10.0
    pixel_size: float = None

    def __post_init__(self):
        for name in ("azimuth", "elevation", "level", "exaggeration"):
            value = getattr(self, name)
            if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value):
                raise ValueError(f"View.{name} must be a finite number, not {value!r}")
        if not 1.0 <= self.elevation <= 89.0:
            raise ValueError(f"View.elevation {self.elevation!r}: 1 .. 89 degrees")
        if not self.exaggeration > 0:
            raise ValueError(f"View.exaggeration {self.exaggeration!r} must be positive")
        if self.pixel_size is not None and not (np.isfinite(self.pixel_size) and self.pixel_size > 0):
            raise ValueError(f"View.pixel_size {self.pixel_size!r} must be positive")

    def zfac(self, pixel_size=None):
        size = self.pixel_size if self.pixel_size is not None else pixel_size
        if size is None:
            raise ValueError("View.pixel_size is required where the grid is not a Raster")
        return float(self.exaggeration) / float(size)

    def angles(self):
        """(sin A, cos A, sin E, cos E, tan E)"""
        sin_a, cos_a = sincos_degrees(self.azimuth)
        e = math.radians(float(self.elevation))
        return sin_a, cos_a, math.sin(e), math.cos(e), math.tan(e)


def perspective_frame(H, W, hmin, hmax, view, width=None, scale=None):
    """(Wo, Ho, sx0, sy0, step): the image that holds the scene.  The screen bounding box [xmin, xmax] x [ymin, ymax] of the eight
    corners (east 0 or W - 1, north 0 or -(H - 1), height min(0, hmin) or max(0, hmax); heights in grid steps) under `view`: screen x
    = -east cos A + north sin A, screen y = (-east sin A - north cos A) sin E + height cos E; an extent of 0 counts as 1.  width: Wo =
    width, step = (xmax - xmin) / width; scale (pixels per grid step): step = 1 / scale, Wo = ceil((xmax - xmin) / step).  Ho =
    ceil((ymax - ymin) / step), sx0 = xmin, sy0 = ymax.  Exactly one of width and scale is given."""
    if not isinstance(view, View):
        raise ValueError(f"perspective_frame: view must be a View, not {type(view).__name__}")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"perspective_frame: empty grid ({H} x {W})")
    if (width is None) == (scale is None):
        raise ValueError("perspective_frame: give width or scale, and not both")
    if not (np.isfinite(hmin) and np.isfinite(hmax) and hmin <= hmax):
        raise ValueError(f"perspective_frame: heights {hmin!r} .. {hmax!r}: finite and ascending")
    sin_a, cos_a, sin_e, cos_e, _ = view.angles()
    xs, ys = [], []
    for east in (0.0, float(W - 1)):
        for north in (0.0, -float(H - 1)):
            for height in (min(0.0, float(hmin)), max(0.0, float(hmax))):
                xs.append(-east * cos_a + north * sin_a)
                ys.append((-east * sin_a - north * cos_a) * sin_e + height * cos_e)
    xmin, ymax = min(xs), max(ys)
    span_x, span_y = max(xs) - xmin, ymax - min(ys)
    span_x, span_y = span_x if span_x > 0 else 1.0, span_y if span_y > 0 else 1.0
    if width is not None:
        if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 1:
            raise ValueError(f"perspective_frame: width {width!r}: a number of pixels, at least 1")
        Wo, step = int(width), span_x / int(width)
    else:
        if not (isinstance(scale, (int, float, np.integer, np.floating)) and np.isfinite(scale) and scale > 0):
            raise ValueError(f"perspective_frame: scale {scale!r}: pixels per grid step, positive")
        step = 1.0 / float(scale)
        Wo = max(1, int(math.ceil(span_x / step)))
    Ho = max(1, int(math.ceil(span_y / step)))
    if Wo * Ho >= 1 << 31:
        raise ValueError(f"perspective_frame: {Wo} x {Ho} pixels: Wo Ho must stay below 2^31")
    return Wo, Ho, xmin, ymax, step


def _rgba(who, name, colour):
    try:
        values = [int(v) for v in colour]
    except (TypeError, ValueError):
        values = []
    if len(values) != 4 or not all(0 <= v <= 255 for v in values):
        raise ValueError(f"{who}: {name} {colour!r}: four bytes r, g, b, a")
    return np.array(values, dtype=np.uint8)


def scene_arguments(who, H, W, drape_shape, drape_dtype, view, geometry, count, zmin, zmax, width, scale, facade, background):
    """The arguments the two entries share: (view values, Wo, Ho, facade bytes or None, background bytes)."""
    if not isinstance(view, View):
        raise ValueError(f"{who}: view must be a View, not {type(view).__name__}")
    drape_shape = tuple(int(s) for s in drape_shape)
    if np.dtype(drape_dtype) != np.uint8 or len(drape_shape) != 3 or drape_shape[:2] != (H, W) or drape_shape[2] not in (3, 4):
        raise ValueError(f"{who}: the drape must be uint8 ({H}, {W}, 3 | 4), registered at the nodes; got {np.dtype(drape_dtype).name} {drape_shape}")
    if H * W >= 1 << 31 or 2 * (H - 1) * (W - 1) >= 1 << 31:
        raise ValueError(f"{who}: {H} x {W}: H W and the triangles' ids 2 (H - 1) (W - 1) must stay below 2^31")
    pixel_size = None
    if geometry is not None:
        if abs(geometry.dx) != abs(geometry.dy):
            raise ValueError(f"{who}: nodes must be square; the geometry has dx = {geometry.dx!r}, dy = {geometry.dy!r}")
        pixel_size = abs(geometry.dx)
    zfac = view.zfac(pixel_size)
    sin_a, cos_a, sin_e, _, tan_e = view.angles()
    level = float(view.level)
    if count > 0 and H >= 2 and W >= 2:
        hmin, hmax = (float(zmin) - level) * zfac, (float(zmax) - level) * zfac
    else:
        hmin = hmax = 0.0
    Wo, Ho, sx0, sy0, step = perspective_frame(H, W, hmin, hmax, view, width=width, scale=scale)
    values = np.array([sin_a, cos_a, sin_e, tan_e, level, zfac, sx0, sy0, step], dtype=np.float64)
    return values, Wo, Ho, None if facade is None else _rgba(who, "facade", facade), _rgba(who, "background", background)


def grid_minmax(plane):
    """(count of finite samples, min, max) of a resident float32 plane (dbm_grid_minmax; NaN, NaN if the count is 0)."""
    H, W = plane_shape(plane)
    out = np.zeros(3, dtype=np.float64)
    plane.ctx.call("dbm_grid_minmax", devptr(plane), H, W, devptr(out))
    return int(out[0]), float(out[1]), float(out[2])


def perspective_image(grid, drape, view, width=1600, facade=None, background=(0, 0, 0, 0), return_hits=False, ctx=None, scale=None):
    """The perspective view of a plane on the GPU (dbm_grid_perspective; the rule: DESIGN.md 6o).  grid: a float32 DeviceArray (H, W) or
    (1, H, W), a Raster (its geometry gives the pixel size and must have square nodes), or a NumPy array that is uploaded.  drape: the
    uint8 image (H, W, 3 | 4) whose pixels sit at the nodes -- what `relief_image` returns for the plane -- resident or a NumPy array.
    view: a View.  width: the image's width in pixels (or scale: pixels per grid step, with width=None); its height follows from the
    scene (`perspective_frame`, with the plane's range from dbm_grid_minmax).  facade: None, or the r, g, b, a of the walls between
    `view.level` and the surface on the four outer edges.  background: the r, g, b, a of a pixel that sees nothing.
    Returns the resident uint8 DeviceArray (Ho, Wo, 4); with return_hits also the int32 DeviceArray (Ho, Wo) of the visible
    triangles' ids (2 (r (W - 1) + c) + t, a wall -2, none -1)."""
    from .tiling import Raster

    who = "perspective_image"
    geometry = None
    if isinstance(grid, Raster):
        geometry = grid.geometry
        grid = grid.device()
    if isinstance(grid, DeviceArray):
        if grid.dtype != np.float32:
            raise ValueError(f"{who}: grid holds {grid.dtype.name}: float32 planes are rendered")
        plane = grid
    else:
        host = np.asarray(grid, dtype=np.float32)
        plane = to_device(host.reshape(plane_shape(host)), ctx)
    H, W = plane_shape(plane)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: empty grid ({H} x {W})")
    if not isinstance(drape, DeviceArray):
        host = np.ascontiguousarray(drape)
        scene_arguments(who, H, W, host.shape, host.dtype, view, geometry, 0, 0.0, 0.0, width, scale, facade, background)   # refusals before the upload
        drape = DeviceArray(host.shape, plane.ctx, dtype=np.uint8).set(host)
    count, zmin, zmax = 0, 0.0, 0.0
    if isinstance(view, View) and H >= 2 and W >= 2:
        count, zmin, zmax = grid_minmax(plane)
    values, Wo, Ho, facade, background = scene_arguments(who, H, W, drape.shape, drape.dtype, view, geometry, count, zmin, zmax, width, scale, facade,
                                                background)
    out = DeviceArray((Ho, Wo, 4), plane.ctx, dtype=np.uint8)
    hits = DeviceArray((Ho, Wo), plane.ctx, dtype=np.int32) if return_hits else None
    plane.ctx.call("dbm_grid_perspective", devptr(plane), H, W, devptr(drape), drape.shape[2], devptr(values), Wo, Ho, devptr(facade),
                   devptr(background), devptr(out), devptr(hits))
    return (out.written(), hits.written()) if return_hits else out.written()


def perspective_image_host(grid, drape, view, width=1600, facade=None, background=(0, 0, 0, 0), return_hits=False, scale=None, geometry=None,
                           nthreads=None):
    """`perspective_image` on the host (dbm_grid_perspective_host: the kernel's own cell function under a plain traversal, on `nthreads`
    host threads): the float32 NumPy plane (H, W) and the uint8 NumPy drape (H, W, 3 | 4) -> the uint8 NumPy image (Ho, Wo, 4), with
    return_hits also the int32 ids.  geometry: a GridGeometry that gives the pixel size in place of `view.pixel_size`.  No GPU."""
    who = "perspective_image_host"
    z = np.ascontiguousarray(grid, dtype=np.float32)
    if z.ndim != 2 or z.size == 0:
        raise ValueError(f"{who}: grid must be (H, W) and not empty; got {z.shape}")
    if geometry is not None and not isinstance(geometry, GridGeometry):
        raise ValueError(f"{who}: geometry must be a GridGeometry, not {type(geometry).__name__}")
    drape = np.ascontiguousarray(drape)
    H, W = z.shape
    finite = z[np.isfinite(z)]
    count = int(finite.size) if H >= 2 and W >= 2 else 0
    zmin, zmax = (float(finite.min()), float(finite.max())) if count else (0.0, 0.0)
    values, Wo, Ho, facade, background = scene_arguments(who, H, W, drape.shape, drape.dtype, view, geometry, count, zmin, zmax, width, scale, facade,
                                                background)
    out = np.empty((Ho, Wo, 4), dtype=np.uint8)
    hits = np.empty((Ho, Wo), dtype=np.int32) if return_hits else None
    threads = int(nthreads) if nthreads else min(16, os.cpu_count() or 1)
    _lib.check(_lib.lib().dbm_grid_perspective_host(devptr(z), H, W, devptr(drape), drape.shape[2], devptr(values), Wo, Ho, devptr(facade),
                                                    devptr(background), devptr(out), devptr(hits), threads))
    return (out, hits) if return_hits else out


def plot_3d_view(grid, path, cpt, elev=60, azim=202.5, zmin=-1400, exaggeration=10, shading=None, width=1600, facade=(128, 128, 128, 255),
                 nodata=None, reduce=0, world_file=False, ctx=None, pixel_size=None):
    """The reference's `plot_3d_view` (deepbedmap.py:258-295) without GMT and without downloading the plane: `grid` -- a float32
    DeviceArray, a Raster (its nodata and geometry are used) or a NumPy array that is uploaded -- coloured by the ColorTable `cpt` (with
    `shading`, as `relief_image` does it), seen from azimuth `azim` and elevation `elev` above the level `zmin` with the vertical
    `exaggeration`, and written as the PNG `path`, `width` pixels wide, transparent where nothing is seen.  nodata and reduce: as in
    `render_dem` (the same code).  facade: the colour of the walls down to `zmin`, or None.  pixel_size: the grid step in the units of
    z where the grid is not a Raster.  world_file: a perspective view has no affine georeference; True is refused.  Returns the path."""
    from .relief import ColorTable, prepared_plane, relief_image, shading_parameters, write_png_resident

    who = "plot_3d_view"
    if not isinstance(cpt, ColorTable):
        raise ValueError(f"{who}: cpt must be a ColorTable (read_cpt, make_cpt, grey_cpt), not {type(cpt).__name__}")
    shading_parameters(shading)
    if world_file:
        raise ValueError(f"{who}: a perspective view has no world file (its pixels are not an affine map of the ground)")
    view = View(azimuth=azim, elevation=elev, level=zmin, exaggeration=exaggeration, pixel_size=pixel_size)
    plane, geometry = prepared_plane(who, grid, nodata, reduce, 4096, ctx)
    if geometry is not None and pixel_size is None:
        if abs(geometry.dx) != abs(geometry.dy):
            raise ValueError(f"{who}: nodes must be square; the geometry has dx = {geometry.dx!r}, dy = {geometry.dy!r}")
        view = dataclasses.replace(view, pixel_size=abs(geometry.dx))
    view.zfac()   # (refuses a missing pixel size before anything is launched)
    drape = relief_image(plane, cpt, shading=shading, channels=4)
    image = perspective_image(plane, drape, view, width=width, facade=facade)
    write_png_resident(path, image)
    return path
