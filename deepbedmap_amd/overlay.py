"""The maps' vector layers drawn where the image lies: lines, boxes and points (reference paper_figures.py:533-562, Figure 2: the
grounding line `fig.coast(shorelines="0.25p")` on the continent's DEM, the study regions and the 4028 training tiles as boxes
`fig.plot(style="r+s", pen="1p,orange2")`; paper_figures.py:1039-1045, Figure 5a: the transect's survey points
`fig.plot(style="c0.1c", color="orange")` on the Thwaites DEM).

The reference hands the layers to GMT.  Here `relief_image` leaves the picture in HBM, dbm_image_overlay (csrc/overlay.hip) paints one
layer after the other into it, and `write_png_resident` encodes it from there: nothing is downloaded, drawn on the host and uploaded
again.  A `Polygons` (the grounding line `read_polygons` read) and a `DevicePoints` (the survey `ascii_to_xyz` parsed) are painted from
the tables they already have in HBM.

The rule is this project's own and is stated in DESIGN.md 6p; GMT's pixels are NOT claimed.  `draw_layers_host` is its NumPy statement.
Filled polygons, dashed pens, symbols other than circles, text, axes, colour bars and legends stay out of scope.  No CPU fallback:
`draw_layers` and `render_map` raise DbmError without a GPU; `Layer`, `draw_layers_host` and every argument check need none.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .polygons import Polygons
from .resident import DeviceArray, DevicePoints, GridGeometry, devptr, f64ptr, points_table

TILE = 16          # DBM_OVERLAY_TILE: pixels along the side of a tile (one workgroup)
CHUNK = 256        # DBM_OVERLAY_CHUNK: primitives staged into LDS at a time
SEGMENTS, DISCS = 0, 1     # DBM_OVERLAY_SEGMENTS, DBM_OVERLAY_DISCS
SAMPLES = (1, 2, 4)
_KINDS = {"segments": SEGMENTS, "discs": DISCS}


def _colour(colour):
    try:
        c = tuple(colour)
    except TypeError:
        c = ()
    if len(c) == 3:
        c = c + (255,)
    if len(c) != 4 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in c):
        raise ValueError(f"colour {colour!r}: (r, g, b) or (r, g, b, a), integers in 0..255")
    return tuple(int(v) for v in c)


def _size(size, what):
    try:
        size = float(size)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {size!r} is not a number of pixels") from None
    if not np.isfinite(size) or size < 0:
        raise ValueError(f"{what} {size!r}: a number of pixels, finite and not negative")
    return size


def _host_table(table, kind, what):
    """float64 C-contiguous (n, 4) segments or (n, 2 | 3) points, every coordinate finite (a z column is not looked at)."""
    t = np.ascontiguousarray(table, dtype=np.float64)
    if kind == "segments":
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError(f"{what}: segments must be (n, 4) rows of (xa, ya, xb, yb); got shape {t.shape}")
        used = t
    else:
        if t.ndim != 2 or t.shape[1] not in (2, 3):
            raise ValueError(f"{what}: points must be (n, 2) x, y or (n, 3) x, y, z (a row stride of 2 or 3 doubles); got shape {t.shape}")
        used = t[:, :2]
    if len(t) >= 2 ** 31:
        raise ValueError(f"{what}: a layer holds fewer than 2^31 primitives")
    if not np.isfinite(used).all():
        raise ValueError(f"{what}: primitive {int(np.flatnonzero(~np.isfinite(used).all(axis=1))[0])} has a non-finite coordinate")
    return t


@dataclasses.dataclass(frozen=True, eq=False)
class Layer:
    """Primitives of one kind, one size in pixels and one colour.  kind: "segments" -- `primitives` is a float64 (n, 4) array of rows
    (xa, ya, xb, yb) in map coordinates or a `Polygons` (its pooled edges), drawn with a pen of `size` pixels, a segment of length
    zero as a dot -- or "discs" -- a float64 (n, 2 | 3) array of rows (x, y[, z]) or a `DevicePoints`, drawn as discs of diameter `size`
    pixels.  colour: (r, g, b, a) in 0..255.  resident: the primitives are a table in HBM (a Polygons, a DevicePoints) and are painted
    from there.  Made by `Layer.lines`, `Layer.boxes` and `Layer.points`; the constructor checks the same things."""
    kind: str
    primitives: object
    size: float
    colour: tuple
    resident: bool = False

    def __post_init__(self):
        if self.kind not in _KINDS:
            raise ValueError(f"Layer: kind {self.kind!r}: \"segments\" or \"discs\"")
        what = "Layer.lines" if self.kind == "segments" else "Layer.points"
        prims, resident = self.primitives, False
        if isinstance(prims, Polygons):
            if self.kind != "segments":
                raise ValueError("Layer: a Polygons is drawn as segments")
            resident = True
        elif isinstance(prims, DevicePoints):
            if self.kind != "discs":
                raise ValueError("Layer: a DevicePoints is drawn as discs")
            if prims.ncol not in (2, 3):
                raise ValueError(f"{what}: a row stride of {prims.ncol} doubles: 2 or 3")
            resident = True
        else:
            if self.kind == "discs":
                prims = points_table(prims, ncols=lambda c: True, what=what)
            prims = _host_table(prims, self.kind, what)
            prims.setflags(write=False)
        object.__setattr__(self, "primitives", prims)
        object.__setattr__(self, "resident", resident)
        object.__setattr__(self, "size", _size(self.size, "width" if self.kind == "segments" else "diameter"))
        object.__setattr__(self, "colour", _colour(self.colour))

    def __len__(self):
        return len(self.primitives)

    @classmethod
    def lines(cls, segments, width, colour):
        """Segments (n, 4) of rows (xa, ya, xb, yb), or a `Polygons` -- every edge of every ring, from its table in HBM -- drawn with
        a pen of `width` pixels (GMT's `pen`; `fig.coast(shorelines=...)` for the grounding line)."""
        return cls("segments", segments, width, colour)

    @classmethod
    def boxes(cls, bounds, width, colour):
        """GMT's `style="r+s"`: every row (minx, miny, maxx, maxy) of `bounds` (n, 4) -- or of the lists of a {grid_name: bounds}
        dict, as `read_tiles_geojson` returns it, in its order -- as four segments, in this order: south (minx, miny)-(maxx, miny),
        east (maxx, miny)-(maxx, maxy), north (maxx, maxy)-(minx, maxy), west (minx, maxy)-(minx, miny)."""
        if isinstance(bounds, dict):
            bounds = [b for rows in bounds.values() for b in rows]
        b = np.asarray(bounds, dtype=np.float64)
        if b.size == 0:
            b = b.reshape(0, 4)
        if b.ndim != 2 or b.shape[1] != 4:
            raise ValueError(f"Layer.boxes: bounds must be (n, 4) rows of (minx, miny, maxx, maxy); got shape {b.shape}")
        minx, miny, maxx, maxy = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        sides = np.stack([np.stack([minx, miny, maxx, miny], axis=1), np.stack([maxx, miny, maxx, maxy], axis=1),
                          np.stack([maxx, maxy, minx, maxy], axis=1), np.stack([minx, maxy, minx, miny], axis=1)], axis=1)
        return cls("segments", sides.reshape(-1, 4), width, colour)

    @classmethod
    def points(cls, points, diameter, colour):
        """Points -- an (n, 2 | 3) array of rows (x, y[, z]), a DataFrame with columns x, y[, z], or a `DevicePoints`, from its table in
        HBM -- drawn as discs of `diameter` pixels (GMT's `style="c..."`)."""
        return cls("discs", points, diameter, colour)


def _geom4(geometry):
    if isinstance(geometry, GridGeometry):
        return np.array([geometry.x0, geometry.y0, geometry.dx, geometry.dy], dtype=np.float64)
    try:
        g = np.array([float(v) for v in tuple(geometry)[:4]], dtype=np.float64)
    except (TypeError, ValueError):
        g = np.zeros(0)
    if g.size != 4 or not np.isfinite(g).all() or g[2] == 0 or g[3] == 0:
        raise ValueError(f"geometry {geometry!r}: a GridGeometry or (x0, y0, dx, dy), finite, dx and dy non-zero")
    return g


def _arguments(who, shape, dtype, layers, samples):
    shape = tuple(int(s) for s in shape)
    if np.dtype(dtype) != np.uint8:
        raise ValueError(f"{who}: image holds {np.dtype(dtype).name}: uint8 images are drawn on")
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: image must be (H, W, channels) and not empty; got {shape}")
    if shape[2] not in (3, 4):
        raise ValueError(f"{who}: channels {shape[2]}: 3 (RGB) or 4 (RGBA)")
    if shape[0] * shape[1] >= 1 << 31:
        raise ValueError(f"{who}: H W must stay below 2^31 pixels")
    if isinstance(samples, bool) or samples not in SAMPLES:
        raise ValueError(f"{who}: samples {samples!r}: 1, 2 or 4 sub-samples along a pixel's side")
    layers = list(layers)
    for k, layer in enumerate(layers):
        if not isinstance(layer, Layer):
            raise ValueError(f"{who}: layers[{k}] must be a Layer (Layer.lines, Layer.boxes, Layer.points), not {type(layer).__name__}")
    return shape, layers, int(samples)


# ---- the rule on the host ----
def _host_primitives(layer):
    """The layer's table on the host: (n, 4) for segments, (n, 2) for discs, float64."""
    prims = layer.primitives
    if isinstance(prims, Polygons):
        return prims.edges
    if isinstance(prims, DevicePoints):
        prims = prims.ctx.download(prims.ptr, np.float64, (prims.n, prims.ncol))
        if not np.isfinite(prims[:, :2]).all():
            raise ValueError("draw_layers_host: a resident point has a non-finite coordinate")
    return prims if layer.kind == "segments" else prims[:, :2]


def _coverage_host(H, W, g, kind, table, size, S):
    """m (H, W): the number of covered sub-samples of every pixel.  Primitive by primitive, each on the window of pixels its box --
    grown by the radius and, generously, by more than the margin of DESIGN.md 6p -- can reach."""
    x0, y0, dx, dy = (np.float64(v) for v in g)
    offsets = (np.arange(S, dtype=np.float64) + 0.5) / S - 0.5
    h = np.float64(size) / 2
    h2 = h * h
    cover = np.zeros((H, S, W, S), dtype=bool)    # [r, i, c, j]
    with np.errstate(all="ignore"):
        t = np.asarray(table, dtype=np.float64)
        ua, va = (t[:, 0] - x0) / dx, (t[:, 1] - y0) / dy
        ub, vb = ((t[:, 2] - x0) / dx, (t[:, 3] - y0) / dy) if kind == "segments" else (ua, va)
        for k in range(len(t)):
            au, av, bu, bv = ua[k], va[k], ub[k], vb[k]
            if not (np.isfinite(au) and np.isfinite(av) and np.isfinite(bu) and np.isfinite(bv)):
                continue    # overflowed pixel coordinates: every d2 is inf or NaN
            reach = h + 2.0 + max(abs(au), abs(av), abs(bu), abs(bv), W, H, h) * 2.0 ** -29
            lo_c, hi_c, lo_r, hi_r = min(au, bu) - reach, max(au, bu) + reach, min(av, bv) - reach, max(av, bv) + reach
            if hi_c < 0 or lo_c > W - 1 or hi_r < 0 or lo_r > H - 1:
                continue
            c0, c1 = int(max(0.0, np.floor(lo_c))), int(min(W - 1.0, np.ceil(hi_c)))
            r0, r1 = int(max(0.0, np.floor(lo_r))), int(min(H - 1.0, np.ceil(hi_r)))
            su = np.arange(c0, c1 + 1, dtype=np.float64)[:, None] + offsets[None, :]
            sv = np.arange(r0, r1 + 1, dtype=np.float64)[:, None] + offsets[None, :]
            px, py = (su - au)[None, None, :, :], (sv - av)[:, :, None, None]
            if kind == "segments":
                ex, ey = bu - au, bv - av
                L = ex * ex + ey * ey
                if L > 0:
                    tt = (px * ex + py * ey) / L
                    tt = np.where(tt < 0.0, 0.0, np.where(tt > 1.0, 1.0, tt))
                else:
                    tt = np.float64(0.0)
                qx, qy = px - tt * ex, py - tt * ey
            else:
                qx, qy = px, py
            d2 = qx * qx + qy * qy
            cover[r0:r1 + 1, :, c0:c1 + 1, :] |= d2 <= h2
    return cover.sum(axis=(1, 3), dtype=np.int64)


def _blend_host(image, m, rgba, S):
    D = S * S * 255
    w = (m * rgba[3])[..., None]
    src = np.array(list(rgba[:3]) + [255], dtype=np.int64)[:image.shape[2]]
    out = (w * src + (D - w) * image.astype(np.int64) + D // 2) // D
    return np.where((m > 0)[..., None], out, image).astype(np.uint8)


def draw_layers_host(image, geometry, layers, samples=4):
    """The NumPy statement of DESIGN.md 6p, without a GPU: a copy of the uint8 (H, W, 3 | 4) `image` with `layers` painted in list
    order.  geometry: the GridGeometry of the pixel centres, or (x0, y0, dx, dy)."""
    who = "draw_layers_host"
    if not isinstance(image, np.ndarray):
        raise ValueError(f"{who}: image must be a uint8 NumPy array, not {type(image).__name__} (a DeviceArray is drawn on by draw_layers)")
    (H, W, _), layers, S = _arguments(who, image.shape, image.dtype, layers, samples)
    g = _geom4(geometry)
    out = np.array(image, dtype=np.uint8, copy=True)
    for layer in layers:
        m = _coverage_host(H, W, g, layer.kind, _host_primitives(layer), layer.size, S)
        out = _blend_host(out, m, layer.colour, S)
    return out


# ---- the rule on the device ----
def last_stats(ctx=None):
    """{"kept", "entries", "schedule" (0 unbinned, 1 binned), "primitives"} of the context's last layer: the primitives the cull kept,
    the entries of the tile bins, which schedule painted, and how many primitives the layer held."""
    ctx = ctx or _lib.default_context()
    out = (C.c_int64 * 4)()
    ctx.call("dbm_image_overlay_stats", out)
    return dict(zip(("kept", "entries", "schedule", "primitives"), (int(v) for v in out)))


def draw_layers(image, geometry, layers, samples=4, workspace_limit=None, ctx=None):
    """Paints `layers` in list order into the resident uint8 DeviceArray `image` (H, W, 3 | 4), in place, and returns it
    (dbm_image_overlay, one call per layer; the rule: DESIGN.md 6p, `draw_layers_host` is its NumPy statement).  geometry: the
    GridGeometry of the pixel centres -- what `render_dem` returns, `reduced_geometry` for a level of the pyramid -- or (x0, y0, dx,
    dy).  samples: sub-samples along a pixel's side, 1, 2 or 4.  workspace_limit: bytes the per-tile bins of a layer may take before
    every tile runs over the whole culled list instead (None: the library's default); the bytes do not depend on it.
    Every argument and every host table is checked before the first layer is painted.  A resident table's coordinates are checked by
    its own layer's cull pass: a non-finite one raises DbmError before that layer writes a byte, the layers before it stay painted."""
    who = "draw_layers"
    if not isinstance(image, DeviceArray):
        raise ValueError(f"{who}: image must be a uint8 DeviceArray, not {type(image).__name__} (a NumPy array is drawn on by draw_layers_host)")
    (H, W, channels), layers, S = _arguments(who, image.shape, image.dtype, layers, samples)
    g = _geom4(geometry)
    if workspace_limit is None:
        workspace_limit = 0
    workspace_limit = int(workspace_limit)
    if workspace_limit < 0:
        raise ValueError(f"{who}: workspace_limit must not be negative")
    if ctx is not None and ctx is not image.ctx:
        raise ValueError(f"{who}: the image lives in another context")
    ctx = image.ctx
    for layer in layers:
        if isinstance(layer.primitives, DevicePoints) and layer.primitives.ctx is not ctx:
            raise ValueError(f"{who}: a layer's DevicePoints live in another context than the image")
    for layer in layers:
        prims = layer.primitives
        if isinstance(prims, Polygons):
            table, n, stride, flags = devptr(prims.device(ctx)), len(prims), 4, _lib.DEVICE_PTRS
        elif isinstance(prims, DevicePoints):
            table, n, stride, flags = devptr(prims), prims.n, prims.ncol, _lib.DEVICE_PTRS
        else:
            table, n, stride, flags = devptr(prims), prims.shape[0], prims.shape[1], 0
        ctx.call("dbm_image_overlay", devptr(image), H, W, channels, f64ptr(g), table, n, _KINDS[layer.kind], stride, layer.size,
                 bytes(layer.colour), S, workspace_limit, flags)
        image.written()
    return image


# ---- the product ----
def render_map(grid, path, cpt, layers, shading=None, reduce=0, max_size=4096, nodata=None, samples=4, filter=1, world_file=True,
               ctx=None, aspect=1.0, channels=4, band_rows=None, workspace_limit=None):
    """`render_dem` with the maps' vector layers (paper_figures.py:521-562, :1039-1045): the Raster `grid` coloured by `cpt` (with
    `shading`), `layers` painted over it in list order with the geometry of the rendered level, and the picture written as the PNG
    `path` -- `prepared_plane`, `relief_image`, `draw_layers`, `write_png_resident`; the image never leaves HBM uncompressed.
    The layers are in map coordinates, so the grid must carry a geometry: anything but a Raster raises ValueError.  nodata, reduce,
    max_size, filter, aspect, channels, band_rows: as in `render_dem`; samples, workspace_limit: as in `draw_layers`.
    world_file: the .pgw of the rendered level is written next to the file.  Returns (path, the GridGeometry of the image)."""
    from .relief import ColorTable, prepared_plane, relief_image, shading_parameters, write_png_resident
    from .tiling import Raster

    who = "render_map"
    if not isinstance(grid, Raster):
        raise ValueError(f"{who}: layers are in map coordinates: grid must be a Raster with its geometry, not {type(grid).__name__}")
    if not isinstance(cpt, ColorTable):
        raise ValueError(f"{who}: cpt must be a ColorTable (read_cpt, make_cpt, grey_cpt), not {type(cpt).__name__}")
    if not np.isfinite(float(aspect)):
        raise ValueError(f"{who}: aspect {aspect!r} must be finite")
    shading_parameters(shading)
    _, layers, samples = _arguments(who, (1, 1, channels), np.uint8, layers, samples)
    plane, geometry = prepared_plane(who, grid, nodata, reduce, max_size, ctx)
    image = relief_image(plane, cpt, shading=shading, aspect=aspect, channels=channels)
    draw_layers(image, geometry, layers, samples=samples, workspace_limit=workspace_limit)
    write_png_resident(path, image, filter=filter, band_rows=band_rows, world_file=geometry if world_file else None)
    return path, geometry
