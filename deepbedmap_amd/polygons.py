"""Selecting the training tiles inside the buffered grounding line on the GPU (reference data_prep.py:582-616, "Subset tiles to those
within grounding line": `gpd.read_file("misc/GroundingLine_Antarctica_v2.shp")` at :600, `.buffer(distance=10000)` at :602,
`gpd.sjoin(tile_gdf, op="within", gline)` at :606, `to_file("model/train/tiles_3031.geojson")` at :613, read back at :745-751).

The reference buffers the polygon with GEOS and tests window boxes against it; here every node of a raster is tested against the polygon
set's edges by dbm_grid_polygon_mask (include/dbm.h) -- this project's own, exactly defined selection, not a reproduction
of GEOS -- and a window is kept iff all its nodes are inside and hold data (`get_window_bounds` on the raster with NaN written outside).
The readers (ESRI shapefile, GeoJSON) and the tile-list files are host code without new dependencies.  No CPU fallback: without a GPU
every call that reaches the library raises DbmError; argument errors are raised before that.
"""
import ctypes as C
import json
import struct

import numpy as np

from . import _lib
from .resident import DeviceArray, GridGeometry, devptr, f64ptr
from .tiling import Raster, get_window_bounds

TILE = 16          # DBM_POLY_TILE: nodes along the side of a tile (one workgroup)
EDGE_CHUNK = 256   # DBM_POLY_CHUNK: edges staged into LDS at a time
TILES_CRS = "urn:ogc:def:crs:EPSG::3031"


class MaskArray(DeviceArray):
    """uint8 C-contiguous array of 0 / 1 resident in HBM."""

    def __init__(self, shape, ctx=None):
        super().__init__(shape, ctx, dtype=np.uint8)


class Polygons:
    """A polygon set as the pooled edges of all rings of all parts, holes included: `edges` (E, 4) float64 rows (xa, ya, xb, yb), every
    ring closed; `n_rings`; `bounds` (minx, miny, maxx, maxy) or None without edges.  Inside is the even-odd rule over all edges, so ring
    orientation does not matter and overlapping parts cancel."""

    def __init__(self, edges, n_rings):
        e = np.ascontiguousarray(edges, dtype=np.float64)
        if e.ndim != 2 or e.shape[1] != 4:
            raise ValueError(f"edges must be (E, 4) rows of (xa, ya, xb, yb); got shape {e.shape}")
        if not np.isfinite(e).all():
            raise ValueError("edges must be finite")
        if len(e) >= 2 ** 31:
            raise ValueError("a polygon set holds fewer than 2^31 edges")
        self.edges, self.n_rings = e, int(n_rings)
        self.bounds = None
        if len(e):
            xs, ys = e[:, [0, 2]], e[:, [1, 3]]
            self.bounds = (float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max()))
        self._dev = {}   # context -> device table

    @classmethod
    def from_rings(cls, rings):
        """`rings`: an iterable of (n, 2) vertex arrays.  An open ring is closed; a ring of fewer than 3 distinct points or with a
        non-finite value is refused."""
        out, n = [], 0
        for k, ring in enumerate(rings):
            p = np.asarray(ring, dtype=np.float64)
            if p.ndim != 2 or p.shape[1] < 2:
                raise ValueError(f"ring {k}: expected (n, 2) vertices, got shape {p.shape}")
            p = p[:, :2]
            if not np.isfinite(p).all():
                raise ValueError(f"ring {k} has a non-finite coordinate")
            if len(p) > 1 and np.array_equal(p[0], p[-1]):
                p = p[:-1]
            if len(np.unique(p, axis=0)) < 3:
                raise ValueError(f"ring {k} has fewer than 3 distinct points")
            out.append(np.concatenate([p, np.roll(p, -1, axis=0)], axis=1))
            n += 1
        return cls(np.concatenate(out) if out else np.zeros((0, 4)), n)

    @classmethod
    def box(cls, minx, miny, maxx, maxy):
        minx, miny, maxx, maxy = float(minx), float(miny), float(maxx), float(maxy)
        if not (minx < maxx and miny < maxy):
            raise ValueError("box: min must lie below max on both axes")
        return cls.from_rings([[(maxx, miny), (maxx, maxy), (minx, maxy), (minx, miny)]])

    def __len__(self):
        return len(self.edges)

    def device(self, ctx=None):
        """The edge table in HBM: one upload per context, reused across grids.  Returns the device pointer."""
        ctx = ctx or _lib.default_context()
        if ctx not in self._dev:
            self._dev[ctx] = ctx.malloc(max(self.edges.nbytes, 32))
            ctx.upload(self._dev[ctx], self.edges)
        return self._dev[ctx]

    def __del__(self):
        try:
            for ctx, ptr in self._dev.items():
                ctx.free(ptr)
            self._dev = {}
        except Exception:
            pass


# ---- readers ----
_SHP_POLYGONS = {5: "Polygon", 15: "PolygonZ", 25: "PolygonM"}
_SHP_NAMES = {0: "Null", 1: "Point", 3: "PolyLine", 5: "Polygon", 8: "MultiPoint", 11: "PointZ", 13: "PolyLineZ", 15: "PolygonZ",
              18: "MultiPointZ", 21: "PointM", 23: "PolyLineM", 25: "PolygonM", 28: "MultiPointM", 31: "MultiPatch"}


def _read_shp(buf, path):
    if len(buf) < 100:
        raise ValueError(f"{path}: {len(buf)} bytes are shorter than a shapefile header")
    code, = struct.unpack(">i", buf[:4])
    words, = struct.unpack(">i", buf[24:28])
    version, shape_type = struct.unpack("<ii", buf[28:36])
    if code != 9994 or version != 1000:
        raise ValueError(f"{path}: not an ESRI shapefile (file code {code}, version {version})")
    if 2 * words != len(buf):
        raise ValueError(f"{path}: the header promises {2 * words} bytes, the file has {len(buf)}")
    if shape_type not in _SHP_POLYGONS and shape_type != 0:
        raise ValueError(f"{path}: shape type {shape_type} ({_SHP_NAMES.get(shape_type, 'unknown')}) is not a polygon type")
    rings, at = [], 100
    while at < len(buf):
        if at + 8 > len(buf):
            raise ValueError(f"{path}: truncated record header at byte {at}")
        number, clen = struct.unpack(">ii", buf[at:at + 8])
        at += 8
        end = at + 2 * clen
        if clen < 2 or end > len(buf):
            raise ValueError(f"{path}: record {number} (content of {2 * clen} bytes at byte {at}) does not fit the file")
        rtype, = struct.unpack("<i", buf[at:at + 4])
        if rtype == 0:
            at = end
            continue
        if rtype not in _SHP_POLYGONS:
            raise ValueError(f"{path}: record {number} has shape type {rtype} ({_SHP_NAMES.get(rtype, 'unknown')}), not a polygon type")
        if 2 * clen < 44:
            raise ValueError(f"{path}: record {number} is shorter than a polygon header")
        nparts, npoints = struct.unpack("<ii", buf[at + 36:at + 44])
        need = 44 + 4 * nparts + 16 * npoints
        if nparts < 0 or npoints < 0 or need > 2 * clen:
            raise ValueError(f"{path}: record {number} declares {nparts} parts and {npoints} points, more than its {2 * clen} bytes hold")
        parts = np.frombuffer(buf, dtype="<i4", count=nparts, offset=at + 44).astype(np.int64)
        pts = np.frombuffer(buf, dtype="<f8", count=2 * npoints, offset=at + 44 + 4 * nparts).reshape(npoints, 2)
        bounds = np.append(parts, npoints)
        if nparts and (parts[0] != 0 or (np.diff(bounds) < 0).any()):
            raise ValueError(f"{path}: record {number} has part offsets that are not ascending from 0")
        for a, b in zip(bounds[:-1], bounds[1:]):
            rings.append(pts[a:b])
        at = end
    return rings


def _geojson_rings(obj, path, rings):
    kind = obj.get("type") if isinstance(obj, dict) else None
    if kind == "FeatureCollection":
        for f in obj.get("features", []):
            _geojson_rings(f, path, rings)
    elif kind == "Feature":
        if obj.get("geometry") is not None:
            _geojson_rings(obj["geometry"], path, rings)
    elif kind == "GeometryCollection":
        for g in obj.get("geometries", []):
            _geojson_rings(g, path, rings)
    elif kind == "Polygon":
        rings.extend(obj["coordinates"])
    elif kind == "MultiPolygon":
        for part in obj["coordinates"]:
            rings.extend(part)
    else:
        raise ValueError(f"{path}: GeoJSON type {kind!r} is not a Polygon, MultiPolygon or a collection of them")


def read_polygons(path):
    """The XY rings of an ESRI `.shp` (shape types 5, 15, 25: Polygon, PolygonZ, PolygonM; null shapes skipped; any other type raises
    ValueError naming it; header and record lengths validated) or of a GeoJSON file (Polygon, MultiPolygon, bare or inside Feature,
    FeatureCollection or GeometryCollection) as a Polygons -- what data_prep.py:600 reads with geopandas.  Host only."""
    path = str(path)
    with open(path, "rb") as f:
        buf = f.read()
    if path.lower().endswith(".shp"):
        return Polygons.from_rings(_read_shp(buf, path))
    rings = []
    _geojson_rings(json.loads(buf.decode("utf-8")), path, rings)
    return Polygons.from_rings(rings)


# ---- the mask ----
def _arguments(geometry, shape, polygons, buffer, workspace_limit):
    if not isinstance(geometry, GridGeometry):
        raise TypeError("geometry must be a GridGeometry")
    if not isinstance(polygons, Polygons):
        raise TypeError("polygons must be a Polygons")
    H, W = (int(v) for v in shape)
    if H < 1 or W < 1:
        raise ValueError(f"empty raster ({H} x {W})")
    if H * W >= 2 ** 31:
        raise ValueError("H W must stay below 2^31 nodes")
    buffer = float(buffer)
    if not np.isfinite(buffer):
        raise ValueError("buffer must be finite")
    if workspace_limit is None:
        workspace_limit = 0
    workspace_limit = int(workspace_limit)
    if workspace_limit < 0:
        raise ValueError("workspace_limit must not be negative")
    return H, W, buffer, workspace_limit


def _run(ctx, geometry, H, W, polygons, buffer, workspace_limit, mask, grid):
    """dbm_grid_polygon_mask into `mask` (a uint8 DeviceArray) or onto `grid` (a float32 one), the other None"""
    ctx.call("dbm_grid_polygon_mask", devptr(polygons.device(ctx)), len(polygons), H, W, f64ptr(geometry.as_array()), buffer, devptr(mask),
             devptr(grid), workspace_limit, _lib.DEVICE_PTRS)
    (grid if mask is None else mask).written()


def last_stats(ctx=None):
    """{"proximity_edges", "parity_edges", "tile_entries", "band_entries", "schedule" (0 unbinned, 1 binned, 2 no culling), "edges"} of the
    context's last polygon_mask / mask_outside call."""
    ctx = ctx or _lib.default_context()
    out = (C.c_int64 * 6)()
    ctx.call("dbm_grid_polygon_stats", out)
    return dict(zip(("proximity_edges", "parity_edges", "tile_entries", "band_entries", "schedule", "edges"), (int(v) for v in out)))


def polygon_mask(geometry, shape, polygons, buffer=0.0, download=True, workspace_limit=None, ctx=None):
    """The nodes of the (H, W) grid `geometry` inside `polygons` dilated (buffer >= 0) or eroded (buffer < 0) by |buffer| -- inside by
    the even-odd rule or within `buffer` of an edge; inside and farther than |buffer| from every edge.  Returns a NumPy
    bool (H, W), or with download=False a uint8 device array of 0 / 1.  workspace_limit: bytes the per-tile edge bins may take before
    every tile runs over the culled edge lists instead (None: the library's default); the result does not depend on it."""
    H, W, buffer, workspace_limit = _arguments(geometry, shape, polygons, buffer, workspace_limit)
    ctx = ctx or _lib.default_context()
    out = MaskArray((H, W), ctx)
    _run(ctx, geometry, H, W, polygons, buffer, workspace_limit, out, None)
    return out.get().astype(bool) if download else out


def mask_outside(raster, polygons, buffer=0.0, workspace_limit=None):
    """A new Raster with the same geometry and nodata: a device copy of `raster` with NaN written at the nodes outside the buffered
    polygon set, every other node's bits unchanged.  The argument is not modified."""
    if not isinstance(raster, Raster):
        raise TypeError("raster must be a Raster")
    H, W, buffer, workspace_limit = _arguments(raster.geometry, raster.shape, polygons, buffer, workspace_limit)
    src = raster.device()
    ctx = src.ctx
    out = DeviceArray((H, W), ctx)
    ctx.call("dbm_memcpy2d_d2d", devptr(out), 4 * W, devptr(src), 4 * W, 4 * W, H)
    _run(ctx, raster.geometry, H, W, polygons, buffer, workspace_limit, None, out)
    return Raster(out, raster.geometry, nodata=raster.nodata)


def select_tiles(raster, polygons, buffer=10000.0, height=36, width=36, step=3):
    """data_prep.py:577 + 600-606 for one grid: the bounding boxes (minx, miny, maxx, maxy) of every height x width window, moved by
    `step` pixels from the north-west corner, all of whose nodes hold data and lie inside `polygons` buffered by `buffer`:
    get_window_bounds(mask_outside(raster, polygons, buffer), height, width, step)."""
    return get_window_bounds(mask_outside(raster, polygons, buffer), height=height, width=width, step=step)


# ---- tile lists (data_prep.py:611-613 written, :745-751 read back) ----
def _num(v):
    return repr(float(v))


def tiles_to_geojson(path, tiles):
    """`tiles`: an ordered {grid_name: [(minx, miny, maxx, maxy), ...]}.  Writes the FeatureCollection geopandas' GeoJSON driver writes
    at data_prep.py:613: the EPSG:3031 crs member, one Feature per tile with a `grid_name` property, each ring in
    `shapely.geometry.box` order -- (maxx, miny), (maxx, maxy), (minx, maxy), (minx, miny), closed.  (The EPSG:4326 copy of :614-616
    needs an inverse projection and is not written.)  Returns the number of features."""
    lines = []
    for name, bounds in tiles.items():
        b = np.asarray(bounds, dtype=np.float64).reshape(-1, 4)
        if not np.isfinite(b).all():
            raise ValueError(f"tiles of {name!r} must be finite")
        for minx, miny, maxx, maxy in b:
            ring = [(maxx, miny), (maxx, maxy), (minx, maxy), (minx, miny), (maxx, miny)]
            coords = ", ".join(f"[ {_num(x)}, {_num(y)} ]" for x, y in ring)
            lines.append('{ "type": "Feature", "properties": { "grid_name": %s }, "geometry": { "type": "Polygon", "coordinates": [ [ %s ] ] } }'
                         % (json.dumps(str(name)), coords))
    head = '{\n"type": "FeatureCollection",\n"crs": { "type": "name", "properties": { "name": "%s" } },\n"features": [\n' % TILES_CRS
    with open(str(path), "w") as f:
        f.write(head + ",\n".join(lines) + "\n]\n}\n")
    return len(lines)


def read_tiles_geojson(path):
    """{grid_name: [(minx, miny, maxx, maxy), ...]} in file order (names in order of first appearance), the bounds from each ring's
    minimum and maximum: what data_prep.py:745-751 takes from `tiles_3031.geojson` (`geometry.bounds`, grouped by `grid_name`)."""
    with open(str(path)) as f:
        obj = json.load(f)
    if obj.get("type") != "FeatureCollection":
        raise ValueError(f"{path}: not a FeatureCollection")
    out = {}
    for k, feat in enumerate(obj.get("features", [])):
        geom = feat.get("geometry") or {}
        if geom.get("type") != "Polygon" or not geom.get("coordinates"):
            raise ValueError(f"{path}: feature {k} is not a Polygon")
        name = (feat.get("properties") or {}).get("grid_name")
        if name is None:
            raise ValueError(f"{path}: feature {k} has no grid_name property")
        ring = np.asarray(geom["coordinates"][0], dtype=np.float64)[:, :2]
        out.setdefault(str(name), []).append((float(ring[:, 0].min()), float(ring[:, 1].min()), float(ring[:, 0].max()), float(ring[:, 1].max())))
    return out
