"""CPU checks of the buffered-polygon tile selection (deepbedmap_amd/polygons.py, dbm_grid_polygon_mask; reference
data_prep.py:582-616): the NumPy restatement of the definition (tests/polygon_restatement.py) against matplotlib's point-in-polygon test
and against closed forms, the shapefile / GeoJSON readers, the tile-list files, and the boundary behaviour without a GPU."""
import json
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import polygon_restatement as pr  # noqa: E402

GEOM = (-1_600_000.0, -200_000.0, 250.0, -250.0)   # north-west node, 250 m pixels, north-up
SHAPE = (33, 47)


def star(seed, geom=GEOM, shape=SHAPE):
    """A seeded star polygon of 3-39 vertices around a point of the grid.  Odd seeds round the vertices to nodes and half-nodes, even
    seeds to centimetres."""
    r = np.random.default_rng(seed)
    x0, y0, dx, dy = geom
    H, W = shape
    n = int(r.integers(3, 40))
    cx, cy = x0 + r.uniform(0.2, 0.8) * (W - 1) * dx, y0 + r.uniform(0.2, 0.8) * (H - 1) * dy
    ang = np.sort(r.uniform(0, 2 * np.pi, n))
    rad = r.uniform(0.1, 0.6, n) * min(H, W) * abs(dx)
    p = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)
    if seed % 2:
        p[:, 0] = x0 + np.round((p[:, 0] - x0) / (dx / 2)) * (dx / 2)
        p[:, 1] = y0 + np.round((p[:, 1] - y0) / (dy / 2)) * (dy / 2)
    else:
        p = np.round(p, 2)
    return p


def boundary_distance(geom, shape, edges):
    """Distance of every node to the nearest edge (float64, the restatement's own operation order)."""
    xs, ys = pr.node_axes(geom, shape)
    e = np.asarray(edges)
    xa, ya, xb, yb = (e[:, k][None, None, :] for k in range(4))
    ex, ey = xb - xa, yb - ya
    L = ex * ex + ey * ey
    px, py = xs[None, :, None] - xa, ys[:, None, None] - ya
    with np.errstate(all="ignore"):
        t = np.clip(np.where(L > 0, (px * ex + py * ey) / np.where(L > 0, L, 1.0), 0.0), 0.0, 1.0)
    return np.sqrt(((px - t * ex) ** 2 + (py - t * ey) ** 2).min(axis=2))


def test_restatement_against_matplotlib_on_200_star_polygons():
    from matplotlib.path import Path

    xs, ys = pr.node_axes(GEOM, SHAPE)
    nodes = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    excluded = disagreements = total = 0
    for seed in range(200):
        p = star(seed)
        ring = pr.ring_edges([p])
        got, _ = pr.inside_near(GEOM, SHAPE, ring, 0.0)
        want = Path(np.concatenate([p, p[:1]]), closed=True).contains_points(nodes).reshape(SHAPE)
        clear = boundary_distance(GEOM, SHAPE, ring) > 1e-6
        excluded += int((~clear).sum())
        disagreements += int((got != want)[clear].sum())
        total += got.size
    print("nodes", total, "excluded", excluded, "disagreements", disagreements)
    assert total == 200 * SHAPE[0] * SHAPE[1]
    assert excluded <= 0.01 * total, (excluded, total)
    assert disagreements == 0


def test_dilation_and_erosion_of_a_rectangle_against_closed_forms():
    geom, shape = (-1_600_000.0, -200_000.0, 250.0, -250.0), (90, 110)
    xs, ys = pr.node_axes(geom, shape)
    x0, x1, y0, y1 = xs[30], xs[80], ys[65], ys[20]   # (on nodes: minx, maxx, miny, maxy)
    edges = pr.ring_edges([[(x1, y0), (x1, y1), (x0, y1), (x0, y0)]])
    X, Y = np.meshgrid(xs, ys)
    b = 7.3 * 250.0
    gx = np.maximum(np.maximum(x0 - X, X - x1), 0.0)
    gy = np.maximum(np.maximum(y0 - Y, Y - y1), 0.0)
    want = gx * gx + gy * gy <= b * b
    got = pr.mask(geom, shape, edges, b)
    assert want.any() and not want.all()
    assert np.array_equal(got, want), int((got != want).sum())
    # the erosion: strictly inside the rectangle shrunk by the buffer (a node AT distance |buffer| from an edge is near, hence out)
    shrunk = (X > x0 + b) & (X < x1 - b) & (Y > y0 + b) & (Y < y1 - b)
    got = pr.mask(geom, shape, edges, -b)
    assert shrunk.any()
    assert np.array_equal(got, shrunk), int((got != shrunk).sum())
    # buffer 0 and -0.0: between the open and the closed rectangle.  (A node ON an edge has t = (px ex) / (ex ex) rounded, so its d2 may
    # come out a few ulps above 0: at buffer 0 a boundary node is in only where the parity rule or an exact d2 says so.)
    zero = pr.mask(geom, shape, edges, 0.0)
    closed = (X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1)
    interior = (X > x0) & (X < x1) & (Y > y0) & (Y < y1)
    assert not (zero & ~closed).any() and not (interior & ~zero).any()
    assert np.array_equal(pr.mask(geom, shape, edges, -0.0), zero)
    # no edges: nothing
    assert not pr.mask(geom, shape, np.zeros((0, 4)), 1e9).any()


# ---- readers ----
def _shp_polygon(parts, shape_type=5):
    pts = np.concatenate(parts)
    starts = np.cumsum([0] + [len(p) for p in parts[:-1]])
    body = struct.pack("<i4d2i", shape_type, pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max(), len(parts), len(pts))
    body += struct.pack(f"<{len(parts)}i", *starts) + pts.astype("<f8").tobytes()
    if shape_type == 15:     # Z range + Z array, M range + M array
        body += struct.pack("<2d", 0.0, 1.0) + np.linspace(0, 1, len(pts)).astype("<f8").tobytes()
        body += struct.pack("<2d", 0.0, 0.0) + np.zeros(len(pts), "<f8").tobytes()
    if shape_type == 25:
        body += struct.pack("<2d", 0.0, 0.0) + np.zeros(len(pts), "<f8").tobytes()
    return body


def _shp_file(records, shape_type=5):
    out = b""
    for k, body in enumerate(records):
        assert len(body) % 2 == 0
        out += struct.pack(">2i", k + 1, len(body) // 2) + body
    header = struct.pack(">7i", 9994, 0, 0, 0, 0, 0, (100 + len(out)) // 2) + struct.pack("<2i", 1000, shape_type) + struct.pack("<8d", *([0.0] * 8))
    assert len(header) == 100
    return header + out


def _closed(p):
    p = np.asarray(p, dtype=np.float64)
    return np.concatenate([p, p[:1]])


OUTER = [(0.0, 0.0), (0.0, 10.0), (10.0, 10.0), (10.0, 0.0)]
HOLE = [(4.0, 4.0), (6.0, 4.0), (6.0, 6.0), (4.0, 6.0)]
PART_A = [(20.0, 0.0), (20.0, 5.0), (25.0, 5.0)]
PART_B = [(30.0, 0.0), (30.0, 5.0), (35.0, 5.0), (35.0, 0.0)]


def test_read_polygons_shapefile(tmp_path):
    import deepbedmap_amd as dbm

    path = tmp_path / "gl.shp"
    records = [_shp_polygon([_closed(OUTER), _closed(HOLE)]), struct.pack("<i", 0), _shp_polygon([_closed(PART_A), _closed(PART_B)]),
               _shp_polygon([_closed(PART_B)], 15)]
    path.write_bytes(_shp_file(records))
    p = dbm.read_polygons(path)
    assert p.n_rings == 5 and p.edges.shape == (4 + 4 + 3 + 4 + 4, 4) and p.edges.dtype == np.float64
    assert p.bounds == (0.0, 0.0, 35.0, 10.0)
    want = pr.ring_edges([OUTER, HOLE, PART_A, PART_B, PART_B])
    assert np.array_equal(p.edges, want)
    # every ring is closed: each vertex starts one edge and ends one
    assert sorted(map(tuple, p.edges[:, :2])) == sorted(map(tuple, p.edges[:, 2:]))
    # PolygonM
    (tmp_path / "m.shp").write_bytes(_shp_file([_shp_polygon([_closed(OUTER)], 25)], 25))
    assert len(dbm.read_polygons(tmp_path / "m.shp")) == 4
    # a polyline record is refused by name
    (tmp_path / "line.shp").write_bytes(_shp_file([_shp_polygon([_closed(OUTER)], 3)], 3))
    with pytest.raises(ValueError, match="PolyLine"):
        dbm.read_polygons(tmp_path / "line.shp")
    (tmp_path / "mixed.shp").write_bytes(_shp_file([_shp_polygon([_closed(OUTER)]), _shp_polygon([_closed(OUTER)], 3)]))
    with pytest.raises(ValueError, match="record 2.*PolyLine"):
        dbm.read_polygons(tmp_path / "mixed.shp")
    # truncated: the header's length, a record's length, a record's point count
    whole = _shp_file(records)
    (tmp_path / "cut.shp").write_bytes(whole[:-24])
    with pytest.raises(ValueError, match="header promises"):
        dbm.read_polygons(tmp_path / "cut.shp")
    cut = bytearray(whole[:-24])
    cut[24:28] = struct.pack(">i", len(cut) // 2)
    (tmp_path / "cut2.shp").write_bytes(bytes(cut))
    with pytest.raises(ValueError, match="does not fit"):
        dbm.read_polygons(tmp_path / "cut2.shp")
    lying = bytearray(whole)
    lying[100 + 8 + 40:100 + 8 + 44] = struct.pack("<i", 10_000)
    (tmp_path / "lying.shp").write_bytes(bytes(lying))
    with pytest.raises(ValueError, match="more than its"):
        dbm.read_polygons(tmp_path / "lying.shp")
    (tmp_path / "short.shp").write_bytes(whole[:60])
    with pytest.raises(ValueError, match="shorter than a shapefile header"):
        dbm.read_polygons(tmp_path / "short.shp")
    (tmp_path / "other.shp").write_bytes(b"\0" * 200)
    with pytest.raises(ValueError, match="not an ESRI shapefile"):
        dbm.read_polygons(tmp_path / "other.shp")


def test_read_polygons_geojson_in_every_nesting(tmp_path):
    import deepbedmap_amd as dbm

    poly = {"type": "Polygon", "coordinates": [_closed(OUTER).tolist(), _closed(HOLE).tolist()]}
    multi = {"type": "MultiPolygon", "coordinates": [[_closed(PART_A).tolist()], [_closed(PART_B).tolist()]]}
    feature = {"type": "Feature", "properties": {}, "geometry": poly}
    cases = {
        "polygon": (poly, [OUTER, HOLE]),
        "multi": (multi, [PART_A, PART_B]),
        "feature": (feature, [OUTER, HOLE]),
        "collection": ({"type": "FeatureCollection", "features": [feature, {"type": "Feature", "properties": {}, "geometry": multi},
                                                                  {"type": "Feature", "properties": {}, "geometry": None}]},
                       [OUTER, HOLE, PART_A, PART_B]),
        "geometries": ({"type": "GeometryCollection", "geometries": [multi, poly]}, [PART_A, PART_B, OUTER, HOLE]),
    }
    for name, (obj, rings) in cases.items():
        path = tmp_path / f"{name}.geojson"
        path.write_text(json.dumps(obj))
        p = dbm.read_polygons(path)
        assert p.n_rings == len(rings), name
        assert np.array_equal(p.edges, pr.ring_edges(rings)), name
    (tmp_path / "line.geojson").write_text(json.dumps({"type": "LineString", "coordinates": OUTER}))
    with pytest.raises(ValueError, match="LineString"):
        dbm.read_polygons(tmp_path / "line.geojson")


def test_from_rings_and_box():
    import deepbedmap_amd as dbm

    open_ring = dbm.Polygons.from_rings([OUTER])
    closed_ring = dbm.Polygons.from_rings([_closed(OUTER)])
    assert np.array_equal(open_ring.edges, closed_ring.edges) and len(open_ring) == 4
    assert np.array_equal(open_ring.edges[-1], [10.0, 0.0, 0.0, 0.0])     # the closing edge
    for bad, match in (([[(0, 0), (1, 1)]], "fewer than 3"), ([[(0, 0), (1, 1), (0, 0), (1, 1)]], "fewer than 3"),
                       ([[(0, 0), (1, 1), (0, 0)]], "fewer than 3"), ([[(0, 0), (1, np.nan), (2, 0)]], "non-finite"),
                       ([[(0, 0), (np.inf, 1), (2, 0)]], "non-finite"), ([[0.0, 1.0, 2.0]], "vertices")):
        with pytest.raises(ValueError, match=match):
            dbm.Polygons.from_rings(bad)
    empty = dbm.Polygons.from_rings([])
    assert len(empty) == 0 and empty.bounds is None and empty.n_rings == 0
    b = dbm.Polygons.box(1, 2, 3, 5)
    assert b.bounds == (1.0, 2.0, 3.0, 5.0) and b.n_rings == 1
    assert np.array_equal(b.edges[:, :2], [(3, 2), (3, 5), (1, 5), (1, 2)])   # shapely.geometry.box order
    with pytest.raises(ValueError):
        dbm.Polygons.box(1, 2, 1, 5)


# ---- tile lists ----
def test_tile_list_round_trip(tmp_path):
    import deepbedmap_amd as dbm

    tiles = {"b.nc": [(0.0, -9000.0, 9000.0, 0.0), (750.0, -9000.0, 9750.0, 0.0)], "a.nc": [(-1.5e6, 2.25, -1.4e6, 100000.125)]}
    path = tmp_path / "tiles.geojson"
    assert dbm.tiles_to_geojson(path, tiles) == 3
    back = dbm.read_tiles_geojson(path)
    assert list(back) == ["b.nc", "a.nc"] and back == {k: [tuple(b) for b in v] for k, v in tiles.items()}
    obj = json.loads(path.read_text())
    assert obj["crs"] == {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3031"}}
    assert [f["properties"]["grid_name"] for f in obj["features"]] == ["b.nc", "b.nc", "a.nc"]
    minx, miny, maxx, maxy = tiles["b.nc"][1]
    assert obj["features"][1]["geometry"]["coordinates"] == [[[maxx, miny], [maxx, maxy], [minx, maxy], [minx, miny], [maxx, miny]]]


def test_tile_list_of_the_reference(tmp_path):
    """tests/golden/tiles_3031_head.geojson: the header and the first 40 features of the file the reference wrote at data_prep.py:613."""
    import deepbedmap_amd as dbm

    golden = os.path.join(HERE, "golden", "tiles_3031_head.geojson")
    tiles = dbm.read_tiles_geojson(golden)
    assert list(tiles) == ["2010tr.nc"] and len(tiles["2010tr.nc"]) == 40
    b = np.asarray(tiles["2010tr.nc"])
    assert np.all(b[:, 2] - b[:, 0] == 9000.0) and np.all(b[:, 3] - b[:, 1] == 9000.0)   # 36 pixels of 250 m
    assert tiles["2010tr.nc"][0] == (-1587750.0, -145500.0, -1578750.0, -136500.0)
    out = tmp_path / "again.geojson"
    dbm.tiles_to_geojson(out, tiles)
    theirs, ours = json.load(open(golden)), json.load(open(out))
    assert ours["crs"] == theirs["crs"] and ours["type"] == theirs["type"] and len(ours["features"]) == 40
    for f, g in zip(ours["features"], theirs["features"]):
        assert f["geometry"]["coordinates"] == g["geometry"]["coordinates"]      # ring order and coordinates
        assert f["properties"] == g["properties"] and f["geometry"]["type"] == g["geometry"]["type"]
    assert open(out).read() == open(golden).read()                                # ... and the text itself


# ---- boundary behaviour ----
def test_header_cites_the_reference_and_states_the_definition():
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    i = text.index("int dbm_grid_polygon_mask(")
    doc = text[max(0, i - 6000):i]
    assert re.search(r"data_prep\.py:582-616", doc)
    for phrase in ("even-odd", "(ya <= y) != (yb <= y)", "d2 <= buffer * buffer", "CANCEL", "Refused (status 1", "4028"):
        assert phrase in doc, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 6h." in design and "assumed, not measured" in design


def test_constants_agree_with_the_header():
    from deepbedmap_amd import polygons

    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"\b(DBM_POLY_[A-Z]+)\s*=\s*(\d+)", text)}
    assert flags == {"DBM_POLY_TILE": polygons.TILE, "DBM_POLY_CHUNK": polygons.EDGE_CHUNK}


def test_argument_errors_come_first_and_no_gpu_means_dbm_error():
    import deepbedmap_amd as dbm

    g = dbm.GridGeometry(*GEOM)
    box = dbm.Polygons.box(-1_599_000.0, -203_000.0, -1_595_000.0, -201_000.0)
    with pytest.raises(TypeError):
        dbm.polygon_mask(GEOM, SHAPE, box)
    with pytest.raises(TypeError):
        dbm.polygon_mask(g, SHAPE, box.edges)
    with pytest.raises(ValueError, match="empty"):
        dbm.polygon_mask(g, (0, 5), box)
    with pytest.raises(ValueError, match="2\\^31"):
        dbm.polygon_mask(g, (65536, 32768), box)
    with pytest.raises(ValueError, match="finite"):
        dbm.polygon_mask(g, SHAPE, box, buffer=float("nan"))
    with pytest.raises(ValueError, match="workspace_limit"):
        dbm.polygon_mask(g, SHAPE, box, workspace_limit=-1)
    with pytest.raises(TypeError):
        dbm.mask_outside(np.zeros(SHAPE, np.float32), box)
    with pytest.raises(TypeError):
        dbm.select_tiles(np.zeros(SHAPE, np.float32), box)
    with pytest.raises(ValueError):
        dbm.Polygons(np.zeros((3, 3)), 1)
    import torch

    if torch.cuda.is_available():
        return
    with pytest.raises(dbm.DbmError):
        dbm.polygon_mask(g, SHAPE, box)
    with pytest.raises(dbm.DbmError):
        dbm.mask_outside(dbm.Raster(np.zeros(SHAPE, np.float32), g), box)
    with pytest.raises(dbm.DbmError):
        dbm.select_tiles(dbm.Raster(np.zeros((40, 40), np.float32), g), box)
