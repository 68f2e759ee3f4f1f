"""The maps' vector layers on the host (deepbedmap_amd/overlay.py; reference paper_figures.py:533-562, :1039-1045): the
NumPy restatement of the rule (tests/overlay_restatement.py) against closed forms, `draw_layers_host` against the restatement byte for
byte on the scenes the GPU tests draw (tests/overlay_cases.py), the Layer constructors and every refusal.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlay_cases as oc  # noqa: E402
import overlay_restatement as orr  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402
from deepbedmap_amd import overlay  # noqa: E402

GEOM, PX = oc.GEOM, oc.PX


def test_constants_agree_with_the_header():
    import re

    text = open(os.path.join(os.path.dirname(HERE), "include", "dbm.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"\b(DBM_OVERLAY_[A-Z]+)\s*=\s*(\d+)", text)}
    assert flags == {"DBM_OVERLAY_SEGMENTS": overlay.SEGMENTS, "DBM_OVERLAY_DISCS": overlay.DISCS, "DBM_OVERLAY_TILE": overlay.TILE,
                     "DBM_OVERLAY_CHUNK": overlay.CHUNK}
    assert (oc.T, oc.K) == (overlay.TILE, overlay.CHUNK)


# ---- the restatement against closed forms ----
@pytest.mark.parametrize("d", [1, 2, 3, 5, 10])
def test_disc_on_a_centre_covers_the_lattice_points_within_its_radius(d):
    shape, (cc, cr) = (33, 47), (20, 16)
    m = orr.coverage(GEOM, shape, "discs", np.array([oc.xy(GEOM, cc, cr)]), d, 1)
    want = np.zeros(shape, dtype=np.int64)
    for r in range(shape[0]):
        for c in range(shape[1]):
            want[r, c] = Fraction(c - cc) ** 2 + Fraction(r - cr) ** 2 <= Fraction(d, 2) ** 2
    assert np.array_equal(m, want)
    assert m.sum() == {1: 1, 2: 5, 3: 9, 5: 21, 10: 81}[d]


def test_sub_samples_exactly_on_the_boundary_are_covered():
    """A horizontal segment along a row of centres, width 0.5, S = 2: the sub-samples lie at +-0.25 from the row, exactly on the pen's
    edge.  The comparison is closed: between the end points all four are covered; in the end pixels only the two towards the segment
    (the outer two are at 0.25 sqrt 2 from the end point)."""
    shape = (12, 20)
    seg = np.array([oc.segment(GEOM, 3, 5, 11, 5)])
    m = orr.coverage(GEOM, shape, "segments", seg, 0.5, 2)
    want = np.zeros(shape, dtype=np.int64)
    want[5, 4:11] = 4
    want[5, 3] = want[5, 11] = 2
    assert np.array_equal(m, want)
    # ... and a hair narrower covers nothing
    assert not orr.coverage(GEOM, shape, "segments", seg, np.nextafter(0.5, 0.0), 2).any()


def test_width_zero_paints_only_exact_hits():
    shape = (12, 20)
    # (lengths of 8 pixels: t = k / 8 and t ex are exact, so the centres on the segments have d2 = 0)
    segs = np.array([oc.segment(GEOM, 3, 5, 11, 5), oc.segment(GEOM, 2, 2, 10, 10), oc.segment(GEOM, 15, 1, 15, 1)])
    m = orr.coverage(GEOM, shape, "segments", segs, 0.0, 1)
    want = np.zeros(shape, dtype=np.int64)
    want[5, 3:12] = 1
    want[np.arange(2, 11), np.arange(2, 11)] = 1
    want[1, 15] = 1
    assert np.array_equal(m, want)
    for S in (2, 4):       # no sub-sample lies on a row or a column of centres
        assert not orr.coverage(GEOM, shape, "segments", segs[[0, 2]], 0.0, S).any()
    # ... but the sub-samples (i, i) lie on the diagonal: with S = 2 those at k - 0.25 and k + 0.25 that are within the segment's ends
    m = orr.coverage(GEOM, shape, "segments", segs[[1]], 0.0, 2)
    want = np.zeros(shape, dtype=np.int64)
    want[np.arange(3, 10), np.arange(3, 10)] = 2
    want[2, 2] = want[10, 10] = 1
    assert np.array_equal(m, want)
    # a disc of diameter 0 on a sub-sample of S = 2 covers that one
    m = orr.coverage(GEOM, shape, "discs", np.array([oc.xy(GEOM, 7.25, 3.75)]), 0.0, 2)
    assert m.sum() == 1 and m[4, 7] == 1


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_blend_formula(S, channels):
    """m in {0, 1, S^2} with A in {0, 128, 255}: a disc of diameter 0 on one sub-sample of pixel (4, 7), a disc that swallows pixel
    (9, 12) whole; every other pixel keeps its bytes."""
    shape = (12, 20)
    first = (1 / (2 * S) - 0.5) if S > 1 else 0.0
    discs_one = np.array([oc.xy(GEOM, 7 + first, 4 + first)])
    discs_all = np.array([oc.xy(GEOM, 12, 9)])
    dst = oc.destination(shape, channels, seed=S)
    D = S * S * 255
    for A in (0, 128, 255):
        rgba = (200, 17, 255, A)
        got = orr.paint(dst, GEOM, [("discs", discs_one, 0.0, rgba), ("discs", discs_all, 1.5, rgba)], S)
        m = orr.coverage(GEOM, shape, "discs", discs_one, 0.0, S) + orr.coverage(GEOM, shape, "discs", discs_all, 1.5, S)
        assert m[4, 7] == 1 and m[9, 12] == S * S
        for (r, c) in ((4, 7), (9, 12)):
            w = int(m[r, c]) * A
            for ch in range(channels):
                src = rgba[ch] if ch < 3 else 255
                assert got[r, c, ch] == (w * src + (D - w) * int(dst[r, c, ch]) + D // 2) // D == orr.blend_value(m[r, c], A, src, dst[r, c, ch], S)
        if A == 255:
            assert tuple(got[9, 12, :3]) == rgba[:3] and (channels == 3 or got[9, 12, 3] == 255)
        if A == 0:
            assert np.array_equal(got, dst)
        untouched = m == 0
        assert np.array_equal(got[untouched], dst[untouched])


# ---- draw_layers_host against the restatement, on the GPU tests' scenes ----
def host(dst, geom, layers, S):
    return dbm.draw_layers_host(dst, dbm.GridGeometry(*geom), oc.layers_of(dbm, layers), samples=S)


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_statement_equals_the_restatement_on_every_shape(shape):
    for S in (1, 2, 4):
        for channels in (3, 4):
            dst = oc.destination(shape, channels, seed=S + channels, transparent=True)
            layers = oc.two_layers(GEOM, shape, 2.5)
            want = orr.paint(dst, GEOM, layers, S)
            assert np.array_equal(host(dst, GEOM, layers, S), want), (S, channels)
    assert shape == (1, 1) or not np.array_equal(want, dst)


@pytest.mark.parametrize("name", list(oc.GEOMETRIES))
@pytest.mark.parametrize("size", oc.SIZES)
def test_host_statement_on_every_geometry_and_size(name, size):
    geom, shape = oc.GEOMETRIES[name], (33, 47)
    dst = oc.destination(shape, 4, seed=3)
    for S in (1, 4):
        layers = oc.two_layers(geom, shape, size)
        want = orr.paint(dst, geom, layers, S)
        assert np.array_equal(host(dst, geom, layers, S), want), S
        both = orr.paint(dst, geom, layers[::-1], S)
        assert np.array_equal(host(dst, geom, layers[::-1], S), both)
        if size == 40.0:
            assert not np.array_equal(want, both)     # two layers that overlap: the order shows


@pytest.mark.parametrize("kind", ["segments", "discs"])
@pytest.mark.parametrize("count", oc.COUNTS)
def test_host_statement_on_every_primitive_count(count, kind):
    shape = (oc.T + 1, 2 * oc.T + 1)
    table = oc.padded(GEOM, shape, count, 2.5, kind)
    assert len(table) == count
    dst = oc.destination(shape, 3, seed=count)
    layers = [(kind, table, 2.5, oc.BLUE)]
    want = orr.paint(dst, GEOM, layers, 2)
    assert np.array_equal(host(dst, GEOM, layers, 2), want)
    assert (count == 0) == np.array_equal(want, dst)
    perm = np.random.default_rng(1).permutation(count)
    assert np.array_equal(orr.paint(dst, GEOM, [(kind, table[perm], 2.5, oc.BLUE)], 2), want)


def test_overflowing_pixel_coordinates_cover_nothing():
    shape = (8, 9)
    geom = (0.0, 0.0, 1e-300, -1e-300)
    segs = np.array([[1e20, -3e-300, 4e-300, -3e-300], [2e-300, -1e-300, 6e-300, -5e-300]])
    dst = oc.destination(shape, 4)
    want = orr.paint(dst, geom, [("segments", segs, 1.0, oc.ORANGE)], 2)
    assert np.array_equal(want, orr.paint(dst, geom, [("segments", segs[1:], 1.0, oc.ORANGE)], 2)) and not np.array_equal(want, dst)
    assert np.array_equal(host(dst, geom, [("segments", segs, 1.0, oc.ORANGE)], 2), want)


# ---- Layer ----
def test_boxes_are_four_segments_each_in_order():
    bounds = np.array([[0.0, 1.0, 2.0, 3.0], [-10.0, -20.0, -5.0, -15.0]])
    layer = dbm.Layer.boxes(bounds, 1.0, (255, 165, 0))
    assert layer.kind == "segments" and layer.size == 1.0 and layer.colour == (255, 165, 0, 255) and not layer.resident and len(layer) == 8
    assert np.array_equal(layer.primitives, np.array([
        [0, 1, 2, 1], [2, 1, 2, 3], [2, 3, 0, 3], [0, 3, 0, 1],
        [-10, -20, -5, -20], [-5, -20, -5, -15], [-5, -15, -10, -15], [-10, -15, -10, -20]], dtype=np.float64))
    assert len(dbm.Layer.boxes(np.zeros((0, 4)), 1.0, (1, 2, 3))) == 0
    assert len(dbm.Layer.boxes({"a": [(0, 0, 1, 1)], "b": [(1, 1, 2, 2), (3, 3, 4, 4)]}, 1.0, (1, 2, 3))) == 12
    with pytest.raises(ValueError, match="bounds"):
        dbm.Layer.boxes(np.zeros((3, 3)), 1.0, (1, 2, 3))


class Frame:
    """What `points_table` asks of a DataFrame: `.columns` and `frame[columns].to_numpy()`."""

    def __init__(self, **columns):
        self.data = {k: np.asarray(v, dtype=np.float64) for k, v in columns.items()}
        self.columns = list(self.data)

    def __getitem__(self, names):
        return Frame(**{k: self.data[k] for k in names})

    def to_numpy(self):
        return np.stack([self.data[k] for k in self.columns], axis=1)


def test_points_accept_a_dataframe():
    x, y, z = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]
    frames = [Frame(x=x, y=y, z=z), Frame(x=x, y=y)]
    try:
        import pandas as pd

        frames += [pd.DataFrame({"z": z, "y": y, "x": x}), pd.DataFrame({"x": x, "y": y})]
    except ImportError:
        pass
    for frame in frames:
        layer = dbm.Layer.points(frame, 3, (1, 2, 3, 4))
        assert layer.kind == "discs" and layer.colour == (1, 2, 3, 4) and layer.size == 3.0
        assert np.array_equal(layer.primitives[:, :2], np.stack([x, y], axis=1)) and layer.primitives.shape[1] in (2, 3)
    three, two = dbm.Layer.points(np.stack([x, y, z], axis=1), 3, (9, 9, 9)), dbm.Layer.points(np.stack([x, y], axis=1), 3, (9, 9, 9))
    canvas = np.zeros((8, 8, 3), np.uint8)
    g = dbm.GridGeometry(0.0, 7.0, 1.0, -1.0)
    assert np.array_equal(dbm.draw_layers_host(canvas, g, [three]), dbm.draw_layers_host(canvas, g, [two]))
    assert dbm.draw_layers_host(canvas, g, [three]).any()


def test_refusals():
    canvas, g = np.zeros((8, 8, 4), np.uint8), dbm.GridGeometry(0.0, 7.0, 1.0, -1.0)
    segs, pts = np.array([[1.0, 1.0, 5.0, 5.0], [2.0, 2.0, 3.0, 3.0]]), np.array([[1.0, 1.0], [2.0, 5.0]])
    good = dbm.Layer.lines(segs, 1.0, (1, 2, 3))
    nan_last = segs.copy()
    nan_last[-1, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        dbm.Layer.lines(nan_last, 1.0, (1, 2, 3))
    with pytest.raises(ValueError, match="non-finite"):
        dbm.Layer.points(np.array([[1.0, np.inf]]), 1.0, (1, 2, 3))
    dbm.Layer.points(np.array([[1.0, 2.0, np.nan]]), 1.0, (1, 2, 3))      # z is not a coordinate
    for size in (-1.0, np.nan, np.inf, "wide"):
        with pytest.raises(ValueError, match="width"):
            dbm.Layer.lines(segs, size, (1, 2, 3))
        with pytest.raises(ValueError, match="diameter"):
            dbm.Layer.points(pts, size, (1, 2, 3))
    with pytest.raises(ValueError, match="stride"):
        dbm.Layer.points(np.zeros((3, 4)), 1.0, (1, 2, 3))
    with pytest.raises(ValueError, match="stride"):
        dbm.Layer.points(np.zeros((3, 1)), 1.0, (1, 2, 3))
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        dbm.Layer.lines(np.zeros((3, 2)), 1.0, (1, 2, 3))
    for colour in ((1, 2), (1, 2, 3, 4, 5), (1, 2, 256), (1, -2, 3), (1.5, 2, 3), "red"):
        with pytest.raises(ValueError, match="colour"):
            dbm.Layer.lines(segs, 1.0, colour)
    with pytest.raises(ValueError, match="kind"):
        dbm.Layer("arcs", segs, 1.0, (1, 2, 3))
    for S in (3, 0, 8, 1.5, True):
        with pytest.raises(ValueError, match="samples"):
            dbm.draw_layers_host(canvas, g, [good], samples=S)
    for channels in (2, 1, 5):
        with pytest.raises(ValueError, match="channels"):
            dbm.draw_layers_host(np.zeros((8, 8, channels), np.uint8), g, [good])
    with pytest.raises(ValueError, match="uint8"):
        dbm.draw_layers_host(np.zeros((8, 8, 4), np.float32), g, [good])
    with pytest.raises(ValueError, match="Layer"):
        dbm.draw_layers_host(canvas, g, [segs])
    with pytest.raises(ValueError, match="geometry"):
        dbm.draw_layers_host(canvas, (0.0, 0.0, 0.0, 1.0), [good])
    with pytest.raises(ValueError, match="DeviceArray"):
        dbm.draw_layers(canvas, g, [good])
    # nothing was drawn on the argument
    assert not canvas.any() and dbm.draw_layers_host(canvas, g, [good]).any() and not canvas.any()


def test_render_map_needs_a_geometry(tmp_path):
    layer = dbm.Layer.lines(np.array([[1.0, 1.0, 5.0, 5.0]]), 1.0, (1, 2, 3))
    with pytest.raises(ValueError, match="Raster"):
        dbm.render_map(np.zeros((8, 8), np.float32), str(tmp_path / "x.png"), dbm.grey_cpt(), [layer])
    assert not os.path.exists(str(tmp_path / "x.png"))


def test_training_tiles_as_boxes():
    """tests/golden/tiles_3031_head.geojson through `read_tiles_geojson` and `Layer.boxes` (paper_figures.py:545-562) onto a canvas of
    1 km pixels around the tiles."""
    tiles = dbm.read_tiles_geojson(os.path.join(HERE, "golden", "tiles_3031_head.geojson"))
    bounds = np.array([b for rows in tiles.values() for b in rows])
    assert len(bounds) > 8
    layer = dbm.Layer.boxes(tiles, 1.0, (238, 154, 0))
    assert len(layer) == 4 * len(bounds) and np.array_equal(layer.primitives[4], [bounds[1, 0], bounds[1, 1], bounds[1, 2], bounds[1, 1]])
    west, north = bounds[:, 0].min() - 5000.0, bounds[:, 3].max() + 5000.0
    H, W = int((north - bounds[:, 1].min() + 5000.0) // 1000.0), int((bounds[:, 2].max() + 5000.0 - west) // 1000.0)
    geom = (west + 500.0, north - 500.0, 1000.0, -1000.0)
    dst = oc.destination((H, W), 4, seed=9, transparent=True)
    got = dbm.draw_layers_host(dst, dbm.GridGeometry(*geom, registration="pixel"), [layer], samples=4)
    want = orr.paint(dst, geom, [("segments", layer.primitives, 1.0, (238, 154, 0, 255))], 4)
    assert np.array_equal(got, want)
    changed = (got != dst).any(axis=2)
    assert 0 < changed.sum() < H * W
