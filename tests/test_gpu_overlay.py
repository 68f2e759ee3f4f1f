"""-m gpu: dbm_image_overlay (overlay.hip) and deepbedmap_amd/overlay.py against the float64 NumPy restatement of the rule
(tests/overlay_restatement.py, itself checked against closed forms in tests/test_overlay_host.py); reference
paper_figures.py:533-562, :1039-1045.

Every comparison is byte for byte, without tolerance: a pixel is a pure function of identically rounded float64 operations and of
integers, and culling, binning and the skips of the paint kernel may never change it.  Images and primitive counts sit on the kernel's
own boundaries (T = overlay.TILE, K = overlay.CHUNK); the scenes are tests/overlay_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlay_cases as oc  # noqa: E402
import overlay_restatement as orr  # noqa: E402

pytestmark = pytest.mark.gpu

from deepbedmap_amd import overlay as _ov  # noqa: E402

T, K = _ov.TILE, _ov.CHUNK
GEOM, PX = oc.GEOM, oc.PX


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    assert (T, K) == (oc.T, oc.K)
    return d


@pytest.fixture(scope="module")
def ctx(dbm):
    return dbm.default_context()


def drawn(dbm, ctx, dst, geom, layers, S, limit=None):
    """`layers` (restatement tuples or Layer objects) painted into a resident copy of dst."""
    image = dbm.DeviceArray(dst.shape, ctx, dtype=np.uint8).set(dst)
    layers = [la if isinstance(la, dbm.Layer) else oc.layers_of(dbm, [la])[0] for la in layers]
    out = dbm.draw_layers(image, dbm.GridGeometry(*geom), layers, samples=S, workspace_limit=limit)
    assert out is image
    return image.get()


def check(dbm, ctx, dst, geom, layers, S, limit=None, want=None):
    want = orr.paint(dst, geom, layers, S) if want is None else want
    got = drawn(dbm, ctx, dst, geom, layers, S, limit)
    bad = np.argwhere((got != want).any(axis=2))
    assert np.array_equal(got, want), (dst.shape, S, limit, len(bad), bad[:5])
    return want


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_equals_the_restatement(dbm, ctx, shape):
    """Every shape: S in {1, 2, 4}, channels 3 and 4, alpha 255 (the segments) and 128 (the discs), random destinations, one of them
    with alpha 0 where relief_image puts nodata."""
    for S in (1, 2, 4):
        for channels in (3, 4):
            dst = oc.destination(shape, channels, seed=S + channels, transparent=(S == 4))
            want = check(dbm, ctx, dst, GEOM, oc.two_layers(GEOM, shape, 2.5), S)
    assert shape == (1, 1) or not np.array_equal(want, dst)


@pytest.mark.parametrize("name", ["dy_positive", "dx_negative"])
def test_flipped_axes(dbm, ctx, name):
    geom = oc.GEOMETRIES[name]
    for shape in ((T + 1, 2 * T + 1), (97, 131)):
        dst = oc.destination(shape, 4, seed=2)
        want = check(dbm, ctx, dst, geom, oc.two_layers(geom, shape, 2.5), 4)
        assert not np.array_equal(want, dst)
        assert not np.array_equal(want, orr.paint(dst, GEOM, oc.two_layers(geom, shape, 2.5), 4))     # (the geometry matters)


@pytest.mark.parametrize("name", list(oc.GEOMETRIES))
@pytest.mark.parametrize("size", oc.SIZES, ids=lambda s: f"size{s}")
def test_sizes(dbm, ctx, name, size):
    """0 (exact hits only), 1, 2.5 and 40 pixels -- wider than two tiles: one primitive lands in many bins -- on either schedule."""
    geom, shape = oc.GEOMETRIES[name], (33, 47)
    dst = oc.destination(shape, 4, seed=3)
    for S in (1, 2, 4):
        want = check(dbm, ctx, dst, geom, oc.two_layers(geom, shape, size), S)
        check(dbm, ctx, dst, geom, oc.two_layers(geom, shape, size), S, limit=1, want=want)
    if size == 40.0:
        stats = _ov.last_stats(ctx)
        assert stats["schedule"] == 0 and stats["entries"] > stats["kept"] > 0


@pytest.mark.parametrize("kind", ["segments", "discs"])
@pytest.mark.parametrize("count", oc.COUNTS)
def test_primitive_counts_around_the_chunk(dbm, ctx, count, kind):
    shape = (T + 1, 2 * T + 1)
    table = oc.padded(GEOM, shape, count, 2.5, kind)
    assert len(table) == count
    dst = oc.destination(shape, 3, seed=count)
    for S in (2, 4):
        want = None
        for limit in (None, 1):     # binned, and every tile over the whole culled list
            want = check(dbm, ctx, dst, GEOM, [(kind, table, 2.5, oc.BLUE)], S, limit=limit, want=want)
            stats = _ov.last_stats(ctx)
            assert stats["primitives"] == count and stats["schedule"] == (1 if limit is None and count else 0)
            if count > K:
                assert 0 < stats["kept"] < count        # the far-away ones were dropped
        assert (count == 0) == np.array_equal(want, dst)


def test_every_path_gives_the_same_bytes(dbm, ctx):
    """Host tables and resident ones (Polygons.device, DevicePoints with 2 and with 3 columns), both schedules, a permutation, the
    same call again."""
    shape, S = (97, 131), 4
    g = dbm.GridGeometry(*GEOM)
    dst = oc.destination(shape, 4, seed=5, transparent=True)
    segs, pts = oc.padded(GEOM, shape, 2 * K + 3, 2.5, "segments"), oc.padded(GEOM, shape, 2 * K + 3, 2.5, "discs")
    layers = [("segments", segs, 2.5, oc.ORANGE), ("discs", pts, 2.5, oc.BLUE)]
    want = orr.paint(dst, GEOM, layers, S)
    assert not np.array_equal(want, dst)
    perm = np.random.default_rng(5).permutation(len(segs))
    pts3 = np.concatenate([pts, np.full((len(pts), 1), np.nan)], axis=1)          # z is not read
    poly = dbm.Polygons(segs, n_rings=1)
    lines, lines_perm = dbm.Layer.lines(poly, 2.5, oc.ORANGE), dbm.Layer.lines(dbm.Polygons(segs[perm], n_rings=1), 2.5, oc.ORANGE)
    assert lines.resident and lines.primitives is poly
    variants = {
        "host": layers,
        "again": layers,
        "resident": [lines, dbm.Layer.points(dbm.DevicePoints(pts, ctx), 2.5, oc.BLUE)],
        "three columns": [lines, dbm.Layer.points(dbm.DevicePoints(pts3, ctx), 2.5, oc.BLUE)],
        "host three columns": [layers[0], dbm.Layer.points(pts3, 2.5, oc.BLUE)],
        "permuted": [lines_perm, ("discs", pts[perm], 2.5, oc.BLUE)],
    }
    first = poly.device(ctx)
    for name, ls in variants.items():
        for limit in (None, 1):
            got = drawn(dbm, ctx, dst, GEOM, ls, S, limit)
            assert np.array_equal(got, want), (name, limit)
            stats = _ov.last_stats(ctx)
            assert stats["schedule"] == (1 if limit is None else 0) and stats["primitives"] == len(pts), (name, limit)
            assert 0 < stats["kept"] < len(pts) and stats["entries"] >= stats["kept"]
    assert poly.device(ctx) == first          # one upload, used where it lies
    assert isinstance(dbm.Layer.points(dbm.DevicePoints(pts, ctx), 1, oc.BLUE).primitives, dbm.DevicePoints)
    # the host statement reads a resident layer back
    assert np.array_equal(dbm.draw_layers_host(dst, g, variants["resident"][:1] + [dbm.Layer.points(dbm.DevicePoints(pts, ctx), 2.5, oc.BLUE)],
                                               samples=S), want)


def test_layers_blend_in_list_order(dbm, ctx):
    shape = (33, 47)
    dst = oc.destination(shape, 4, seed=8)
    a, b = oc.two_layers(GEOM, shape, 5.0, first=(250, 10, 10, 128), second=oc.BLUE)
    ab = check(dbm, ctx, dst, GEOM, [a, b], 4)
    ba = check(dbm, ctx, dst, GEOM, [b, a], 4)
    both = (orr.coverage(GEOM, shape, a[0], a[1], a[2], 4) > 0) & (orr.coverage(GEOM, shape, b[0], b[1], b[2], 4) > 0)
    assert both.any() and (ab[both] != ba[both]).any() and np.array_equal(ab[~both], ba[~both])


class Abi:
    """dbm_image_overlay called directly."""

    def __init__(self, dbm, ctx):
        self.lib, self.L, self.ctx = dbm._lib.lib(), dbm._lib, ctx

    def __call__(self, dst, geom, table, kind, stride=None, size=2.5, rgba=oc.ORANGE, S=4, limit=0, device=False, handle="ctx", channels=None,
                 shape=None, null=()):
        t = np.ascontiguousarray(table, dtype=np.float64)
        image = self.ctx.malloc(max(dst.nbytes, 32))
        self.ctx.upload(image, dst)
        tptr = None
        if device:
            tptr = self.ctx.malloc(max(t.nbytes, 32))
            self.ctx.upload(tptr, t)
        g = np.asarray(geom, dtype=np.float64)
        H, W = dst.shape[:2] if shape is None else shape
        try:
            rc = self.lib.dbm_image_overlay(
                self.ctx.handle if handle == "ctx" else None, None if "image" in null else C.c_void_p(image), H, W,
                dst.shape[2] if channels is None else channels, None if "geom" in null else g.ctypes.data_as(C.POINTER(C.c_double)),
                None if "prims" in null else (C.c_void_p(tptr) if device else t.ctypes.data_as(C.c_void_p)), len(t),
                kind, t.shape[1] if stride is None else stride, size, None if "rgba" in null else bytes(rgba), S, limit,
                self.L.DEVICE_PTRS if device else 0)
            out = self.ctx.download(image, np.uint8, dst.shape)
        finally:
            self.ctx.free(image)
            if tptr:
                self.ctx.free(tptr)
        return rc, out


def test_refusals_leave_the_image_untouched(dbm, ctx):
    abi = Abi(dbm, ctx)
    shape = (T + 1, 2 * T + 1)
    dst = oc.destination(shape, 4, seed=4)
    segs, pts = oc.padded(GEOM, shape, K + 1, 2.5, "segments"), oc.padded(GEOM, shape, K + 1, 2.5, "discs")
    nan_last, inf_first, nan_point = segs.copy(), segs.copy(), np.concatenate([pts, np.zeros((len(pts), 1))], axis=1)
    nan_last[-1, 3] = np.nan
    inf_first[0, 0] = np.inf
    nan_point[-1, 1] = np.nan
    SEG, DISC = _ov.SEGMENTS, _ov.DISCS
    rc, out = abi(dst, GEOM, segs, SEG)
    assert rc == 0 and np.array_equal(out, orr.paint(dst, GEOM, [("segments", segs, 2.5, oc.ORANGE)], 4))
    cases = {
        "null ctx": dict(handle=None),
        "null image": dict(null=("image",)),
        "null geom": dict(null=("geom",)),
        "null rgba": dict(null=("rgba",)),
        "null prims": dict(null=("prims",)),
        "H 0": dict(shape=(0, shape[1])),
        "W negative": dict(shape=(shape[0], -3)),
        "H W 2^31": dict(shape=(65536, 32768)),
        "channels 2": dict(channels=2),
        "channels 5": dict(channels=5),
        "geom nan": dict(geom=(np.nan, GEOM[1], PX, -PX)),
        "dx zero": dict(geom=(GEOM[0], GEOM[1], 0.0, -PX)),
        "dy inf": dict(geom=(GEOM[0], GEOM[1], PX, np.inf)),
        "kind 2": dict(kind=2),
        "segments stride 3": dict(stride=3),
        "discs stride 4": dict(kind=DISC, stride=4),
        "discs stride 1": dict(kind=DISC, stride=1),
        "size negative": dict(size=-1.0),
        "size nan": dict(size=np.nan),
        "size inf": dict(size=np.inf),
        "samples 3": dict(S=3),
        "samples 0": dict(S=0),
        "samples 8": dict(S=8),
        "host nan in the last segment": dict(table=nan_last),
        "host inf in the first segment": dict(table=inf_first),
        "device nan in the last segment": dict(table=nan_last, device=True),
        "device inf in the first segment": dict(table=inf_first, device=True),
        "device nan in the last point": dict(table=nan_point, kind=DISC, device=True),
        "host nan in the last point": dict(table=nan_point, kind=DISC),
    }
    for name, kw in cases.items():
        args = dict(geom=GEOM, table=segs, kind=SEG)
        args.update(kw)
        rc, out = abi(dst, args.pop("geom"), args.pop("table"), args.pop("kind"), **args)
        assert rc == 1, name
        assert np.array_equal(out, dst), name
    # z may be anything; NULL primitives are fine without primitives
    nan_z = np.concatenate([pts, np.full((len(pts), 1), np.nan)], axis=1)
    for device in (False, True):
        rc, out = abi(dst, GEOM, nan_z, DISC, device=device)
        assert rc == 0 and np.array_equal(out, orr.paint(dst, GEOM, [("discs", pts, 2.5, oc.ORANGE)], 4))
    rc, out = abi(dst, GEOM, np.zeros((0, 4)), SEG, null=("prims",))
    assert rc == 0 and np.array_equal(out, dst)
    # Python: the refused layer raises before it writes; a DevicePoints with a NaN is found by its cull pass
    image = dbm.DeviceArray(dst.shape, ctx, dtype=np.uint8).set(dst)
    with pytest.raises(dbm.DbmError, match="non-finite"):
        dbm.draw_layers(image, dbm.GridGeometry(*GEOM), [dbm.Layer.points(dbm.DevicePoints(nan_point, ctx), 2.5, oc.BLUE)])
    assert np.array_equal(image.get(), dst)
    with pytest.raises(ValueError, match="samples"):
        dbm.draw_layers(image, dbm.GridGeometry(*GEOM), [dbm.Layer.lines(segs, 1.0, oc.BLUE)], samples=3)
    assert np.array_equal(image.get(), dst)


def test_render_map(dbm, ctx, tmp_path):
    """The product: a 97 x 131 Raster, reduce=1, the grounding line and survey points over the relief, read back from the PNG."""
    from deepbedmap_amd import relief

    shape = (97, 131)
    r = np.random.default_rng(6)
    z = (r.standard_normal(shape) * 800.0).astype(np.float32)
    z[10:20, 30:50] = np.nan
    geometry = dbm.GridGeometry(GEOM[0], GEOM[1], PX, -PX, registration="pixel")
    raster = dbm.Raster(dbm.to_device(z), geometry)
    cpt = dbm.make_cpt(dbm.read_cpt(os.path.join(HERE, "golden", "oleron.cpt")), (-2000.0, 2000.0))
    poly = dbm.Polygons(oc.zoo_segments(GEOM, shape, 1.5), n_rings=1)
    points = dbm.DevicePoints(np.concatenate([oc.zoo_discs(GEOM, shape, 3.0), np.zeros((7, 1))], axis=1), ctx)
    layers = [dbm.Layer.lines(poly, 1.5, (0, 0, 0)), dbm.Layer.points(points, 3.0, (255, 165, 0, 200))]
    path, image_geometry = dbm.render_map(raster, str(tmp_path / "map.png"), cpt, layers, reduce=1)
    assert image_geometry == relief.reduced_geometry(geometry, 1)
    level, level_geometry = relief.prepared_plane("test", raster, reduce=1)
    assert level_geometry == image_geometry and tuple(level.shape[-2:]) == (49, 66)
    bare = dbm.relief_image_host(level.get().reshape(49, 66), cpt)
    want = dbm.draw_layers_host(bare, image_geometry, layers)
    got = dbm.read_png(path)
    assert np.array_equal(got, want) and not np.array_equal(got, bare)
    assert np.array_equal(want, orr.paint(bare, (image_geometry.x0, image_geometry.y0, image_geometry.dx, image_geometry.dy),
                                          [("segments", poly.edges, 1.5, (0, 0, 0, 255)), ("discs", oc.zoo_discs(GEOM, shape, 3.0), 3.0, (255, 165, 0, 200))], 4))
    assert [float(v) for v in open(str(tmp_path / "map.pgw")).read().split()] == [2 * PX, 0.0, 0.0, -2 * PX, GEOM[0] + PX / 2, GEOM[1] - PX / 2]
    with pytest.raises(ValueError, match="Raster"):
        dbm.render_map(dbm.to_device(z), str(tmp_path / "bare.png"), cpt, layers)


def test_an_image_beyond_two_gibibytes(dbm, ctx):
    """(23 000, 23 500, 4): 2.16e9 bytes, pixel offsets beyond 2^31.  A handful of primitives near the last rows; the touched band is
    compared against the restatement run on that band, rows elsewhere against the destination."""
    H, W, channels, S = 23_000, 23_500, 4, 2
    geom = (-2_937_500.0, 2_875_000.0, PX, -PX)
    try:
        image = dbm.DeviceArray((H, W, channels), ctx, dtype=np.uint8)
    except dbm.DbmError as e:
        pytest.skip(f"no room for a {H * W * channels} byte image: {e}")
    ctx.call("dbm_fill_f32", C.c_void_p(image.ptr), H * W, C.c_float(1.5))       # every pixel: the bytes of 1.5f, 00 00 c0 3f
    pattern = np.frombuffer(np.float32(1.5).tobytes(), dtype=np.uint8)
    band0, row_bytes = H - 20, W * channels
    band = oc.destination((H - band0, W), channels, seed=12)
    ctx.upload(image.ptr + band0 * row_bytes, band)
    segs = np.array([oc.segment(geom, W - 300.5, H - 12.25, W + 3.0, H - 2.0), oc.segment(geom, 5.0, H - 6.0, 900.25, H - 6.0),
                     oc.segment(geom, W - 1, H - 1, W - 1, H - 1)])
    pts = np.array([oc.xy(geom, W - 40.0, H - 5.5), oc.xy(geom, 0.0, H - 1.0), oc.xy(geom, W // 2 + 0.5, H + 0.25)])
    layers = [("segments", segs, 3.0, oc.ORANGE), ("discs", pts, 9.0, oc.BLUE)]
    dbm.draw_layers(image, geom, oc.layers_of(dbm, layers), samples=S)
    assert _ov.last_stats(ctx)["schedule"] == 1
    want = orr.paint(band, geom, layers, S, rows=(band0, H, H))
    got = ctx.download(image.ptr + band0 * row_bytes, np.uint8, band.shape)
    assert np.array_equal(got, want) and not np.array_equal(want, band)
    assert (want[-1, -1] != band[-1, -1]).any() and (want[2:] != band[2:]).any()
    rows = [0, 1, band0 - 1] + [int(v) for v in np.random.default_rng(3).integers(2, band0 - 1, size=5)]
    rows += [int((2 ** 31) // row_bytes), int((2 ** 31) // row_bytes) + 1]     # the rows on either side of byte 2^31
    for row in rows:
        got = ctx.download(image.ptr + row * row_bytes, np.uint8, (W, channels))
        assert (got == pattern[None, :]).all(), row
