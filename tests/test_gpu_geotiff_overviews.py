"""-m gpu: the overview pyramid built next to the canvas (dbm_grid_overviews, pyramid.hip; DESIGN.md 6j, "Overviews") against its NumPy
statement `overview_pyramid` -- itself checked against the loop-per-pixel restatement in tests/test_geotiff_overviews_host.py --, the
files `write_geotiff_resident(overviews=)` writes against the host writer's, and the readers on an overview.  The definition is exact
(one float32 sum in a fixed order, one IEEE division, rint): no comparison has a tolerance.

Shapes: the host test's -- 1 x 1 to 3 x 5 (single, partial windows), 257 x 513 and 300 x 520 (several 64 x 64 tiles, ragged in both
directions; 513 and 257 take the scalar loads, 520 the 16-byte ones) -- plus 2 x 70001 (1094 tiles in a row, an odd width) and 515 x 67
(nine tiles down), each down to 1 x 1: four launches of three levels and a remainder."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pyramid_restatement as pr  # noqa: E402
import test_geotiff_open_host as host  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = host.BOUND
bits = host.bits
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (257, 513), (300, 520), (2, 70001), (515, 67)]
NODATA = -2000


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


def canvas(shape, dtype):
    """A float32 canvas whose cast to `dtype` is the branch plane of the host test; for int16 with fractions, NaN and values beyond int16
    on top, so that level 0 really is the cast (NaN -> 0, 40000.7 -> -25536)."""
    plane = pr.branch_plane(shape[0], shape[1], dtype, NODATA).astype(np.float32)
    if dtype == "int16" and plane.size >= 15:
        flat = plane.reshape(-1)
        keep = flat != NODATA
        flat[keep] += np.where(flat[keep] >= 0, np.float32(0.75), np.float32(-0.75))   # truncation brings them back
        flat[7] = np.nan
        flat[11] = 40000.7
        flat[13] = -1e20
    return plane


def as_written(a, dtype):
    with np.errstate(invalid="ignore"):
        return a.astype(dtype)


@pytest.fixture(scope="module")
def pyramids(dbm):
    """{(shape, dtype): (canvas, overview_pyramid of the canvas as written, down to 1 x 1)}, computed once."""
    out = {}
    for shape in SHAPES:
        for dtype in ("int16", "float32"):
            a = canvas(shape, dtype)
            out[shape, dtype] = (a, dbm.overview_pyramid(as_written(a, dtype), pr.max_levels(*shape), NODATA))
    return out


def call_overviews(ctx, plane, H, W, sample_type, nodata, levels, out):
    from deepbedmap_amd.resident import devptr

    ctx.call("dbm_grid_overviews", devptr(plane), H, W, sample_type, C.byref(C.c_double(nodata)) if nodata is not None else None, levels,
             devptr(out))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_entry_point_equals_the_numpy_statement(dbm, pyramids, shape, dtype):
    a, want = pyramids[shape, dtype]
    H, W = shape
    dev = dbm.to_device(a)
    total = sum(w.size for w in want)
    guard = 64
    out = dbm.DeviceArray((total + guard,)).set(np.full(total + guard, 12345.0, dtype=np.float32))
    call_overviews(dev.ctx, dev, H, W, 1 if dtype == "int16" else 4, float(NODATA), len(want), out)
    got = out.get()
    assert (got[total:] == 12345.0).all()   # nothing behind the last level
    at = 0
    for k, w in enumerate(want):
        level = got[at:at + w.size].reshape(w.shape)
        at += w.size
        assert np.array_equal(bits(level), bits(w.astype(np.float32))), (k, w.shape, np.flatnonzero(bits(level).ravel() != bits(w.astype(np.float32)).ravel())[:5])
    assert np.array_equal(bits(dev.get()), bits(a))   # the canvas is only read
    # fewer levels are a prefix: 1, 2 (one launch, the third result unused) and 4 (a second launch of one level)
    for levels in (n for n in (1, 2, 4) if n < len(want)):
        size = sum(w.size for w in want[:levels])
        part = dbm.DeviceArray((size + guard,)).set(np.full(size + guard, 12345.0, dtype=np.float32))
        call_overviews(dev.ctx, dev, H, W, 1 if dtype == "int16" else 4, float(NODATA), levels, part)
        p = part.get()
        assert np.array_equal(bits(p[:size]), bits(got[:size])) and (p[size:] == 12345.0).all()


def test_an_unaligned_plane_and_nan_nodata(dbm, pyramids):
    """A plane that does not start on 16 bytes (W % 4 == 0, yet scalar loads), and NaN as the nodata value."""
    from deepbedmap_amd.resident import DeviceArray

    a, _ = pyramids[(300, 520), "float32"]
    H, W = 298, 520
    flat = dbm.to_device(a.reshape(-1))
    view = DeviceArray((H, W), flat.ctx, ptr=flat.ptr + 4 * 521, owner=flat)
    sub = a.reshape(-1)[521:521 + H * W].reshape(H, W)
    for nodata in (float(NODATA), float("nan")):
        want = dbm.overview_pyramid(sub, 5, nodata)
        got = dbm.build_overviews(view, 5, nodataval=nodata)
        assert all(np.array_equal(bits(g.get()), bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_build_overviews_on_a_device_array(dbm, pyramids, dtype):
    a, want = pyramids[(300, 520), dtype]
    for dev in (dbm.to_device(a), dbm.to_device(a[None])):
        got = dbm.build_overviews(dev, "auto", dtype=dtype, nodataval=NODATA)
        assert [g.shape for g in got] == [(150, 260), (75, 130)]
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and np.array_equal(bits(g.get()), bits(w.astype(np.float32)))
    assert dbm.build_overviews(dev, 0) == []
    with pytest.raises(ValueError, match="build_overviews: levels 11: an image of 300 x 520 admits 10 levels"):
        dbm.build_overviews(dev, 11)


def same_bytes(got, want):
    a, b = open(got, "rb").read(), open(want, "rb").read()
    if a != b:
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError(f"{got}: {len(a)} bytes, {want}: {len(b)} bytes, first difference at byte {first}")


@pytest.mark.parametrize("bigtiff", [True, False])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_the_file_equals_the_host_writers(dbm, tmp_path, pyramids, dtype, predictor, tiled, bigtiff):
    a, want = pyramids[(300, 520), dtype]
    dev = dbm.to_device(a[None])
    kw = dict(dtype=dtype, predictor=predictor, tiled=tiled, bigtiff=bigtiff, compression="lzw", nodataval=NODATA, overviews=4)
    got = dbm.write_geotiff_resident(str(tmp_path / "dev"), BOUND, dev, **kw)
    same_bytes(got, dbm.save_array_to_grid(str(tmp_path / "host"), BOUND, dev.get(), **kw))
    assert dbm.open_geotiff(got).overview_count == 4
    back, info = dbm.read_geotiff(got, overview=4)
    assert np.array_equal(bits(back[0]), bits(want[3]))


def test_batches_and_defaults(dbm, tmp_path, pyramids, monkeypatch):
    a, _ = pyramids[(300, 520), "int16"]
    dev = dbm.to_device(a)
    kw = dict(dtype=np.int16, nodataval=NODATA)
    whole = dbm.write_geotiff_resident(str(tmp_path / "whole"), BOUND, dev, overviews="auto", **kw)
    same_bytes(whole, dbm.save_array_to_grid(str(tmp_path / "host"), BOUND, dev.get()[None], tiled=True, compression="lzw", overviews="auto", **kw))
    calls = []
    real = dev.ctx.call
    monkeypatch.setattr(dev.ctx, "call", lambda name, *args: (calls.append((name, args)), real(name, *args))[1], raising=False)
    # level 0: 6 tiles of 131072 raw bytes + a slot of 196672 each, two per batch; level 1 (150 x 260): 2 tiles, level 2: 1 tile
    parts = dbm.write_geotiff_resident(str(tmp_path / "parts"), BOUND, dev, overviews="auto", workspace_limit=700_000, **kw)
    monkeypatch.undo()
    assert calls[0][0] == "dbm_grid_overviews" and [c[0] for c in calls].count("dbm_grid_overviews") == 1
    assert [(n, a[1], a[2], a[9], a[10]) for n, a in calls if n == "dbm_tiff_encode"] == [("dbm_tiff_encode", 300, 520, 0, 2), ("dbm_tiff_encode", 300, 520, 2, 2),
                                                               ("dbm_tiff_encode", 300, 520, 4, 2), ("dbm_tiff_encode", 150, 260, 0, 2),
                                                               ("dbm_tiff_encode", 75, 130, 0, 1)]
    same_bytes(parts, whole)
    # several batches inside every level: one block per call
    one = dbm.write_geotiff_resident(str(tmp_path / "one"), BOUND, dev, overviews="auto", workspace_limit=1, **kw)
    same_bytes(one, whole)
    # overviews=0 is the file written without the argument
    same_bytes(dbm.write_geotiff_resident(str(tmp_path / "zero"), BOUND, dev, overviews=0, **kw),
               dbm.write_geotiff_resident(str(tmp_path / "none"), BOUND, dev, **kw))
    for bad in (-1, 11, "all", 1.5):
        with pytest.raises(ValueError, match="write_geotiff_resident: overviews .* admits 10 levels"):
            dbm.write_geotiff_resident(str(tmp_path / "bad"), BOUND, dev, overviews=bad, **kw)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_the_readers_on_an_overview(dbm, tmp_path, pyramids, dtype):
    a, want = pyramids[(300, 520), dtype]
    path = dbm.write_geotiff_resident(str(tmp_path / "r"), BOUND, dbm.to_device(a), dtype=dtype, predictor=2, nodataval=NODATA, overviews=3)
    minx, _, _, maxy = BOUND
    for k in (1, 2, 3):
        back, info = dbm.read_geotiff_resident(path, overview=k)
        assert back.shape == want[k - 1].shape and info["dtype"] == np.dtype(dtype) and info["nodata"] == str(NODATA)
        assert np.array_equal(bits(back.get()), bits(want[k - 1].astype(np.float32)))
        assert info["geometry"] == dbm.open_geotiff(path, k).geometry
    # a window on level 1 (pixels of 200 m): rows 5..14, columns 100..259, across both tiles of that level (260 wide)
    bound = (minx + 20000, maxy - 3000, minx + 54000, maxy - 1000)
    back, info = dbm.read_geotiff_resident(path, window_bound=bound, overview=1)
    assert info["window"] == (5, 100, 10, 160)
    assert np.array_equal(bits(back.get()), bits(want[0][5:15, 100:260].astype(np.float32)))
    raster = dbm.Raster.open(path, overview=1)
    assert raster.shape == (150, 260) and raster.nodata == float(NODATA) and raster.geometry == dbm.GridGeometry.from_bounds(BOUND, 150, 260)
    assert np.array_equal(bits(raster.device().get()), bits(want[0].astype(np.float32)))
    part = dbm.Raster.open(path, window_bound=bound, overview=1)
    assert part.shape == (10, 160) and np.array_equal(bits(part.device().get()), bits(want[0][5:15, 100:260].astype(np.float32)))
    assert part.geometry.x0 == 100 * 200.0 + raster.geometry.x0 and part.geometry.dx == 200.0
    with pytest.raises(ValueError, match="overview 4 asked for, the file holds 3"):
        dbm.read_geotiff_resident(path, overview=4)
    with pytest.raises(ValueError, match="overview 4 asked for, the file holds 3"):
        dbm.Raster.open(path, overview=4)


def test_refusals_of_the_entry_point(dbm):
    """Status 1 before any device work."""
    from deepbedmap_amd import _lib

    dev = dbm.to_device(np.zeros((300, 520), dtype=np.float32))
    out = dbm.DeviceArray((70000,))
    call_overviews(dev.ctx, dev, 300, 520, 1, -2000.0, 10, out)
    call_overviews(dev.ctx, dev, 300, 520, 4, -2000.0, 0, None)   # nothing to write
    for args, message in (((dev, 300, 520, 1, -2000.0, -1, out), r"levels must lie in 0\.\.10 for a plane of 300 x 520"),
                          ((dev, 300, 520, 1, -2000.0, 11, out), r"levels must lie in 0\.\.10 for a plane of 300 x 520"),
                          ((dev, 1, 1, 4, -2000.0, 1, out), r"levels must lie in 0\.\.0 for a plane of 1 x 1"),
                          ((dev, 300, 520, 2, -2000.0, 1, out), "sample_type must be 1"),
                          ((None, 300, 520, 1, -2000.0, 1, out), "NULL plane"),
                          ((dev, 300, 520, 1, None, 1, out), "NULL nodata"),
                          ((dev, 300, 520, 1, float("nan"), 1, out), "nodata value of an int16 file must be finite"),
                          ((dev, 300, 520, 1, -2000.0, 1, None), "NULL output"),
                          ((dev, 300, 520, 1, -2000.0, 1, dev), "the output must not be the input"),
                          ((dev, 0, 520, 1, -2000.0, 1, out), "empty plane"),
                          ((dev, 1 << 20, 1 << 20, 1, -2000.0, 1, out), "H W must stay below 2\\^31 samples")):
        with pytest.raises(_lib.DbmError, match=message) as e:
            call_overviews(dev.ctx, *args)
        assert e.value.code == 1, args
