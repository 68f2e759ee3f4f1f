"""-m gpu: colour relief and hillshade of a resident plane (dbm_grid_relief, dbm_grid_shade_stats; relief.hip) and the PNG written from
a resident image (dbm_png_encode: filters, one wavefront per band, framing 1 / 2; png_encode.hip, deflate_encode.hip), DESIGN.md 6n,
against the restatements of tests/relief_restatement.py, the host writer and independent decoders.

Relief.  Unshaded bytes equal the restatement with no tolerance: division, product and sum are IEEE operations on both sides.  Shaded
bytes are compared with the restatement fed the device's own (mean, sigma): only atan may differ in its last bits, so a byte is left
out if its pre-rounding value in the restatement lies within 1e-9 of some k + 0.5; at most 0.1 % of an image may be left out (the host
test shows it is none for these inputs) and every other byte is equal.  Planes: (1, 1); (1, 7) and (7, 1) where g is undefined; (37,
29); (150, 210): ten tiles down and four across at the kernel's 16 x 64 tile, so halos cross tiles both ways.
PNG.  The device's file equals `save_png`'s file from the downloaded image byte for byte; `read_png` and PIL return the image."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pyramid_restatement as pr  # noqa: E402
import relief_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

TABLES = ["oleron", "hinge", "bands", "one", "wide"]


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(scope="module")
def tables(dbm):
    from deepbedmap_amd import relief

    oleron = relief.read_cpt(rr.GOLDEN_CPT)
    we, wc = rr.wide_master()
    wide = relief.ColorTable(we, np.concatenate([np.array(wc, dtype=np.uint8).ravel(), np.array([1, 2, 3, 250, 251, 252, 9, 8, 7], dtype=np.uint8)]))
    return {"oleron": relief.make_cpt(oleron, (-4500, 4500)), "hinge": relief.make_cpt(oleron, (-2000, 4500), hinge=0),
            "bands": relief.make_cpt(oleron, (-2800, 2800, 200), overrule_bg=True), "one": relief.make_cpt(relief.grey_cpt(), (-4500, 4500)),
            "wide": relief.make_cpt(wide, (-4500, 4500))}


@pytest.fixture(scope="module")
def planes(dbm):
    cache = {}

    def get(name, shape):
        if (name, shape) not in cache:
            cache[name, shape] = dbm.to_device(rr.plane_of(name, shape))
        return cache[name, shape]

    return get


def compare_shaded(got, want, pre):
    """Every byte equal but those within 1e-9 of a rounding tie in the restatement; at most 0.1 % of them."""
    skip = rr.near_tie(pre)
    share = skip.mean()
    print(f"near-tie share {share:.6f}, differing bytes {(got[:, :, :3] != want[:, :, :3]).sum()}")
    assert share <= 1e-3
    assert np.array_equal(np.where(skip, 0, got[:, :, :3]), np.where(skip, 0, want[:, :, :3]))
    if got.shape[2] == 4:
        assert np.array_equal(got[:, :, 3], want[:, :, 3])


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("shape", rr.SHAPES)
@pytest.mark.parametrize("name", TABLES)
def test_unshaded_relief_equals_the_restatement(dbm, tables, planes, name, shape, channels):
    got = dbm.relief_image(planes(name, shape), tables[name], channels=channels)
    assert got.shape == shape + (channels,) and got.dtype == np.uint8
    want, _ = rr.reference(name, shape)
    assert np.array_equal(got.get(), want[:, :, :channels])


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("shape", rr.SHAPES)
@pytest.mark.parametrize("name", TABLES)
def test_shaded_relief_equals_the_restatement_fed_the_device_statistics(dbm, tables, planes, name, shape, channels):
    from deepbedmap_amd import relief

    sin_a, cos_a, k = rr.shading_constants()
    n, mean, sigma = relief.shade_stats(planes(name, shape), sin_a, cos_a, 1.0)
    got = dbm.relief_image(planes(name, shape), tables[name], shading="+d", channels=channels).get()
    if min(shape) == 1:   # g is undefined everywhere: I = 0
        assert (n, mean, sigma) == (0, 0.0, 0.0)
        assert np.array_equal(got, rr.reference(name, shape)[0][:, :, :channels])
        return
    want, pre = rr.reference(name, shape, (mean, sigma))
    compare_shaded(got, want[:, :, :channels], pre)
    # the same through (azimuth, amplitude) and given statistics
    again = dbm.relief_image(planes(name, shape), tables[name], shading=rr.SHADING, channels=channels, stats=(n, mean, sigma)).get()
    assert np.array_equal(again, got)


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_shade_stats_against_numpy(dbm, planes, shape):
    from deepbedmap_amd import relief

    sin_a, cos_a, _ = rr.shading_constants()
    g, ok = rr.gradient_of("oleron", shape)
    n, mean, sigma = rr.stats(g, ok)
    first = relief.shade_stats(planes("oleron", shape), sin_a, cos_a, 1.0)
    second = relief.shade_stats(planes("oleron", shape), sin_a, cos_a, 1.0)
    assert np.array(first).tobytes() == np.array(second).tobytes()   # identical bits
    print(shape, first, (n, mean, sigma))
    assert first[0] == n
    if n == 0:
        assert first == (0, 0.0, 0.0)
        return
    values = g[ok]
    assert abs(first[1] - float(np.sum(values) / n)) <= n * 2.0 ** -52 * np.abs(values).mean()
    assert abs(first[1] - mean) <= n * 2.0 ** -52 * np.abs(values).mean()
    numpy_sigma = float(np.sqrt(np.sum((values - np.sum(values) / n) ** 2) / (n - 1)))
    assert abs(first[2] - numpy_sigma) <= 2 * n * 2.0 ** -52 * numpy_sigma
    assert abs(first[2] - sigma) <= 2 * n * 2.0 ** -52 * sigma


def test_other_azimuth_amplitude_and_aspect(dbm, tables, planes):
    """The arguments reach the kernel: azimuth 200 degrees, amplitude 0.4, aspect 1.7 on the 37 x 29 plane."""
    import math

    from deepbedmap_amd import relief

    z, t = rr.plane_of("oleron", (37, 29)), rr.tables()["oleron"]
    a = math.radians(200.0)
    sin_a, cos_a, k = math.sin(a), math.cos(a), 0.4 * (2.0 / math.pi)
    n, mean, sigma = relief.shade_stats(planes("oleron", (37, 29)), sin_a, cos_a, 1.7)
    g, ok = rr.gradient(z, sin_a, cos_a, 1.7)
    assert n == ok.sum()
    want, pre = rr.relief(z, t[0], t[1], t[2], t[3], t[4], 4, (k, mean, sigma), g, ok)
    got = dbm.relief_image(planes("oleron", (37, 29)), tables["oleron"], shading=(200.0, 0.4), aspect=1.7).get()
    compare_shaded(got, want, pre)


def test_relief_takes_rasters_and_host_arrays(dbm, tables):
    z = rr.plane_of("oleron", (37, 29))
    want = rr.reference("oleron", (37, 29))[0]
    raster = dbm.Raster(z, dbm.GridGeometry(0.0, 0.0, 1.0, -1.0))
    assert np.array_equal(dbm.relief_image(raster, tables["oleron"]).get(), want)
    assert np.array_equal(dbm.relief_image(z[None], tables["oleron"]).get(), want)


def test_relief_refusals_return_status_1_with_a_message(dbm, tables, planes):
    from deepbedmap_amd import _lib

    ctx = dbm.default_context()
    lib = _lib.lib()
    plane = planes("oleron", (37, 29))
    out = dbm.DeviceArray((37, 29, 4), ctx, dtype=np.uint8)
    t = tables["oleron"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(plane_ptr=plane.ptr, H=37, W=29, edges=t.edges, colors=t.colors, n=t.n, channels=4, shade=0, sin_a=0.0, cos_a=1.0, aspect=1.0,
             mean=0.0, sigma=1.0, k=0.5, out_ptr=out.ptr):
        return lib.dbm_grid_relief(ctx.handle, C.c_void_p(plane_ptr), H, W, None if edges is None else p(edges), None if colors is None else p(colors),
                                   n, channels, shade, sin_a, cos_a, aspect, mean, sigma, k, C.c_void_p(out_ptr))

    assert call() == 0
    bad = t.edges.copy()
    bad[5] = bad[4]
    nan = t.edges.copy()
    nan[7] = np.nan
    for kw in (dict(plane_ptr=None), dict(out_ptr=None), dict(edges=None), dict(colors=None), dict(H=0), dict(H=1 << 16, W=1 << 15), dict(channels=2),
               dict(channels=5), dict(n=0), dict(n=2049), dict(edges=bad), dict(edges=nan), dict(shade=1, sigma=0.0), dict(shade=1, sigma=-1.0),
               dict(shade=1, mean=np.nan), dict(shade=1, sigma=np.inf), dict(shade=1, k=np.nan), dict(shade=1, k=0.64), dict(shade=1, k=-0.64)):
        assert call(**kw) == 1, kw
        assert b"dbm_grid_relief" in lib.dbm_last_error(ctx.handle), kw
    assert call(shade=1, k=2.0 / np.pi) == 0
    assert lib.dbm_grid_relief(None, C.c_void_p(plane.ptr), 37, 29, p(t.edges), p(t.colors), t.n, 4, 0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.5, C.c_void_p(out.ptr)) == 1
    stats = np.zeros(3)
    assert lib.dbm_grid_shade_stats(ctx.handle, None, 37, 29, 0.0, 1.0, 1.0, p(stats)) == 1
    assert lib.dbm_grid_shade_stats(ctx.handle, C.c_void_p(plane.ptr), 37, 29, 0.0, 1.0, 1.0, None) == 1
    assert lib.dbm_grid_shade_stats(ctx.handle, C.c_void_p(plane.ptr), 0, 29, 0.0, 1.0, 1.0, p(stats)) == 1
    assert lib.dbm_grid_shade_stats(ctx.handle, C.c_void_p(plane.ptr), 37, 29, np.nan, 1.0, 1.0, p(stats)) == 1
    assert b"dbm_grid_shade_stats" in lib.dbm_last_error(ctx.handle)
    ctx.synchronize()


# ---- PNG ----
def png_images():
    rng = np.random.default_rng(11)

    def kinds(shape):
        H, W, ch = shape
        if ch == 4 and H >= 37:
            z = rr.sample_plane(H, W)
            t = rr.tables()["oleron"]
            rendered = rr.relief(z, t[0], t[1], t[2], t[3], t[4], 4)[0] if (H, W) != (37, 29) else rr.reference("oleron", (37, 29))[0]
        else:   # a smooth picture of the shape's own
            rendered = ((np.add.outer(np.arange(H) * 3, np.arange(W) * 5)[:, :, None] + np.arange(ch) * 40) % 251).astype(np.uint8)
        return {"relief": rendered, "constant": np.full(shape, 200, dtype=np.uint8), "noise": rng.integers(0, 256, shape, dtype=np.uint8)}

    return kinds


PNG_CASES = [((1, 1, 4), None), ((3, 5, 3), None), ((37, 29, 4), 5), ((37, 29, 4), 1), ((37, 29, 4), 64), ((96, 200, 4), 96), ((40, 33, 1), None)]


@pytest.fixture(scope="module")
def png_sources():
    kinds, cache = png_images(), {}

    def get(shape):
        if shape not in cache:
            cache[shape] = kinds(shape)
        return cache[shape]

    return get


@pytest.mark.parametrize("filter", [0, 1, 2])
@pytest.mark.parametrize("content", ["relief", "constant", "noise"])
@pytest.mark.parametrize("shape,band_rows", PNG_CASES)
def test_the_png_equals_the_host_writers(dbm, tmp_path, png_sources, shape, band_rows, content, filter):
    image = png_sources(shape)[content]
    dev = dbm.DeviceArray(shape, dtype=np.uint8).set(image)
    got = dbm.write_png_resident(str(tmp_path / "dev.png"), dev, filter=filter, band_rows=band_rows, idat_bytes=4096)
    want = dbm.save_png(str(tmp_path / "host.png"), dev.get(), filter=filter, band_rows=band_rows, idat_bytes=4096)
    a, b = open(got, "rb").read(), open(want, "rb").read()
    assert len(a) == len(b) and a == b
    assert np.array_equal(dbm.read_png(got).reshape(shape), image)
    if shape == (96, 200, 4):
        assert 96 * (200 * 4 + 1) == 76896   # one band beyond the 32 KiB window
    if content == "noise" and shape[0] * shape[1] > 100:
        assert len(a) > image.size           # the stream outgrows the raw bytes
    # several batches give the same file
    small = dbm.write_png_resident(str(tmp_path / "small.png"), dev, filter=filter, band_rows=band_rows, idat_bytes=4096, workspace_limit=1)
    assert open(small, "rb").read() == a
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(got) as im:
        assert np.array_equal(np.asarray(im).reshape(shape), image)


def test_a_short_last_batch_of_bands_writes_the_host_writers_png(dbm, tmp_path, png_sources, monkeypatch):
    """37 rows in bands of 8: five bands, the last of 5 rows; four bands per call, so the last call takes one."""
    shape = (37, 29, 4)
    image = png_sources(shape)["relief"]
    dev = dbm.DeviceArray(shape, dtype=np.uint8).set(image)
    band = 8 * (29 * 4 + 1)
    calls = []
    real = dev.ctx.call
    monkeypatch.setattr(dev.ctx, "call", lambda name, *args: (calls.append((name,) + args[6:8]), real(name, *args))[1], raising=False)
    got = dbm.write_png_resident(str(tmp_path / "dev.png"), dev, band_rows=8, idat_bytes=4096, workspace_limit=4 * (band + band + band // 8 + 16))
    monkeypatch.undo()
    assert [c for c in calls if c[0] == "dbm_png_encode"] == [("dbm_png_encode", 0, 4), ("dbm_png_encode", 4, 1)]
    want = dbm.save_png(str(tmp_path / "host.png"), dev.get(), band_rows=8, idat_bytes=4096)
    assert open(got, "rb").read() == open(want, "rb").read()


def test_png_refusals_and_the_world_file(dbm, tmp_path):
    from deepbedmap_amd import _lib

    ctx = dbm.default_context()
    lib = _lib.lib()
    image = dbm.DeviceArray((4, 4, 4), ctx, dtype=np.uint8).set(np.arange(64, dtype=np.uint8))
    out, sizes, adlers = np.zeros(4096, dtype=np.uint8), np.zeros(4, dtype=np.uintp), np.zeros(4, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(ptr=image.ptr, H=4, W=4, ch=4, filter=1, rows=2, first=0, n=2, cap=4096, handle=ctx.handle):
        return lib.dbm_png_encode(handle, C.c_void_p(ptr), H, W, ch, filter, rows, first, n, p(out), cap, p(sizes), p(adlers))

    assert call() == 0
    for kw in (dict(ptr=None), dict(H=0), dict(ch=2), dict(filter=3), dict(rows=0), dict(first=1, n=2), dict(n=-1), dict(cap=10), dict(handle=None)):
        assert call(**kw) == 1, kw
    assert b"dbm_png_encode" in lib.dbm_last_error(ctx.handle)
    assert call(n=0) == 0
    with pytest.raises(ValueError, match="DeviceArray"):
        dbm.write_png_resident(str(tmp_path / "x.png"), np.zeros((2, 2), dtype=np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        dbm.write_png_resident(str(tmp_path / "x.png"), dbm.DeviceArray((2, 2), ctx))
    geometry = dbm.GridGeometry(x0=100.5, y0=-20.25, dx=0.5, dy=-0.5, registration="pixel")
    path = dbm.write_png_resident(str(tmp_path / "w.png"), image, world_file=geometry)
    assert [float(v) for v in open(str(tmp_path / "w.pgw")).read().split()] == [0.5, 0.0, 0.0, -0.5, 100.5, -20.25]
    assert np.array_equal(dbm.read_png(path), image.get())


def test_render_dem_reduced_with_nodata(dbm, tables, tmp_path):
    """render_dem on a resident 150 x 210 Raster, reduce=2, nodata -9999: nodata -> NaN, two nodata-aware halvings (pyramid_restatement),
    the relief of the 38 x 53 level, the PNG, the world file."""
    from deepbedmap_amd import relief

    z = rr.plane_of("oleron", (150, 210)).copy()
    z[~np.isfinite(z)] = 100.0            # (the 2 x 2 means of the restatement run on finite samples and nodata)
    z[40:60, 100:140] = -9999.0           # whole windows of nodata two levels down
    z[::7, ::5] = -9999.0                 # and isolated ones
    geometry = dbm.GridGeometry(x0=1000.0, y0=5000.0, dx=250.0, dy=-250.0, registration="pixel")
    raster = dbm.Raster(dbm.to_device(z), geometry, nodata=-9999.0)
    path, image_geometry = dbm.render_dem(raster, str(tmp_path / "dem.png"), tables["oleron"], shading="+d", reduce=2)
    levels, _ = pr.pyramid(np.where(z == np.float32(-9999.0), np.float32(np.nan), z), 2, np.nan)
    level = levels[-1]
    assert level.shape == (38, 53) and np.isnan(level).any()
    sin_a, cos_a, k = rr.shading_constants()
    n, mean, sigma = relief.shade_stats(dbm.to_device(level), sin_a, cos_a, 1.0)
    g, ok = rr.gradient(level, sin_a, cos_a, 1.0)
    t = rr.tables()["oleron"]
    want, pre = rr.relief(level, t[0], t[1], t[2], t[3], t[4], 4, (k, mean, sigma), g, ok)
    got = dbm.read_png(path)
    compare_shaded(got, want, pre)
    assert (got[:, :, 3] == 0).sum() == np.isnan(level).sum() > 0
    assert image_geometry == relief.reduced_geometry(geometry, 2)
    assert [float(v) for v in open(str(tmp_path / "dem.pgw")).read().split()] == [1000.0, 0.0, 0.0, -1000.0, 1375.0, 4625.0]
    # "auto": the smallest level that fits max_size
    path, g2 = dbm.render_dem(raster, str(tmp_path / "auto.png"), tables["oleron"], reduce="auto", max_size=60, world_file=False)
    assert dbm.read_png(path).shape == (38, 53, 4) and not os.path.exists(str(tmp_path / "auto.pgw"))
    with pytest.raises(ValueError, match="reduce"):
        dbm.render_dem(raster, str(tmp_path / "x.png"), tables["oleron"], reduce=-1)
