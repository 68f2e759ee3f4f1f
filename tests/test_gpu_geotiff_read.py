"""-m gpu: `read_geotiff_resident` / `Raster.open` (dbm_tiff_decode: LZW by one wavefront per block, predictors, conversion, placement;
DESIGN.md 6i) against independent decodes of the same files: Pillow / libtiff for the files Pillow writes, `read_geotiff` (the host
path) for the files of the package's own writer.  Decoding is exact: every comparison is on bits (NaNs count), no tolerance anywhere.
The semantics of the predictors are pinned on the CPU in tests/test_geotiff_open_host.py.

Shapes: 70 x 300 in strips of 16 rows (a short last strip; Gaussian noise fills the 4096-entry table within a strip, so the table
reset and all four code widths occur -- asserted through the stream length), 256 x 256 (one whole tile) and 300 x 520 (2 x 3 tiles,
padded at the right and bottom edges)."""
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_geotiff_open_host as host  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = host.BOUND
bits = host.bits


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(scope="module")
def plane():
    a = np.random.default_rng(5).normal(0.0, 300.0, (300, 520)).astype(np.float32)
    a[40:90, 100:300] = -9999.0
    a[7, 3] = np.nan
    return a


def f32_bits(a):
    with np.errstate(all="ignore"):
        return bits(np.asarray(a).astype(np.float32))


def read_bits(dbm, path, **kw):
    dev, info = dbm.read_geotiff_resident(path, **kw)
    return bits(dev.get()), info


@pytest.mark.parametrize("dtype,predictor", host.CASES)
def test_lzw_strips_from_libtiff(dbm, tmp_path, dtype, predictor):
    a = np.random.default_rng(11).normal(0.0, 300.0, (70, 300)).astype(dtype)
    if dtype == "float32":
        a[3, 5:9] = np.nan
    path = host.pillow_save(tmp_path / "p.tif", a, {317: predictor, 278: 16}, compression="tiff_lzw")
    plan = dbm.open_geotiff(path).plan()
    assert plan.blocks[:, 2].tolist() == [16, 16, 16, 16, 6]
    assert (plan.blocks[:4, 1] > 5 * 1024).all(), plan.blocks[:, 1]   # long enough for > 3837 table entries: reset and 12-bit codes
    got, info = read_bits(dbm, path)
    assert info["predictor"] == predictor and info["dtype"] == np.dtype(dtype) and info["window"] == (0, 0, 70, 300)
    assert np.array_equal(got, f32_bits(host.pillow_decode(path, dtype)))


@pytest.mark.parametrize("bigtiff", [False, True])
@pytest.mark.parametrize("shape", [(256, 256), (300, 520)])
def test_lzw_tiles_of_the_package_writer(dbm, tmp_path, plane, shape, bigtiff):
    a = plane[:shape[0], :shape[1]]
    path = dbm.save_array_to_grid(str(tmp_path / "t"), BOUND, a[None], tiled=True, compression="lzw", bigtiff=bigtiff, nodataval=-9999)
    ref, ref_info = dbm.read_geotiff(path)
    got, info = read_bits(dbm, path)
    assert np.array_equal(got, bits(ref[0])) and np.array_equal(got, bits(a))
    for key, value in ref_info.items():
        assert info[key] == value, key
    assert info["geometry"] == dbm.GridGeometry.from_bounds(BOUND, *shape)


@pytest.mark.parametrize("kind", ["constant", "half"])
def test_long_strings_and_kwkwk(dbm, tmp_path, kind):
    """A constant int16 tile: every code but the first is `next` (KwKwK) and the strings grow to several hundred bytes, so copies take
    more than one 64-lane pass; half constant, half noise: both regimes in one stream."""
    a = np.full((256, 256), -2000, dtype=np.int16)
    if kind == "half":
        a[128:] = np.random.default_rng(3).normal(0.0, 300.0, (128, 256)).astype(np.int16)
    path = dbm.save_array_to_grid(str(tmp_path / "c"), BOUND, a[None], tiled=True, compression="lzw", dtype=np.int16)
    if kind == "constant":
        assert dbm.open_geotiff(path).plan().blocks[0, 1] < 1024   # 131072 bytes in < 1 KiB: strings of hundreds of bytes
    got, info = read_bits(dbm, path)
    assert info["nodata"] == "-2000" and np.array_equal(got, f32_bits(a))


@pytest.mark.parametrize("dtype,predictor,compression", [("int16", 2, "tiff_adobe_deflate"), ("float32", 2, "tiff_adobe_deflate"),
                                                         ("float32", 3, "tiff_adobe_deflate"), ("int16", 2, None), ("float32", 2, None)])
def test_deflate_and_uncompressed(dbm, tmp_path, dtype, predictor, compression):
    """Stage (b) alone.  On an uncompressed file libtiff leaves the Predictor tag without effect; so does this reader."""
    a = np.random.default_rng(12).normal(0.0, 300.0, (70, 300)).astype(dtype)
    kw = {"compression": compression} if compression else {}
    path = host.pillow_save(tmp_path / "d.tif", a, {317: predictor, 278: 16}, **kw)
    got, info = read_bits(dbm, path)
    assert info["compression"] == (8 if compression else 1) and info["predictor"] == (predictor if compression else 1)
    assert np.array_equal(got, f32_bits(host.pillow_decode(path, dtype)))


def test_other_sample_types(dbm, tmp_path):
    r = np.random.default_rng(13)
    u8 = r.integers(0, 256, (70, 300)).astype(np.uint8)
    u16 = r.integers(0, 65536, (70, 300)).astype(np.uint16)
    i32 = r.integers(-2**31, 2**31, (70, 300)).astype(np.int32)     # (beyond 2^24: the conversion rounds to nearest even)
    for name, a, info in (("u8", u8, {278: 16}), ("u16", u16, {317: 2, 278: 16}), ("i32", i32, {317: 2, 278: 16})):
        path = host.pillow_save(tmp_path / (name + ".tif"), a, info, compression="tiff_lzw")
        got, meta = read_bits(dbm, path)
        assert meta["dtype"] == a.dtype
        assert np.array_equal(got, f32_bits(host.pillow_decode(path, a.dtype))) and np.array_equal(got, f32_bits(a))
    f64 = r.normal(0.0, 300.0, (70, 300))
    f64[0, :6] = [np.nan, np.inf, -np.inf, 1e300, -1e-300, 1e-40]   # NaN, overflow to inf, underflow to -0, a float32 subnormal
    f64[1, 0] = 1.0 + 2.0**-24                                        # a tie: to even
    for comp in ("lzw", "none"):
        path = dbm.save_array_to_grid(str(tmp_path / ("f64" + comp)), BOUND, f64[None], tiled=True, compression=comp, dtype=np.float64)
        ref, _ = dbm.read_geotiff(path)
        assert ref.dtype == np.float64
        got, meta = read_bits(dbm, path)
        assert meta["dtype"] == np.float64 and np.array_equal(got, f32_bits(ref[0]))


def test_windowed_reads(dbm, tmp_path, plane):
    path = dbm.save_array_to_grid(str(tmp_path / "w"), BOUND, plane[None], tiled=True, compression="lzw", bigtiff=False, nodataval=-9999)
    full, _ = read_bits(dbm, path)
    assert np.array_equal(full, bits(plane))
    minx, miny, maxx, maxy = BOUND
    whole = dbm.Raster.open(path)
    assert whole.shape == (300, 520) and whole.nodata == -9999.0 and whole.geometry == dbm.GridGeometry.from_bounds(BOUND, 300, 520)
    for wb, (r0, c0, h, w) in (((minx + 30000, maxy - 2000, minx + 31000, maxy - 1000), (10, 300, 10, 10)),       # inside tile 1
                               ((minx + 25000, maxy - 30000, minx + 27000, maxy - 25000), (250, 250, 50, 20)),    # across four tiles
                               ((minx + 25050, maxy - 27030, minx + 26949, maxy - 24999), (250, 250, 20, 19)),    # unaligned bounds
                               ((maxx - 1000, miny - 5000, maxx + 5000, miny + 1000), (290, 510, 10, 10))):       # over the image edge
        got, info = read_bits(dbm, path, window_bound=wb)
        assert info["window"] == (r0, c0, h, w)
        assert np.array_equal(got, full[r0:r0 + h, c0:c0 + w])
        r = dbm.Raster.open(path, window_bound=wb)
        g = whole.geometry
        assert r.shape == (h, w) and r.nodata == -9999.0
        assert r.geometry == dbm.GridGeometry(x0=g.x0 + c0 * g.dx, y0=g.y0 + r0 * g.dy, dx=g.dx, dy=g.dy, registration="pixel")
        assert np.array_equal(bits(r.device().get()), full[r0:r0 + h, c0:c0 + w])


def test_batches_under_a_workspace_limit(dbm, tmp_path, plane):
    from deepbedmap_amd import geotiff

    path = dbm.save_array_to_grid(str(tmp_path / "b"), BOUND, plane[None], tiled=True, compression="lzw")
    gf = dbm.open_geotiff(path)
    assert len(geotiff._batches(gf, gf.plan(), 300000)) == 6 and len(geotiff._batches(gf, gf.plan(), 1 << 30)) == 1
    one, _ = read_bits(dbm, path)
    for limit in (300000, 1, 900000):
        many, _ = read_bits(dbm, path, workspace_limit=limit)
        assert np.array_equal(many, one)
    assert np.array_equal(one, bits(plane))
    # strips, uncompressed: the other staging layout
    path = dbm.save_array_to_grid(str(tmp_path / "s"), BOUND, plane[None], tiled=False, compression="none")
    gf = dbm.open_geotiff(path)
    assert len(geotiff._batches(gf, gf.plan(), 1)) == 2
    assert np.array_equal(read_bits(dbm, path, workspace_limit=1)[0], bits(plane))


def _set_byte_count(buf, index, value):
    """TileByteCounts[index] of a classic little-endian TIFF."""
    ifd = struct.unpack_from("<I", buf, 4)[0]
    for k in range(struct.unpack_from("<H", buf, ifd)[0]):
        tag, typ, count = struct.unpack_from("<HHI", buf, ifd + 2 + 12 * k)
        if tag == 325:
            assert typ == 4 and count > 1
            struct.pack_into("<I", buf, struct.unpack_from("<I", buf, ifd + 2 + 12 * k + 8)[0] + 4 * index, value)
            return
    raise AssertionError("no TileByteCounts")


def test_malformed_streams_are_reported_by_block(dbm, tmp_path, plane):
    """The decoder's bounds hold by construction (every stream read and output write is checked against the block's byte count and
    size; established on the CPU by tools/lzw_twin_check.cpp): a cut stream and a stream with a code beyond the table end in a
    DbmError that names the block, and the host decoder rejects the same bytes."""
    from deepbedmap_amd import geotiff

    path = dbm.save_array_to_grid(str(tmp_path / "e"), BOUND, plane[None], tiled=True, compression="lzw", bigtiff=False)
    gf = dbm.open_geotiff(path)
    off, cnt = int(gf.offsets[2]), int(gf.counts[2])
    good = open(path, "rb").read()
    cut = bytearray(good)
    _set_byte_count(cut, 2, cnt // 2)
    wild = bytearray(good)
    wild[off + 1] |= 0x7F   # the second 9-bit code becomes 511, all ones (4095 in a 12-bit field): beyond the table
    wild[off + 2] |= 0xC0
    for name, data, stream in (("cut", cut, good[off:off + cnt // 2]), ("wild", wild, bytes(wild[off:off + cnt]))):
        bad = tmp_path / (name + ".tif")
        bad.write_bytes(bytes(data))
        with pytest.raises(dbm.DbmError):
            geotiff.lzw_decode(stream, 256 * 256 * 4)
        with pytest.raises(dbm.DbmError, match=r"block 2\b") as e:
            dbm.read_geotiff_resident(str(bad))
        assert e.value.code == 11
        # the other blocks of the same file are good: a window that does not touch block 2
        got, _ = read_bits(dbm, str(bad), window_bound=(BOUND[0], BOUND[3] - 25600, BOUND[0] + 51200, BOUND[3]))
        assert np.array_equal(got, bits(plane[:256, :512]))
    assert np.array_equal(read_bits(dbm, path)[0], bits(plane))


def test_an_opened_raster_feeds_selective_tile(dbm, tmp_path, plane):
    import warnings

    path = dbm.save_array_to_grid(str(tmp_path / "r"), BOUND, plane[None], tiled=True, compression="lzw", nodataval=-9999)
    opened = dbm.Raster.open(path)
    built = dbm.Raster(plane, dbm.GridGeometry.from_bounds(BOUND, 300, 520), nodata=-9999.0)
    minx, _, _, maxy = BOUND
    windows = [(minx + 1000 + 700 * k, maxy - 9000 - 500 * k, minx + 4600 + 700 * k, maxy - 5400 - 500 * k) for k in range(5)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in ({"interpolate": False}, {"padding": 1000, "resolution": 250.0, "gapfiller": -5000.0}):
            a = dbm.selective_tile(opened, windows, **kw).get()
            b = dbm.selective_tile(built, windows, **kw).get()
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    assert dbm.get_window_bounds(opened, 36, 36, 12) == dbm.get_window_bounds(built, 36, 36, 12)
