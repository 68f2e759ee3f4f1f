"""-m gpu: deflate GeoTIFFs inflated on the device (`read_geotiff_resident(..., inflate="device")`: dbm_tiff_decode with compression 8,
one wavefront per block; tiff_inflate.hip) against independent decodes: Pillow / libtiff for the files Pillow writes,
the source plane and the host path (`inflate="host"`: zlib) for tiled files, `zlib.decompress` for raw streams.  Decoding is exact:
every comparison is on bits.  The streams are those of tests/test_inflate_host.py, where what each of them exercises is asserted.

Shapes: 70 x 300 in strips of 16 rows (a short last strip), 300 x 520 (2 x 3 tiles of 256, padded right and bottom), and one block
per raw stream, 256 columns wide."""
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inflate_restatement as rs  # noqa: E402
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
    dev, info = dbm.read_geotiff_resident(path, inflate="device", **kw)
    return bits(dev.get()), info


@pytest.mark.parametrize("dtype,predictor", host.CASES)
def test_deflate_strips_from_libtiff(dbm, tmp_path, dtype, predictor):
    a = np.random.default_rng(12).normal(0.0, 300.0, (70, 300)).astype(dtype)
    if dtype == "float32":
        a[3, 5:9] = np.nan
    path = host.pillow_save(tmp_path / "d.tif", a, {317: predictor, 278: 16}, compression="tiff_adobe_deflate")
    assert dbm.open_geotiff(path).plan().blocks[:, 2].tolist() == [16, 16, 16, 16, 6]
    got, info = read_bits(dbm, path)
    assert info["compression"] == 8 and info["predictor"] == predictor and info["dtype"] == np.dtype(dtype)
    assert np.array_equal(got, f32_bits(host.pillow_decode(path, dtype)))


@pytest.mark.parametrize("bigtiff", [False, True])
@pytest.mark.parametrize("predictor", [1, 3])
def test_deflate_tiles(dbm, tmp_path, plane, predictor, bigtiff):
    from deepbedmap_amd import geotiff

    path = rs.write_deflate_tiles(tmp_path / "t.tif", plane, BOUND, predictor=predictor, bigtiff=bigtiff)
    got, info = read_bits(dbm, path)
    assert info["compression"] == 8 and info["predictor"] == predictor and info["bigtiff"] == bigtiff and info["tile"] == (256, 256)
    assert np.array_equal(got, bits(plane))
    dev, _ = dbm.read_geotiff_resident(path, inflate="host")
    assert np.array_equal(got, bits(dev.get()))
    # a window that takes blocks 0 and 1 only
    wb = (BOUND[0], BOUND[3] - 25600, BOUND[0] + 51200, BOUND[3])
    assert dbm.open_geotiff(path).plan(wb).blocks[:, 5].tolist() == [0, 1]
    part, info = read_bits(dbm, path, window_bound=wb)
    assert info["window"] == (0, 0, 256, 512) and np.array_equal(part, bits(plane[:256, :512]))
    # batches: a deflate block is charged its stream when it is inflated on the device
    gf = dbm.open_geotiff(path)
    assert len(geotiff._batches(gf, gf.plan(), 1, True)) == 6 and len(geotiff._batches(gf, gf.plan(), 1 << 30, True)) == 1
    for limit in (1, 300000):
        many, _ = read_bits(dbm, path, workspace_limit=limit)
        assert np.array_equal(many, got)


def _as_block(stream, raw):
    """One uint8 block through dbm_tiff_decode with compression 8: the bytes as float32.  256 columns wide where the stream decodes
    to whole rows of 256; otherwise (60 000 bytes, the token streams, the one byte) a single row as long as the stream decodes to."""
    from deepbedmap_amd import _lib
    from deepbedmap_amd.resident import DeviceArray, devptr

    w = 256 if len(raw) % 256 == 0 else len(raw)
    rows = len(raw) // w
    ctx = _lib.default_context()
    out = DeviceArray((rows, w), ctx)
    payload = np.frombuffer(stream, dtype=np.uint8)
    table = np.array([[0, len(stream), rows, 0, 0, 7, 0, 0]], dtype=np.int64)
    ctx.call("dbm_tiff_decode", devptr(payload), payload.size, devptr(table), 1, 8, 1, 0, w, rows, devptr(out), rows, w)
    out.written()
    return out.get()


RAW = ["a_level0", "a_level6", "a_fixed", "b_zeros", "c_huffman_only", "d_full_flush", "e_wbits9", "f_one_byte", "distance_32768_at_32768",
       "distance_3_length_258", "distance_1_length_3_at_1", "match_258_across_64", "one_distance_code", "no_distance_code",
       "literal_code_of_15_bits"]


@pytest.mark.parametrize("name", RAW)
def test_raw_streams(dbm, name):
    streams = dict(rs.zlib_streams())
    streams.update(rs.token_streams())
    assert set(RAW) == {k for k, v in streams.items() if v[1] is not None}
    stream, raw = streams[name]
    assert zlib.decompress(stream) == raw
    got = _as_block(stream, raw)
    assert np.array_equal(got.ravel(), np.frombuffer(raw, dtype=np.uint8).astype(np.float32))


def test_malformed_streams_are_reported_by_block(dbm, tmp_path, plane):
    """Block 2 of a 2 x 3-tile file replaced by each stream that tests/test_inflate_host.py and tools/inflate_twin_check.cpp have seen
    the one-lane twin refuse on the CPU: the device reports status 11 and names the block; the other blocks still read."""
    from deepbedmap_amd import geotiff

    good = rs.write_deflate_tiles(tmp_path / "good.tif", plane, BOUND)
    cases = {k: v for k, v in rs.refusals().items() if k != "junk_behind"}
    cases["distance_32768_at_32767"] = rs.token_streams()["distance_32768_at_32767"][0]
    cases["short"] = zlib.compress(bytes(1000))          # a good stream of another size
    cases["long"] = zlib.compress(bytes(256 * 256 * 4 + 1))
    for name, stream in cases.items():
        with pytest.raises(dbm.DbmError):
            geotiff.inflate(stream, 256 * 256 * 4)
        bad = rs.write_deflate_tiles(tmp_path / (name + ".tif"), plane, BOUND, replace={2: stream})
        with pytest.raises(dbm.DbmError, match=r"block 2\b.*deflate") as e:
            dbm.read_geotiff_resident(bad, inflate="device")
        assert e.value.code == 11, name
        got, _ = read_bits(dbm, bad, window_bound=(BOUND[0], BOUND[3] - 25600, BOUND[0] + 51200, BOUND[3]))
        assert np.array_equal(got, bits(plane[:256, :512])), name
    assert np.array_equal(read_bits(dbm, good)[0], bits(plane))


def test_only_compressed_bytes_cross(dbm, tmp_path, plane, monkeypatch):
    from deepbedmap_amd import _lib

    path = rs.write_deflate_tiles(tmp_path / "p.tif", plane, BOUND, predictor=3)
    plan = dbm.open_geotiff(path).plan()
    ctx = _lib.default_context()
    calls = []
    real = ctx.call

    def record(name, *args):
        calls.append((name, args))
        return real(name, *args)

    def no_zlib(*a, **k):
        raise AssertionError("zlib.decompress on the device path")

    monkeypatch.setattr(ctx, "call", record)
    monkeypatch.setattr(zlib, "decompress", no_zlib)
    dev, _ = dbm.read_geotiff_resident(path, inflate="device", workspace_limit=600000, ctx=ctx)
    monkeypatch.undo()
    decodes = [args for name, args in calls if name == "dbm_tiff_decode"]
    assert len(decodes) > 1 and all(args[4] == 8 for args in decodes)
    assert sum(int(args[1]) for args in decodes) == int(plan.blocks[:, 1].sum()) < 6 * 256 * 256 * 4 // 2   # (the host path uploads the six decoded tiles)
    assert np.array_equal(bits(dev.get()), bits(plane))
