"""CPU checks of the writer's predictor 2 (`save_array_to_grid(predictor=2)`: horizontal differencing per block row on the host, tag
317) against Pillow / libtiff's decode and `read_geotiff`, of the unchanged bytes without the keyword, and of the
refusals of `write_geotiff_resident` that need no device.  Every comparison is on bytes or bits; no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_geotiff_open_host as host  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402
from deepbedmap_amd import geotiff  # noqa: E402

BOUND = host.BOUND
bits = host.bits


def plane(shape, dtype):
    a = np.random.default_rng(21).normal(0.0, 300.0, shape).astype(np.float32)
    a[10:30, 40:200] = -2000.0
    if dtype == "float32":
        a[3, 5:9] = np.nan
        a[4, 7] = np.inf
        return a
    return a.astype(np.int16)


@pytest.mark.parametrize("shape", [(70, 300), (300, 520)])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_predictor_2_decodes_with_libtiff_and_read_geotiff(tmp_path, dtype, tiled, shape):
    a = plane(shape, dtype)
    path = dbm.save_array_to_grid(str(tmp_path / "p"), BOUND, a[None], tiled=tiled, compression="lzw", predictor=2)
    gf = geotiff.open_geotiff(path)
    assert gf.predictor == 2 and gf.tags[317] == [2] and gf.tiled == tiled and gf.dtype == np.dtype(dtype)
    assert np.array_equal(bits(host.pillow_decode(path, dtype)), bits(a))
    back, info = dbm.read_geotiff(path)
    assert back.dtype == np.dtype(dtype) and np.array_equal(bits(back[0]), bits(a))
    assert np.array_equal(bits(host.host_decode(path)), bits(a))   # (the restatement of what the device reader computes)
    # the differenced blocks are what the file holds: its first block's stream decodes to the differences, not to the samples
    th, tw = (256, 256) if tiled else (min(256, shape[0]), shape[1])
    blocks, _, _ = geotiff._tiles_of(a, th, tw)
    u = blocks[0].view("<u%d" % a.dtype.itemsize)
    want = u.copy()
    want[:, 1:] = u[:, 1:] - u[:, :-1]
    raw = geotiff.lzw_decode(open(path, "rb").read()[gf.offsets[0]:gf.offsets[0] + gf.counts[0]], want.nbytes)
    assert np.array_equal(raw, want.reshape(-1).view(np.uint8))


@pytest.mark.parametrize("kw", [dict(tiled=True, compression="lzw", dtype=np.int16), dict(tiled=False, compression="lzw"),
                                dict(tiled=True, compression="none", bigtiff=False), dict()])
def test_without_the_keyword_the_file_is_unchanged(tmp_path, kw):
    a = plane((300, 520), "float32")
    plain = dbm.save_array_to_grid(str(tmp_path / "a"), BOUND, a[None], **kw)
    one = dbm.save_array_to_grid(str(tmp_path / "b"), BOUND, a[None], predictor=1, **kw)
    assert open(plain, "rb").read() == open(one, "rb").read()
    assert 317 not in geotiff.open_geotiff(plain).tags


def test_unchanged_bytes_of_a_known_file(tmp_path):
    """The container helper that both writers share writes what the writer wrote before it was factored out: a small file's bytes,
    spelled out (classic TIFF, one strip, uncompressed)."""
    a = np.arange(6, dtype=np.int16).reshape(1, 2, 3)
    path = dbm.save_array_to_grid(str(tmp_path / "k"), (0.0, 0.0, 3.0, 2.0), a, bigtiff=False)
    buf = open(path, "rb").read()
    assert buf[:8] == b"II*\0" + (20).to_bytes(4, "little")                  # header, IFD behind the 12 bytes of samples
    assert buf[8:20] == a.astype("<i2").tobytes()
    assert int.from_bytes(buf[20:22], "little") == 15                         # twelve common tags + RowsPerStrip, offsets, counts
    tags = [int.from_bytes(buf[22 + 12 * k:24 + 12 * k], "little") for k in range(15)]
    assert tags == sorted(tags) == [256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 339, 33550, 33922, 34735, 42113]
    back, info = dbm.read_geotiff(path)
    assert np.array_equal(back, a) and info["nodata"] == "-2000"


def test_predictor_on_uncompressed_data_has_no_effect(tmp_path):
    """libtiff's predictors belong to its codecs: an uncompressed file holds the samples as they are and carries no tag 317."""
    a = plane((70, 300), "int16")
    p1 = dbm.save_array_to_grid(str(tmp_path / "n1"), BOUND, a[None], compression="none")
    p2 = dbm.save_array_to_grid(str(tmp_path / "n2"), BOUND, a[None], compression="none", predictor=2)
    assert open(p1, "rb").read() == open(p2, "rb").read()


def test_save_array_to_grid_refuses_other_predictors(tmp_path):
    a = plane((70, 300), "float32")
    for bad in (0, 3, "2", True, None):
        with pytest.raises(ValueError, match="save_array_to_grid: predictor"):
            dbm.save_array_to_grid(str(tmp_path / "x"), BOUND, a[None], compression="lzw", predictor=bad)
    assert not os.path.exists(str(tmp_path / "x.tif"))


class FakeContext:
    """A context that fails the test if anything reaches the device."""

    def malloc(self, nbytes):
        return 4096

    def free(self, ptr):
        pass

    def call(self, name, *args):
        raise AssertionError(f"{name} was called: the refusal must come before any device work")


def test_write_geotiff_resident_refusals_need_no_device(tmp_path):
    out = str(tmp_path / "r")
    ctx = FakeContext()
    good = dbm.DeviceArray((1, 70, 300), ctx=ctx)
    write = dbm.write_geotiff_resident
    with pytest.raises(ValueError, match="write_geotiff_resident: array must be a float32 DeviceArray or a resident Raster, not ndarray"):
        write(out, BOUND, np.zeros((1, 70, 300), dtype=np.float32))
    for dtype in (np.float64, np.int32, np.uint8):
        with pytest.raises(ValueError, match=f"write_geotiff_resident: array holds {np.dtype(dtype).name}"):
            write(out, BOUND, dbm.DeviceArray((1, 70, 300), ctx=ctx, dtype=dtype))
    with pytest.raises(ValueError, match=r"write_geotiff_resident: array must be \(1, H, W\) or \(H, W\)"):
        write(out, BOUND, dbm.DeviceArray((2, 70, 300), ctx=ctx))
    host_raster = dbm.Raster(np.zeros((70, 300), dtype=np.float32), dbm.GridGeometry.from_bounds(BOUND, 70, 300))
    with pytest.raises(ValueError, match="write_geotiff_resident: array: the Raster is not resident"):
        write(out, BOUND, host_raster)
    for dtype in (np.float64, np.int32, np.uint8, "uint16"):
        with pytest.raises(ValueError, match="write_geotiff_resident: dtype"):
            write(out, BOUND, good, dtype=dtype)
    for predictor in (3, 0, "2"):
        with pytest.raises(ValueError, match="write_geotiff_resident: predictor"):
            write(out, BOUND, good, predictor=predictor)
    for compression in ("deflate", "zstd", 8):
        with pytest.raises(ValueError, match="write_geotiff_resident: unsupported compression"):
            write(out, BOUND, good, compression=compression)
    for limit in (0, []):   # (not positive; not a number: the documented ValueError, where a bare int() raised TypeError)
        with pytest.raises(ValueError, match="write_geotiff_resident: workspace_limit"):
            write(out, BOUND, good, workspace_limit=limit)
    with pytest.raises(ValueError, match="crs"):
        write(out, BOUND, good, crs="+proj=utm +zone=33")
    assert not os.path.exists(out + ".tif")


def test_the_entry_point_is_declared_and_documented():
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "dbm.h")).read()
    i = header.index("int dbm_tiff_encode(")
    comment = header[header.rindex("/*", 0, i):i]
    assert "deepbedmap.py:749-756" in comment and "data_prep.py:779-834" in comment and "Status 12" in comment
    api = open(os.path.join(root, "deepbedmap_amd", "csrc", "api_data.hip")).read()
    assert "DbmError(12," in api and "write_geotiff_resident" in dbm.__dict__
