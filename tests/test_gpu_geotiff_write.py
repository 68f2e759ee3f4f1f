"""-m gpu: `write_geotiff_resident` (dbm_tiff_encode: cast, block cutting, predictor 2 and TIFF 6.0 LZW by one wavefront per block on
the device) against the host writer and independent decoders.  LZW's output is determined by its rule, so the device's
file must equal, byte for byte, the file `save_array_to_grid` writes from the downloaded plane; Pillow / libtiff and
`read_geotiff_resident` then decode it back to the plane's bits.  No comparison has a tolerance.

Shapes: 256 x 256 (one whole tile), 300 x 520 (tiled: 2 x 3 tiles padded right and below; strips: 256 rows plus a short strip of 44)
and 1 x 1, 3 x 5 (blocks of 2 to 60 bytes: the encoder's start and end paths)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_geotiff_open_host as host  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = host.BOUND
bits = host.bits
SHAPES = [(256, 256), (300, 520), (1, 1), (3, 5)]


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


def as_written(a, dtype):
    """The samples a file of `dtype` holds for the float32 plane `a`: NumPy's cast, on the host."""
    with np.errstate(invalid="ignore"):
        return a.astype(dtype)


def both_files(dbm, tmp_path, a, name="f", **kw):
    """(device-written file, host-written file from the downloaded plane) with the same arguments."""
    dev = dbm.to_device(a[None])
    got = dbm.write_geotiff_resident(str(tmp_path / (name + "_dev")), BOUND, dev, **kw)
    assert got == str(tmp_path / (name + "_dev")) + ".tif"
    kw.pop("workspace_limit", None)
    want = dbm.save_array_to_grid(str(tmp_path / (name + "_host")), BOUND, dev.get(), **kw)
    return got, want


def same_bytes(got, want):
    a, b = open(got, "rb").read(), open(want, "rb").read()
    if a != b:
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError(f"{got}: {len(a)} bytes, {want}: {len(b)} bytes, first difference at byte {first}")


def check_decodes(dbm, path, a, dtype):
    """Pillow / libtiff and the device reader return the written samples' bits."""
    want = as_written(a, dtype)
    assert np.array_equal(bits(host.pillow_decode(path, dtype)), bits(want))
    back, info = dbm.read_geotiff_resident(path)
    assert info["dtype"] == np.dtype(dtype)
    assert np.array_equal(bits(back.get()), bits(want.astype(np.float32)))


@pytest.mark.parametrize("bigtiff", [True, False])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_file_equals_the_host_writers(dbm, tmp_path, plane, shape, dtype, predictor, tiled, bigtiff):
    a = np.ascontiguousarray(plane[:shape[0], :shape[1]])
    got, want = both_files(dbm, tmp_path, a, dtype=dtype, predictor=predictor, tiled=tiled, bigtiff=bigtiff, compression="lzw", nodataval=-9999)
    same_bytes(got, want)
    gf = dbm.open_geotiff(got)
    assert gf.tiled == tiled and gf.predictor == predictor and gf.bigtiff == bigtiff and gf.compression == 5
    if shape == (300, 520):
        assert len(gf.offsets) == (6 if tiled else 2)
        if not tiled:
            assert gf.plan().blocks[:, 2].tolist() == [256, 44]


@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_independent_decoders_return_the_plane(dbm, tmp_path, plane, shape, dtype, predictor, tiled):
    a = np.ascontiguousarray(plane[:shape[0], :shape[1]])
    path = dbm.write_geotiff_resident(str(tmp_path / "d"), BOUND, dbm.to_device(a), dtype=dtype, predictor=predictor, tiled=tiled, nodataval=-9999)
    check_decodes(dbm, path, a, dtype)
    back, info = dbm.read_geotiff(path)
    assert info["nodata"] == "-9999" and np.array_equal(bits(back[0]), bits(as_written(a, dtype)))


def contents():
    r = np.random.default_rng(9)
    noise = r.normal(0.0, 300.0, (256, 256)).astype(np.float32)
    constant = np.full((256, 256), -2000.0, dtype=np.float32)
    half = constant.copy()
    half[128:] = noise[128:]
    ramp = (3.0 * np.arange(256, dtype=np.float32)[None, :] + np.arange(256, dtype=np.float32)[:, None]).astype(np.float32)
    special = noise.copy()
    special[0, :8] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3.4e38, -1.5]
    special[100:160, 30:200] = -2000.0
    uniform = r.integers(-32768, 32768, (256, 256)).astype(np.float32)
    return {"noise": (noise, "int16"), "constant": (constant, "int16"), "half": (half, "int16"), "ramp": (ramp, "int16"),
            "special": (special, "float32"), "uniform": (uniform, "int16")}


CONTENTS = contents()


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("kind", sorted(CONTENTS))
def test_contents_that_reach_every_path_of_the_encoder(dbm, tmp_path, kind, predictor):
    a, dtype = CONTENTS[kind]
    got, want = both_files(dbm, tmp_path, a, dtype=dtype, predictor=predictor, tiled=True, compression="lzw")
    stream = int(dbm.open_geotiff(want).counts[0])   # the HOST stream of the one tile
    raw = 256 * 256 * np.dtype(dtype).itemsize
    if kind == "noise" and predictor == 1:
        assert stream > 8 * 1024, stream       # far more than 3836 table entries: table resets and all four code widths occur
    if kind == "constant" and predictor == 1:
        # one two-byte pattern throughout: string k is k bytes long, so about sqrt(2 * 131072) = 512 codes of <= 10 bits, < 1 KiB,
        # and the matches grow to hundreds of bytes (after predictor 2 every row starts anew with the sample itself)
        assert stream < 1024, stream
    if kind == "uniform" and predictor == 1:
        assert stream > raw, (stream, raw)     # the part of the slot beyond block_bytes is in use
    same_bytes(got, want)
    check_decodes(dbm, got, a, dtype)


def test_the_cast_is_numpys(dbm, tmp_path):
    canvas = np.full((40, 70), np.nan, dtype=np.float32)     # the NaN frame that no tile covers
    canvas[4:36, 5:65] = np.random.default_rng(4).normal(-500.0, 900.0, (32, 60)).astype(np.float32)
    canvas[5, 6:13] = [np.inf, -np.inf, 40000.7, -32769.5, -0.9, 2.5e9, -2.5e9]
    want = dbm.canvas_to_int16(canvas)
    assert want[5, 6:13].tolist() == [0, 0, -25536, 32767, 0, 0, 0] and want[0, 0] == 0
    dev = dbm.to_device(canvas[None])
    assert np.array_equal(dbm.canvas_to_int16(dev)[0], want)   # (the kernel that shares the cast's code)
    for tiled in (True, False):
        for predictor in (1, 2):
            path = dbm.write_geotiff_resident(str(tmp_path / "c"), BOUND, dev, dtype=np.int16, tiled=tiled, predictor=predictor)
            back, _ = dbm.read_geotiff(path)
            assert back.dtype == np.int16 and np.array_equal(back[0], want)
            assert np.array_equal(host.pillow_decode(path, "int16"), want)


def test_batches_write_the_same_file(dbm, tmp_path, plane, monkeypatch):
    dev = dbm.to_device(plane)     # (H, W)
    whole = dbm.write_geotiff_resident(str(tmp_path / "whole"), BOUND, dev, dtype=np.int16)
    calls = []
    real = dev.ctx.call
    monkeypatch.setattr(dev.ctx, "call", lambda name, *args: (calls.append((name, args[9], args[10])), real(name, *args))[1], raising=False)
    parts = dbm.write_geotiff_resident(str(tmp_path / "parts"), BOUND, dev, dtype=np.int16, workspace_limit=700_000)
    one = dbm.write_geotiff_resident(str(tmp_path / "one"), BOUND, dev, dtype=np.int16, workspace_limit=1)   # one block always goes through
    monkeypatch.undo()
    # 131072 raw bytes + a slot of 196672 per block: two blocks per batch, three batches
    assert [c for c in calls if c[0] == "dbm_tiff_encode"][:3] == [("dbm_tiff_encode", 0, 2), ("dbm_tiff_encode", 2, 2), ("dbm_tiff_encode", 4, 2)]
    assert len(calls) == 3 + 6
    same_bytes(parts, whole)
    same_bytes(one, whole)


def test_a_short_last_batch_writes_the_host_writers_file(dbm, tmp_path, monkeypatch):
    """Six strips of 8 samples a row (five of 256 rows, one of 20), four per call: the last call takes the two that are left."""
    a = np.random.default_rng(6).normal(0.0, 300.0, (1300, 8)).astype(np.float32)
    strip = 256 * 8 * 2
    calls = []
    real = dbm.default_context().call
    monkeypatch.setattr(dbm.default_context(), "call", lambda name, *args: (calls.append((name,) + args[9:11]), real(name, *args))[1],
                        raising=False)
    got, want = both_files(dbm, tmp_path, a, dtype="int16", tiled=False, compression="lzw", workspace_limit=4 * (strip + strip * 3 // 2 + 64))
    monkeypatch.undo()
    assert [c for c in calls if c[0] == "dbm_tiff_encode"] == [("dbm_tiff_encode", 0, 4), ("dbm_tiff_encode", 4, 2)]
    same_bytes(got, want)


@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_uncompressed_with_predictor_2(dbm, tmp_path, plane, dtype, tiled):
    """compression="none" downloads stage (a)'s bytes.  libtiff's predictors belong to its codecs, so both writers leave the samples as
    they are and write no tag 317."""
    got, want = both_files(dbm, tmp_path, plane, dtype=dtype, predictor=2, tiled=tiled, compression="none", bigtiff=False)
    same_bytes(got, want)
    gf = dbm.open_geotiff(got)
    assert gf.compression == 1 and 317 not in gf.tags
    check_decodes(dbm, got, plane, dtype)


def test_a_written_file_feeds_the_readers(dbm, tmp_path, plane):
    import warnings

    source = dbm.Raster(dbm.to_device(plane), dbm.GridGeometry.from_bounds(BOUND, 300, 520), nodata=-9999.0)
    path = dbm.write_geotiff_resident(str(tmp_path / "r"), BOUND, source, predictor=2, nodataval=-9999)   # a resident Raster, float32
    opened = dbm.Raster.open(path)
    assert opened.shape == source.shape and opened.geometry == source.geometry and opened.nodata == source.nodata
    minx, _, _, maxy = BOUND
    windows = [(minx + 1000 + 700 * k, maxy - 9000 - 500 * k, minx + 4600 + 700 * k, maxy - 5400 - 500 * k) for k in range(5)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in ({"interpolate": False}, {"padding": 1000, "resolution": 250.0, "gapfiller": -5000.0}):
            a = dbm.selective_tile(opened, windows, **kw).get()
            b = dbm.selective_tile(source, windows, **kw).get()
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_refusals_of_the_entry_point(dbm):
    """Status 1 before any device work: the block range, the output capacity, strips that are not W wide."""
    import ctypes as C

    from deepbedmap_amd import _lib
    from deepbedmap_amd.resident import devptr

    dev = dbm.to_device(np.zeros((300, 520), dtype=np.float32))
    out, sizes = np.zeros(6 * 196672, dtype=np.uint8), np.zeros(6, dtype=np.uintp)

    def call(*, H=300, W=520, sample_type=1, bh=256, bw=256, tiled=1, predictor=1, compression=5, first=0, n=6, cap=None, plane=dev):
        dev.ctx.call("dbm_tiff_encode", devptr(plane), H, W, sample_type, bh, bw, tiled, predictor, compression, first, n, devptr(out),
                     out.size if cap is None else cap, devptr(sizes))

    call()
    assert (sizes > 0).all()
    call(n=0)
    for bad, message in ((dict(first=5, n=2), "block range"), (dict(first=-1), "block range"), (dict(cap=6 * 196672 - 1), "worst case"),
                         (dict(tiled=0), "strips are W wide"), (dict(predictor=3), "predictor"), (dict(sample_type=2), "sample_type"),
                         (dict(compression=8), "compression"), (dict(bh=0), "a block must hold"), (dict(H=0), "empty plane"),
                         (dict(plane=None), "NULL plane")):
        with pytest.raises(_lib.DbmError, match=message) as e:
            call(**bad)
        assert e.value.code == 1, bad
    assert C.sizeof(C.c_size_t) == sizes.itemsize
