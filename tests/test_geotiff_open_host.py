"""CPU checks of `geotiff.open_geotiff` (header, geometry, block plan, refusals) and the statement of the predictor
semantics that tests/test_gpu_geotiff_read.py leans on: a NumPy restatement of the predictor 2 / 3 undo, kept here, reproduces
Pillow's (libtiff's) decode of Pillow-written files from the streams that `open_geotiff` plans and `dbm_lzw_decode` / zlib decode."""
import os
import struct
import zlib

import numpy as np
import pytest

import deepbedmap_amd as dbm
from deepbedmap_amd import geotiff

BOUND = (-1000.0, 2000.0, 51000.0, 32000.0)   # 520 x 300 pixels of 100 m


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def undo_predictor(rows, dtype, predictor):
    """rows: (nrows, row bytes) uint8 as decoded from the file -> (nrows, W) samples of `dtype`.
    2: each row is a running sum of its samples, wrapping in the sample's width (floats: on the bit patterns).
    3: each row's bytes are a running sum modulo 256; then byte plane k (W bytes) holds byte k of every sample, most significant first."""
    dtype = np.dtype(dtype)
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if predictor == 1:
        return rows.view(dtype)
    if predictor == 2:
        u = np.dtype("<u%d" % dtype.itemsize)
        return np.cumsum(rows.view(u), axis=1, dtype=u).view(dtype)
    assert predictor == 3 and dtype.kind == "f"
    acc = np.cumsum(rows, axis=1, dtype=np.uint8)
    n, w = rows.shape[0], rows.shape[1] // dtype.itemsize
    planes = acc.reshape(n, dtype.itemsize, w)            # plane 0 = most significant byte
    return np.ascontiguousarray(planes[:, ::-1, :].transpose(0, 2, 1)).reshape(n, w * dtype.itemsize).view(dtype)


def host_decode(path, window_bound=None):
    """The whole read on the host, from open_geotiff's plan: the restatement of what read_geotiff_resident computes, before the float32
    cast."""
    gf = geotiff.open_geotiff(path)
    plan = gf.plan(window_bound)
    r0, c0, H, W = plan.window
    out = np.zeros((H, W), dtype=gf.dtype)
    buf = open(path, "rb").read()
    for off, cnt, rows, orow, ocol, _ in plan.blocks:
        want = rows * gf.block_w * gf.dtype.itemsize
        s = buf[off:off + cnt]
        raw = geotiff.lzw_decode(s, want) if gf.compression == 5 else np.frombuffer(zlib.decompress(s) if gf.compression != 1 else s, dtype=np.uint8)[:want]
        block = undo_predictor(np.asarray(raw).reshape(rows, -1), gf.dtype, gf.predictor)
        ra, rb = max(orow, 0), min(orow + rows, H)
        ca, cb = max(ocol, 0), min(ocol + gf.block_w, W)
        out[ra:rb, ca:cb] = block[ra - orow:rb - orow, ca - ocol:cb - ocol]
    return out


def _write(tmp_path, name, array, **kw):
    return dbm.save_array_to_grid(str(tmp_path / name), BOUND, array[None], **kw)


@pytest.fixture(scope="module")
def plane():
    return np.random.default_rng(5).normal(0.0, 300.0, (300, 520)).astype(np.float32)


@pytest.mark.parametrize("bigtiff", [False, True])
@pytest.mark.parametrize("tiled", [False, True])
def test_header_and_plan_of_the_package_writer(tmp_path, plane, bigtiff, tiled):
    path = _write(tmp_path, "a", plane, tiled=tiled, compression="lzw", bigtiff=bigtiff, nodataval=-9999)
    gf = geotiff.open_geotiff(path)
    assert gf.shape == (300, 520) and gf.dtype == np.float32 and gf.compression == 5 and gf.predictor == 1
    assert gf.bigtiff == bigtiff and gf.tiled == tiled and gf.nodata == "-9999"
    assert (gf.block_h, gf.block_w) == ((256, 256) if tiled else (256, 520))
    assert gf.geometry == dbm.GridGeometry.from_bounds(BOUND, 300, 520)
    plan = gf.plan()
    assert plan.window == (0, 0, 300, 520)
    b = plan.blocks
    if tiled:   # 2 x 3 tiles, all whole (edge tiles are padded)
        assert len(b) == 6 and (b[:, 2] == 256).all()
        assert b[:, 3].tolist() == [0, 0, 0, 256, 256, 256] and b[:, 4].tolist() == [0, 256, 512, 0, 256, 512]
    else:       # the last strip holds the 44 rows that exist
        assert b[:, 2].tolist() == [256, 44] and b[:, 3].tolist() == [0, 256] and b[:, 4].tolist() == [0, 0]
    assert b[:, 5].tolist() == list(range(len(b)))
    _, info = dbm.read_geotiff(path)
    assert b[:, 1].sum() <= os.path.getsize(path) and info["tile"] == (gf.block_h, gf.block_w)
    assert np.array_equal(bits(host_decode(path)), bits(plane))


def test_window_rule(tmp_path, plane):
    path = _write(tmp_path, "w", plane, tiled=True, compression="lzw")
    gf = geotiff.open_geotiff(path)
    minx, miny, maxx, maxy = BOUND
    # bounds on pixel edges: rows 10..29, columns 250..269 (across tiles 0 and 1)
    assert gf.window((minx + 25000, maxy - 3000, minx + 27000, maxy - 1000)) == (10, 250, 20, 20)
    # unaligned: centres in [minx, maxx) x (miny, maxy]; a centre exactly on minx / maxy is in, on maxx / miny is out
    assert gf.window((minx + 50, maxy - 250, minx + 250, maxy - 50)) == (0, 0, 2, 2)
    assert gf.window((minx + 49, maxy - 251, minx + 251, maxy - 49)) == (0, 0, 3, 3)
    assert gf.window((minx + 60, maxy - 240, minx + 240, maxy - 60)) == (1, 1, 1, 1)
    # leaving the image on each side: clipped
    assert gf.window((minx - 5000, maxy - 1000, minx + 1000, maxy + 5000)) == (0, 0, 10, 10)
    assert gf.window((maxx - 1000, miny - 5000, maxx + 5000, miny + 1000)) == (290, 510, 10, 10)
    assert gf.window((minx - 1, miny - 1, maxx + 1, maxy + 1)) == (0, 0, 300, 520)
    with pytest.raises(ValueError, match="holds no pixel centre"):
        gf.window((maxx + 100, miny, maxx + 1000, maxy))
    with pytest.raises(ValueError, match="holds no pixel centre"):
        gf.window((minx + 60, maxy - 90, minx + 90, maxy - 60))
    # the plan of a window: only the blocks that hold it, placed relative to the window
    plan = gf.plan((minx + 25000, maxy - 30000, minx + 27000, maxy - 25000))   # rows 250..299, columns 250..269
    assert plan.window == (250, 250, 50, 20)
    assert plan.blocks[:, 5].tolist() == [0, 1, 3, 4]
    assert plan.blocks[:, 3].tolist() == [-250, -250, 6, 6] and plan.blocks[:, 4].tolist() == [-250, 6, -250, 6]
    inside = gf.plan((minx + 30000, maxy - 2000, minx + 31000, maxy - 1000))
    assert inside.blocks[:, 5].tolist() == [1] and inside.window == (10, 300, 10, 10)
    assert np.array_equal(bits(host_decode(path, (minx + 25000, maxy - 30000, minx + 27000, maxy - 25000))), bits(plane[250:300, 250:270]))


def _patch_tags(path, out, edits, drop=()):
    """Rewrites the classic little-endian file `path` with inline values of some tags changed: edits = {tag: value} (SHORT / LONG
    fields with one value), drop = tags whose id becomes 65000 (an unknown private tag)."""
    buf = bytearray(open(path, "rb").read())
    ifd = struct.unpack_from("<I", buf, 4)[0]
    n = struct.unpack_from("<H", buf, ifd)[0]
    seen = set()
    for k in range(n):
        pos = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack_from("<HHI", buf, pos)
        if tag in edits:
            assert count == 1 and typ in (3, 4)
            struct.pack_into("<H" if typ == 3 else "<I", buf, pos + 8, edits[tag])
            seen.add(tag)
        if tag in drop:
            struct.pack_into("<H", buf, pos, 65000)
            seen.add(tag)
    assert seen == set(edits) | set(drop)
    open(out, "wb").write(bytes(buf))
    return str(out)


def test_refusals_name_the_tag_and_the_value(tmp_path, plane):
    small = plane[:40, :50]
    path = _write(tmp_path, "r", small, compression="lzw", bigtiff=False)
    for edits, match in (({277: 3}, r"SamplesPerPixel \(277\) = 3"),
                         ({259: 7}, r"Compression \(259\) = 7"),
                         ({259: 50000}, r"Compression \(259\) = 50000"),
                         ({258: 16}, r"BitsPerSample \(258\) = 16 with SampleFormat \(339\) = 3"),
                         ({339: 4}, r"SampleFormat \(339\) = 4")):
        with pytest.raises(ValueError, match=match):
            geotiff.open_geotiff(_patch_tags(path, tmp_path / "bad.tif", edits))
    # big endian
    buf = bytearray(open(path, "rb").read())
    buf[:2] = b"MM"
    (tmp_path / "mm.tif").write_bytes(bytes(buf))
    with pytest.raises(ValueError, match="byte order 'MM'"):
        geotiff.open_geotiff(tmp_path / "mm.tif")
    (tmp_path / "nt.tif").write_bytes(b"PK\x03\x04 not a tiff at all")
    with pytest.raises(ValueError, match="not a TIFF"):
        geotiff.open_geotiff(tmp_path / "nt.tif")
    # old-style LZW: the first strip starts 00 01
    gf = geotiff.open_geotiff(path)
    buf = bytearray(open(path, "rb").read())
    buf[gf.offsets[0]:gf.offsets[0] + 2] = b"\x00\x01"
    (tmp_path / "old.tif").write_bytes(bytes(buf))
    with pytest.raises(ValueError, match=r"Compression \(259\) = 5 .* old-style LZW"):
        geotiff.open_geotiff(tmp_path / "old.tif")
    # no georeference: the file opens and plans, its geometry and a windowed plan are refused
    bare = geotiff.open_geotiff(_patch_tags(path, tmp_path / "bare.tif", {}, drop=(33550,)))
    assert bare.plan().window == (0, 0, 40, 50)
    with pytest.raises(ValueError, match=r"no georeference: ModelPixelScale \(33550\)"):
        bare.geometry
    with pytest.raises(ValueError, match="no georeference"):
        bare.plan((0, 0, 1, 1))
    with pytest.raises(ValueError, match="no georeference"):
        dbm.Raster.open(tmp_path / "bare.tif")
    # a block outside the file, a sparse block
    (tmp_path / "cut.tif").write_bytes(bytes(buf[:len(buf) // 2]))   # (the writer puts the IFD behind the pixel data)
    with pytest.raises(ValueError, match="outside the file"):
        geotiff.open_geotiff(tmp_path / "cut.tif")
    sparse = bytearray(open(path, "rb").read())
    ifd = struct.unpack_from("<I", sparse, 4)[0]
    for k in range(struct.unpack_from("<H", sparse, ifd)[0]):
        if struct.unpack_from("<H", sparse, ifd + 2 + 12 * k)[0] == 279:
            struct.pack_into("<I", sparse, ifd + 2 + 12 * k + 8, 0)
    (tmp_path / "sparse.tif").write_bytes(bytes(sparse))
    with pytest.raises(ValueError, match=r"StripByteCounts \(279\)\[0\] = 0"):
        geotiff.open_geotiff(tmp_path / "sparse.tif").plan()
    with pytest.raises(ValueError, match="workspace_limit"):
        dbm.read_geotiff_resident(path, workspace_limit=0)


def pillow_save(path, array, tiffinfo, **kw):
    """Pillow / libtiff as the independent encoder.  int16 goes in as its uint16 bit patterns with SampleFormat 2 (Pillow would widen an
    int16 array to 32 bits); Pillow reads such a file back as int32 values."""
    Image = pytest.importorskip("PIL.Image")
    if array.dtype == np.int16:
        array = array.view(np.uint16)
        tiffinfo[339] = 2
    Image.fromarray(array).save(str(path), tiffinfo=tiffinfo, **kw)
    return str(path)


def pillow_decode(path, dtype):
    Image = pytest.importorskip("PIL.Image")
    return np.array(Image.open(path)).astype(dtype)


def _with_extra_tags(tmp_path, array, name, tiffinfo, **kw):
    return pillow_save(tmp_path / name, array, tiffinfo, **kw)


def test_predictor_and_rotation_refusals_and_pixel_is_point(tmp_path):
    TiffImagePlugin = pytest.importorskip("PIL.TiffImagePlugin")
    a = np.arange(12, dtype=np.int16).reshape(3, 4)

    def info(extra):
        ifd = TiffImagePlugin.ImageFileDirectory_v2()
        for tag, (typ, val) in extra.items():
            ifd[tag] = val
            ifd.tagtype[tag] = typ
        return ifd

    scale, tie = (12, (100.0, 100.0, 0.0)), (12, (0.0, 0.0, 0.0, 5000.0, 7000.0, 0.0))
    area = geotiff.open_geotiff(_with_extra_tags(tmp_path, a, "area.tif", info({33550: scale, 33922: tie, 42113: (2, "-2000")})))
    assert area.geometry == dbm.GridGeometry(x0=5050.0, y0=6950.0, dx=100.0, dy=-100.0, registration="pixel") and area.nodata == "-2000"
    point = geotiff.open_geotiff(_with_extra_tags(tmp_path, a, "point.tif", info({33550: scale, 33922: tie,
                                                                                   34735: (3, (1, 1, 0, 2, 1024, 0, 1, 1, 1025, 0, 1, 2))})))
    assert point.geometry == dbm.GridGeometry(x0=5000.0, y0=7000.0, dx=100.0, dy=-100.0, registration="pixel") and point.nodata == ""
    straight = (100.0, 0.0, 0.0, 5000.0, 0.0, -100.0, 0.0, 7000.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert geotiff.open_geotiff(_with_extra_tags(tmp_path, a, "m.tif", info({34264: (12, straight)}))).geometry == area.geometry
    rotated = list(straight)
    rotated[1], rotated[4] = 3.0, -3.0
    with pytest.raises(ValueError, match=r"ModelTransformation \(34264\) = .*rotated"):
        geotiff.open_geotiff(_with_extra_tags(tmp_path, a, "rot.tif", info({34264: (12, tuple(rotated))}))).geometry
    # predictor 3 on integer samples, predictor 4
    plain = _with_extra_tags(tmp_path, a, "plain.tif", info({317: (3, 1)}))
    for value, match in ((3, r"Predictor \(317\) = 3 with int16"), (4, r"Predictor \(317\) = 4")):
        with pytest.raises(ValueError, match=match):
            geotiff.open_geotiff(_patch_tags(plain, tmp_path / "pred.tif", {317: value}))


CASES = [("float32", 1), ("float32", 2), ("float32", 3), ("int16", 1), ("int16", 2)]


@pytest.mark.parametrize("dtype,predictor", CASES)
@pytest.mark.parametrize("compression", ["tiff_lzw", "tiff_adobe_deflate"])
def test_numpy_restatement_of_the_predictors_reproduces_libtiff(tmp_path, dtype, predictor, compression):
    r = np.random.default_rng(11)
    a = r.normal(0.0, 300.0, (70, 300)).astype(dtype)
    if dtype == "float32":
        a[3, 5:9] = np.nan
    path = pillow_save(tmp_path / "p.tif", a, {317: predictor, 278: 16}, compression=compression)
    gf = geotiff.open_geotiff(path)
    assert gf.dtype == np.dtype(dtype) and gf.predictor == predictor and gf.compression == (5 if compression == "tiff_lzw" else 8) and not gf.tiled
    assert gf.block_h == 16 and gf.plan().blocks[:, 2].tolist() == [16, 16, 16, 16, 6]   # 70 rows: the last strip is short
    expected = pillow_decode(path, dtype)
    assert np.array_equal(bits(expected), bits(a))
    assert np.array_equal(bits(host_decode(path)), bits(expected))


def test_read_geotiff_misreads_a_predictor_file(tmp_path):
    """Why the new reader: the parent's read_geotiff ignores the Predictor tag."""
    a = np.random.default_rng(2).normal(0.0, 300.0, (70, 300)).astype(np.int16)
    path = pillow_save(tmp_path / "p.tif", a, {317: 2, 278: 16}, compression="tiff_lzw")
    old, _ = dbm.read_geotiff(path)
    assert not np.array_equal(old[0], a) and np.array_equal(host_decode(path), a)
