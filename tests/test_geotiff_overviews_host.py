"""CPU checks of GeoTIFF overviews ("Overviews"): the shapes, the NumPy statement `overview_pyramid` against the
loop-per-pixel restatement (tests/pyramid_restatement.py) bit for bit, the files the host writer lays out (read back through Pillow /
libtiff), and the readers' walk along the directory chain.  No comparison has a tolerance: the definition is exact."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pyramid_restatement as pr  # noqa: E402
import test_geotiff_open_host as host  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402
from deepbedmap_amd import geotiff  # noqa: E402

BOUND = host.BOUND
bits = host.bits
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (257, 513), (300, 520)]
NODATA = -2000


def test_overview_shapes():
    assert dbm.overview_shapes(1, 1, 0) == []
    assert dbm.overview_shapes(1, 2, 1) == [(1, 1)]
    assert dbm.overview_shapes(2, 1, 1) == [(1, 1)]
    assert dbm.overview_shapes(3, 5, 3) == [(2, 3), (1, 2), (1, 1)]
    assert dbm.overview_shapes(257, 513, 10) == [(129, 257), (65, 129), (33, 65), (17, 33), (9, 17), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1)]
    assert dbm.overview_shapes(300, 520, 4) == [(150, 260), (75, 130), (38, 65), (19, 33)]
    for H, W in SHAPES:
        assert len(dbm.overview_shapes(H, W, pr.max_levels(H, W))) == pr.max_levels(H, W)
        assert dbm.overview_shapes(H, W, 0) == []
    # "auto": down to the first level whose larger side is at most 256
    assert dbm.overview_shapes(18000, 22000, "auto") == [(9000, 11000), (4500, 5500), (2250, 2750), (1125, 1375), (563, 688), (282, 344),
                                                        (141, 172)]
    assert dbm.overview_shapes(300, 520, "auto") == [(150, 260), (75, 130)]
    assert dbm.overview_shapes(256, 256, "auto") == [] and dbm.overview_shapes(1, 257, "auto") == [(1, 129)]
    for bad in (-1, 1.5, "all", True, None):
        with pytest.raises(ValueError, match=r"overview_shapes: levels .* admits 10 levels"):
            dbm.overview_shapes(300, 520, bad)
    with pytest.raises(ValueError, match=r"overview_shapes: levels 11: an image of 300 x 520 admits 10 levels"):
        dbm.overview_shapes(300, 520, 11)
    with pytest.raises(ValueError, match=r"levels 1: an image of 1 x 1 admits 0 levels"):
        dbm.overview_shapes(1, 1, 1)


@pytest.fixture(scope="module")
def restated():
    """{(shape, dtype name): (plane, the restatement's levels down to 1 x 1, its window counts per n)}, computed once."""
    out = {}
    for shape in SHAPES:
        for dtype in (np.int16, np.float32):
            plane = pr.branch_plane(shape[0], shape[1], dtype, NODATA)
            levels, counts = pr.pyramid(plane, pr.max_levels(*shape), NODATA)
            out[shape, np.dtype(dtype).name] = (plane, levels, counts)
    return out


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_numpy_statement_equals_the_restatement(restated, shape, dtype):
    plane, want, counts = restated[shape, dtype]
    got = dbm.overview_pyramid(plane, len(want), NODATA)
    assert len(got) == len(want) == pr.max_levels(*shape)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == plane.dtype and g.shape == w.shape == dbm.overview_shapes(shape[0], shape[1], k + 1)[-1]
        assert np.array_equal(bits(g), bits(w)), (k, np.flatnonzero(bits(g) != bits(w))[:5])
    if shape[0] >= 257:   # every number of valid samples occurs, empty windows included
        assert all(c > 0 for c in counts), counts
    assert dbm.overview_pyramid(plane, 0, NODATA) == []


def test_the_branches_by_hand():
    """The listed cases one by one, against values worked out by hand (and the restatement)."""
    nd = NODATA
    # int16: ties after / 2 and / 4 in both signs go to even; / 3; the extremes; nodata as a value; an empty window
    a = np.array([[1, 2, -1, -2, 3, 4, -3, -4, 1, 1, 32767, 32767, nd, nd, 5, nd],
                  [nd, nd, nd, nd, nd, nd, nd, nd, 2, nd, 32767, 32767, nd, nd, nd, 8],
                  [1, 1, -1, -1, 2, 3, -2, -3, 1, 2, -32767, -32767, 7, nd, 0, 0],
                  [1, 3, -1, -3, 2, 3, -2, -3, 2, nd, -32767, -32767, nd, nd, 0, 0]], dtype=np.int16)
    want = np.array([[2, -2, 4, -4, 1, 32767, nd, 6], [2, -2, 2, -2, 2, -32767, 7, 0]], dtype=np.int16)   # 1.5 2.5 3.5 -> 2 2 4; 4/3, 5/3 -> 1, 2
    got = dbm.overview_pyramid(a, 1, nd)[0]
    assert np.array_equal(got, want) and np.array_equal(pr.pyramid(a, 1, nd)[0][0], want)
    # float32: NaN and nodata do not count, -0.0 survives alone and is lost beside +0.0 (the invalid samples' +0.0 included)
    f = np.array([[-0.0, -0.0, -0.0, nd, np.nan, np.nan, 1.5, np.nan, nd, nd],
                  [-0.0, -0.0, nd, nd, np.nan, np.nan, nd, 2.0, nd, np.nan]], dtype=np.float32)
    got = dbm.overview_pyramid(f, 1, nd)[0]
    want = np.array([[-0.0, 0.0, nd, 1.75, nd]], dtype=np.float32)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(pr.pyramid(f, 1, nd)[0][0]), bits(want))
    # a mean that equals the nodata value is nodata for the next level (level k + 1 is made from level k alone)
    g = np.array([[nd - 1, nd + 1, 10, 10]], dtype=np.float32)
    levels = dbm.overview_pyramid(g, 2, nd)
    assert levels[0].tolist() == [[nd, 10]] and levels[1].tolist() == [[10]]
    # all nodata; NaN as the nodata value
    assert np.array_equal(dbm.overview_pyramid(np.full((5, 7), nd, np.int16), 3, nd)[2], np.full((1, 1), nd, np.int16))
    h = np.array([[np.nan, np.nan, 1, np.nan]], dtype=np.float32)
    assert np.array_equal(bits(dbm.overview_pyramid(h, 1, np.nan)[0]), bits(np.array([[np.nan, 1]], dtype=np.float32)))
    with pytest.raises(ValueError, match="overview_pyramid: levels 3"):
        dbm.overview_pyramid(g, 3, nd)
    with pytest.raises(ValueError, match="int16 or float32"):
        dbm.overview_pyramid(g.astype(np.float64), 1, nd)


def test_build_overviews_of_a_numpy_array(restated):
    plane, want, _ = restated[(300, 520), "int16"]
    got = dbm.build_overviews(plane.astype(np.float32)[None], 4, dtype=np.int16, nodataval=NODATA)
    assert len(got) == 4 and all(np.array_equal(g, w) and g.dtype == np.int16 for g, w in zip(got, want))
    f = pr.branch_plane(3, 5, np.float32, NODATA)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(dbm.build_overviews(f, 3), pr.pyramid(f, 3, NODATA)[0]))


def _frames(path):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(path)
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append((np.array(im), dict(im.tag_v2)))
    return out


@pytest.mark.parametrize("bigtiff", [False, True])
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("compression", ["lzw", "none"])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_the_file_through_libtiff(tmp_path, restated, dtype, tiled, compression, predictor, bigtiff):
    """Tiled at 300 x 520; strips at 520 x 300, whose level 1 has 260 rows: a strip of 256 and a short one of 4."""
    plane, want, _ = restated[(300, 520), dtype]
    if not tiled:   # level 1 of 520 x 300 has 260 rows: a whole strip and a short one of 4 rows
        plane = np.ascontiguousarray(plane.T)
        want = dbm.overview_pyramid(plane, 3, NODATA)
    levels = 3
    path = dbm.save_array_to_grid(str(tmp_path / "o"), BOUND, plane[None], tiled=tiled, compression=compression, predictor=predictor,
                                  bigtiff=bigtiff, nodataval=NODATA, overviews=levels)
    frames = _frames(path)
    assert len(frames) == levels + 1
    assert 254 not in frames[0][1] and np.array_equal(bits(frames[0][0].astype(dtype)), bits(plane))
    for k in range(1, levels + 1):
        pixels, tags = frames[k]
        assert tags[254] == 1 and pixels.shape == want[k - 1].shape
        assert np.array_equal(bits(pixels.astype(dtype)), bits(want[k - 1]))
        assert not any(t in tags for t in (33550, 33922, 34735, 34264)) and tags[42113].rstrip("\0") == str(NODATA)
        assert tags[259] == (5 if compression == "lzw" else 1) and (tags.get(317, 1) == (predictor if compression == "lzw" else 1))
        gf = geotiff.open_geotiff(path, k)
        assert gf.tiled == tiled and (gf.block_h, gf.block_w) == ((256, 256) if tiled else (min(256, pixels.shape[0]), pixels.shape[1]))
    if not tiled:
        assert geotiff.open_geotiff(path, 1).plan().blocks[:, 2].tolist() == [256, 4]
    # the layout: the streams of level 0, then level 1, ..., at even offsets, then the directories (the chain ends after the last level)
    with open(path, "rb") as f:
        _, directories = geotiff._read_tags(f, path)
        head = f.seek(0) or f.read(16)
    assert len(directories) == levels + 1
    first_ifd = struct.unpack_from("<Q", head, 8)[0] if bigtiff else struct.unpack_from("<I", head, 4)[0]
    offsets = [int(o) for k in range(levels + 1) for o in geotiff.open_geotiff(path, k).offsets]
    assert offsets == sorted(offsets) and offsets[-1] < first_ifd and first_ifd % 2 == 0 and all(o % 2 == 0 for o in offsets)


@pytest.mark.parametrize("kw", [dict(), dict(tiled=True, compression="lzw", predictor=2, dtype=np.int16), dict(bigtiff=False, compression="lzw")])
def test_no_overviews_is_todays_file(tmp_path, restated, kw):
    plane = restated[(300, 520), "float32"][0]
    a = dbm.save_array_to_grid(str(tmp_path / "a"), BOUND, plane[None], **kw)
    b = dbm.save_array_to_grid(str(tmp_path / "b"), BOUND, plane[None], overviews=0, **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    for bad in (-1, 11, "all", 2.0):
        with pytest.raises(ValueError, match="save_array_to_grid: overviews .* admits 10 levels"):
            dbm.save_array_to_grid(str(tmp_path / "c"), BOUND, plane[None], overviews=bad, **kw)
    with pytest.raises(ValueError, match="write_geotiff_resident: array must be"):   # (argument errors need no device)
        dbm.write_geotiff_resident(str(tmp_path / "c"), BOUND, plane[None], overviews=1)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("tiled", [True, False])
def test_every_level_comes_back_through_the_readers(tmp_path, restated, dtype, tiled):
    plane, want, _ = restated[(300, 520), dtype]
    path = dbm.save_array_to_grid(str(tmp_path / "r"), BOUND, plane[None], tiled=tiled, compression="lzw", predictor=2, nodataval=NODATA,
                                  overviews="auto")
    base = geotiff.open_geotiff(path)
    assert base.overview_count == 2 and base.overview == 0 and base.shape == (300, 520)
    assert np.array_equal(bits(host.host_decode(path)), bits(plane))
    g0 = base.geometry
    for k in (1, 2):
        gf = geotiff.open_geotiff(path, overview=k)
        assert gf.overview == k and gf.overview_count == 2 and gf.shape == want[k - 1].shape and gf.nodata == str(NODATA)
        assert gf.geokeys == base.geokeys and gf.dtype == np.dtype(dtype)
        assert np.array_equal(bits(_decode(gf)), bits(want[k - 1]))
        back, info = dbm.read_geotiff(path, overview=k)
        assert np.array_equal(bits(back[0]), bits(want[k - 1])) and info["nodata"] == str(NODATA)
        # the geometry: the outer pixel-edge box divided into W_k x H_k pixels, in float64 and in this order
        H, W = gf.shape
        dx, dy = g0.dx * 520 / W, g0.dy * 300 / H
        assert gf.geometry == dbm.GridGeometry(x0=(g0.x0 - g0.dx / 2) + dx / 2, y0=(g0.y0 - g0.dy / 2) + dy / 2, dx=dx, dy=dy, registration="pixel")
    assert geotiff.open_geotiff(path, 1).geometry == dbm.GridGeometry.from_bounds(BOUND, 150, 260)   # (exact at these sizes)
    # a windowed plan on level 1 (pixels of 200 m): rows 5..14, columns 100..139
    minx, _, _, maxy = BOUND
    gf = geotiff.open_geotiff(path, 1)
    bound = (minx + 20000, maxy - 3000, minx + 28000, maxy - 1000)
    assert gf.window(bound) == (5, 100, 10, 40)
    assert np.array_equal(bits(_decode(gf, bound)), bits(want[0][5:15, 100:140]))
    with pytest.raises(ValueError, match=r"overview 3 asked for, the file holds 2"):
        geotiff.open_geotiff(path, 3)
    with pytest.raises(ValueError, match=r"overview 3 asked for, the file holds 2"):
        dbm.read_geotiff(path, overview=3)
    for bad in (-1, 1.0, "1"):
        with pytest.raises(ValueError, match="open_geotiff: overview"):
            geotiff.open_geotiff(path, bad)


def _decode(gf, window_bound=None):
    """host.host_decode for an opened image (an overview too): the blocks of its plan, decoded on the host."""
    plan = gf.plan(window_bound)
    r0, c0, H, W = plan.window
    out = np.zeros((H, W), dtype=gf.dtype)
    buf = open(gf.path, "rb").read()
    for off, cnt, rows, orow, ocol, _ in plan.blocks:
        want = rows * gf.block_w * gf.dtype.itemsize
        s = buf[off:off + cnt]
        raw = geotiff.lzw_decode(s, want) if gf.compression == 5 else np.frombuffer(zlib.decompress(s) if gf.compression != 1 else s, dtype=np.uint8)[:want]
        block = host.undo_predictor(np.asarray(raw).reshape(rows, -1), gf.dtype, gf.predictor)
        ra, rb = max(orow, 0), min(orow + rows, H)
        ca, cb = max(ocol, 0), min(ocol + gf.block_w, W)
        out[ra:rb, ca:cb] = block[ra - orow:rb - orow, ca - ocol:cb - ocol]
    return out


def _foreign(path, images, loop=False):
    """A classic little-endian TIFF built by hand: images = [(extra tags {tag: (type, values)}, compression, int16 array)], one strip
    each, the directories chained in order (loop: the last one points back to the first)."""
    body = bytearray(b"II*\0\0\0\0\0")
    strips = []
    for _, comp, a in images:
        raw = np.ascontiguousarray(a, dtype="<i2").tobytes()
        s = {1: raw, 8: zlib.compress(raw), 5: None}[comp]
        if s is None:
            s = geotiff.lzw_encode_tiles(np.frombuffer(raw, dtype=np.uint8)[None], 1)[0]
        strips.append((len(body), len(s)))
        body += s + b"\0" * (len(s) % 2)
    first = len(body)
    for k, (extra, comp, a) in enumerate(images):
        tags = {256: (4, [a.shape[1]]), 257: (4, [a.shape[0]]), 258: (3, [16]), 259: (3, [comp]), 262: (3, [1]), 273: (4, [strips[k][0]]),
                277: (3, [1]), 278: (4, [a.shape[0]]), 279: (4, [strips[k][1]]), 339: (3, [2])}
        tags.update(extra)
        entries, extra_bytes = b"", b""
        at = len(body) + 2 + 12 * len(tags) + 4
        for tag in sorted(tags):
            typ, vals = tags[tag]
            data = vals if typ == 2 else struct.pack("<%d%s" % (len(vals), {3: "H", 4: "I", 12: "d"}[typ]), *vals)
            count = len(data) if typ == 2 else len(vals)
            if len(data) <= 4:
                field = data + b"\0" * (4 - len(data))
            else:
                field = struct.pack("<I", at + len(extra_bytes))
                extra_bytes += data + b"\0" * (len(data) % 2)
            entries += struct.pack("<HHI", tag, typ, count) + field
        nxt = at + len(extra_bytes) if k + 1 < len(images) else (first if loop else 0)
        body += struct.pack("<H", len(tags)) + entries + struct.pack("<I", nxt) + extra_bytes
    struct.pack_into("<I", body, 4, first)
    open(path, "wb").write(bytes(body))
    return str(path)


def test_a_foreign_file(tmp_path):
    """Overviews compressed differently from the base, without a nodata tag, behind a mask directory (254 = 4) that is no overview --
    nor is the reduced-resolution mask (254 = 5) at the end."""
    rng = np.random.default_rng(3)
    base = rng.integers(-500, 500, (40, 60)).astype(np.int16)
    ov1, ov2 = dbm.overview_pyramid(base, 2, -9999)
    mask = np.ones((40, 60), dtype=np.int16)
    georef = {33550: (12, [100.0, 100.0, 0.0]), 33922: (12, [0.0, 0.0, 0.0, -1000.0, 32000.0, 0.0]), 42113: (2, b"-9999\0")}
    path = _foreign(tmp_path / "foreign.tif", [(georef, 1, base), ({254: (4, [4])}, 8, mask), ({254: (4, [1])}, 8, ov1),
                                               ({254: (4, [1])}, 5, ov2), ({254: (4, [5])}, 1, mask[:10, :15])])
    gf = geotiff.open_geotiff(path)
    assert gf.overview_count == 2 and gf.compression == 1 and np.array_equal(_decode(gf), base)
    one, two = geotiff.open_geotiff(path, 1), geotiff.open_geotiff(path, 2)
    assert (one.compression, two.compression) == (8, 5) and one.nodata == two.nodata == "-9999" and 42113 not in one.tags
    assert np.array_equal(_decode(one), ov1) and np.array_equal(_decode(two), ov2)
    assert one.geometry == dbm.GridGeometry(x0=-900.0, y0=31900.0, dx=200.0, dy=-200.0, registration="pixel")
    assert np.array_equal(dbm.read_geotiff(path, overview=2)[0][0], ov2)
    with pytest.raises(ValueError, match="overview 3 asked for, the file holds 2"):
        geotiff.open_geotiff(path, 3)
    # an overview goes through the checks of a first directory
    bad = _foreign(tmp_path / "bad.tif", [(georef, 1, base), ({254: (4, [1]), 277: (3, [3])}, 1, ov1)])
    assert geotiff.open_geotiff(bad).overview_count == 1
    with pytest.raises(ValueError, match=r"SamplesPerPixel \(277\) = 3"):
        geotiff.open_geotiff(bad, 1)
    # a chain that loops, and one that leaves the file
    loop = _foreign(tmp_path / "loop.tif", [(georef, 1, base), ({254: (4, [1])}, 1, ov1)], loop=True)
    first = struct.unpack_from("<I", open(loop, "rb").read(), 4)[0]
    with pytest.raises(ValueError, match=rf"at offset {first}: the chain of image directories comes back"):
        geotiff.open_geotiff(loop)
    buf = bytearray(open(path, "rb").read())
    first = struct.unpack_from("<I", buf, 4)[0]
    n = struct.unpack_from("<H", buf, first)[0]
    struct.pack_into("<I", buf, first + 2 + 12 * n, len(buf) + 100)
    (tmp_path / "out.tif").write_bytes(bytes(buf))
    with pytest.raises(ValueError, match=rf"IFD 1 at offset {len(buf) + 100} .* lies outside the file"):
        geotiff.open_geotiff(tmp_path / "out.tif")
