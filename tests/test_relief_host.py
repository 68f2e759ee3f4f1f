"""Host side of DESIGN.md 6n (colour relief, hillshade, PNG): colour tables, the NumPy statement of the pixel rule, the PNG container and
the host writer (dbm_png_encode_host: the device encoder's own loop with one lane, framing 1 / 2), against the independent restatements
of tests/relief_restatement.py and against zlib and PIL as referees.  No GPU."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import relief_restatement as rr  # noqa: E402

from deepbedmap_amd import _lib, relief  # noqa: E402
from deepbedmap_amd.resident import GridGeometry  # noqa: E402


@pytest.fixture(scope="module")
def oleron():
    return relief.read_cpt(rr.GOLDEN_CPT)


def package_tables(oleron):
    """The tables of rr.tables(), made by the package."""
    we, wc = rr.wide_master()
    wide = relief.ColorTable(we, np.concatenate([np.array(wc, dtype=np.uint8).ravel(), np.array([1, 2, 3, 250, 251, 252, 9, 8, 7], dtype=np.uint8)]))
    return {"oleron": relief.make_cpt(oleron, (-4500, 4500)),
            "hinge": relief.make_cpt(oleron, (-2000, 4500), hinge=0),
            "bands": relief.make_cpt(oleron, (-2800, 2800, 200), overrule_bg=True),
            "one": relief.make_cpt(relief.grey_cpt(), (-4500, 4500)),
            "wide": relief.make_cpt(wide, (-4500, 4500))}


def same_table(table, want):
    edges, colours, B, F, N = want[:5]
    assert table.n == len(colours)
    assert table.edges.tobytes() == np.array(edges, dtype=np.float64).tobytes()   # bit for bit
    assert np.array_equal(table.slices, np.array(colours, dtype=np.uint8))
    assert list(table.background) == list(B) and list(table.foreground) == list(F) and list(table.nan) == list(N)


def test_read_cpt_reads_the_reference_table(oleron):
    assert oleron.n == 256 and oleron.edges[0] == -1.0 and oleron.edges[-1] == 1.0 and oleron.hinge == 0.0
    assert list(oleron.background) == [26, 38, 89] and list(oleron.foreground) == [253, 253, 230] and list(oleron.nan) == [255, 255, 255]
    e, c, B, F, N, h = rr.parse_cpt(rr.GOLDEN_CPT)
    same_table(oleron, (e, c, B, F, N))
    assert not oleron.edges.flags.writeable and not oleron.colors.flags.writeable
    with pytest.raises(dataclasses_error()):
        oleron.hinge = 1.0


def dataclasses_error():
    import dataclasses

    return dataclasses.FrozenInstanceError


@pytest.mark.parametrize("name", ["oleron", "hinge", "bands", "one", "wide"])
def test_make_cpt_equals_the_restatement(oleron, name):
    table = package_tables(oleron)[name]
    same_table(table, rr.tables()[name])
    if name == "oleron":
        assert table.edges[0] == -4500.0 and table.edges[-1] == 4500.0
    if name == "hinge":
        assert table.edges[128] == 0.0 and oleron.edges[128] == 0.0 and table.edges[0] == -2000.0 and table.edges[-1] == 4500.0
    if name == "bands":
        assert table.n == 28 and np.array_equal(table.slices[:, 0], table.slices[:, 1])
        assert np.array_equal(table.edges, np.arange(-2800.0, 2801.0, 200.0))
        assert list(table.background) == list(table.slices[0, 0]) and list(table.foreground) == list(table.slices[-1, 1])
    if name == "one":
        assert table.n == 1
    if name == "wide":
        assert table.n == 2048


def test_defaults_of_absent_colours(tmp_path):
    p = tmp_path / "t.cpt"
    p.write_text("0 10/20/30 1 40/50/60 L\n1 40/50/60 3 70/80/90 ;label\n")
    t = relief.read_cpt(p)
    assert t.n == 2 and t.hinge is None and list(t.edges) == [0.0, 1.0, 3.0]
    assert list(t.background) == [0, 0, 0] and list(t.foreground) == [255, 255, 255] and list(t.nan) == [128, 128, 128]
    o = relief.make_cpt(t, (0, 30), overrule_bg=True)
    assert list(o.background) == [10, 20, 30] and list(o.foreground) == [70, 80, 90] and list(o.nan) == [128, 128, 128]


@pytest.mark.parametrize("text,line,match", [
    ("# COLOR_MODEL = HSV\n0 10/20/30 1 40/50/60\n", 1, "COLOR_MODEL"),
    ("0 10/20/30 1 40/50/60\n1 red 2 blue\n", 2, "triplets"),
    ("0 10/20/30 1 40/50/60\n1.5 40/50/60 2 70/80/90\n", 2, "gap or an overlap"),
    ("0 10/20/30 1 40/50/60\n0.5 40/50/60 2 70/80/90\n", 2, "gap or an overlap"),
    ("0 10/20/30 1 40/50/60\n1 40/50/60 1 70/80/90\n", 2, "ascend"),
    ("0 10/20/30 1 40/50/60\n1 40/50/60 0.5 70/80/90\n", 2, "ascend"),
    ("0 10/20/30 1 40/50/300\n", 1, "triplets"),
    ("0 10/20/30 1\n", 1, "z0 r/g/b z1 r/g/b"),
    ("0 10/20/30 1 40/50/60\nB black\n", 2, "triplets"),
])
def test_read_cpt_refusals_name_the_line(tmp_path, text, line, match):
    p = tmp_path / "bad.cpt"
    p.write_text(text)
    with pytest.raises(ValueError, match=match) as e:
        relief.read_cpt(p)
    assert f"bad.cpt:{line}" in str(e.value)


def test_make_cpt_refusals(oleron):
    for kw, match in [(dict(series=(1, 1)), "lo must be below hi"), (dict(series=(0, 1, 2, 3)), "series"), (dict(series=(0, np.inf)), "series"),
                      (dict(series=(-1, 1), hinge=1), "hinge"), (dict(series=(-1, 1), hinge=-2), "hinge"),
                      (dict(series=(0, 1, 0.3)), "integer"), (dict(series=(0, 1, -0.5)), "integer"), (dict(series=(0, 2049, 1)), "2048"),
                      (dict(series=(0, 1e-322)), "ascend")]:
        with pytest.raises(ValueError, match=match):
            relief.make_cpt(oleron, **kw)
    with pytest.raises(ValueError, match="hinge"):
        relief.make_cpt(relief.grey_cpt(), (-1, 1), hinge=0)   # (no inner edge at 0)
    with pytest.raises(ValueError, match="ColorTable"):
        relief.make_cpt("oleron", (-1, 1))
    assert relief.make_cpt(oleron, (0, 2048, 1)).n == 2048
    with pytest.raises(ValueError, match="2048"):
        relief.ColorTable(np.arange(2050.0), np.zeros(6 * 2049 + 9, dtype=np.uint8))
    assert relief.ColorTable(np.arange(2049.0), np.zeros(6 * 2048 + 9, dtype=np.uint8)).n == 2048
    with pytest.raises(ValueError, match="ascending"):
        relief.ColorTable([0.0, 1.0, 1.0], np.zeros(21, dtype=np.uint8))


@pytest.mark.parametrize("n1,n2", [(0, 0), (0, 1), (1, 0), (1, 1), (65520, 65521), (65521, 65520), (65521, 65521), (200000, 1), (1, 200000),
                                   (200000, 200000), (5552, 5553)])
def test_adler32_combine(n1, n2):
    rng = np.random.default_rng(n1 * 7 + n2)
    for fill in (None, 255):
        a = (rng.integers(0, 256, n1, dtype=np.uint8) if fill is None else np.full(n1, fill, dtype=np.uint8)).tobytes()
        b = (rng.integers(0, 256, n2, dtype=np.uint8) if fill is None else np.full(n2, fill, dtype=np.uint8)).tobytes()
        want = zlib.adler32(a + b)
        assert relief.adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == want
        assert rr.adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == want


def images():
    rng = np.random.default_rng(5)
    t = rr.tables()["oleron"]
    rendered = rr.reference("oleron", (37, 29))[0]
    return {"relief": rendered, "constant": np.full((37, 29, 4), 77, dtype=np.uint8), "noise": rng.integers(0, 256, (37, 29, 4), dtype=np.uint8),
            "tiny": rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), "rgb": rng.integers(0, 4, (3, 5, 3), dtype=np.uint8),
            "grey": (np.add.outer(np.arange(40), np.arange(33)) % 7).astype(np.uint8).reshape(40, 33, 1),
            "window": np.repeat(rng.integers(0, 3, (96, 50, 4), dtype=np.uint8), 4, axis=1)}


def host_segments(image, filter, band_rows, first=0, count=None, nthreads=3):
    H, W, ch = image.shape
    bands = -(-H // band_rows)
    count = bands - first if count is None else count
    worst = (relief.deflate_slot(min(band_rows, H) * (W * ch + 1)) + 1) & ~1
    out = np.zeros(max(count, 1) * worst, dtype=np.uint8)
    sizes = np.zeros(max(count, 1), dtype=np.uintp)
    adlers = np.zeros(max(count, 1), dtype=np.uint32)
    image = np.ascontiguousarray(image)
    rc = _lib.lib().dbm_png_encode_host(image.ctypes.data_as(C.c_void_p), H, W, ch, filter, band_rows, first, count, out.ctypes.data_as(C.c_void_p),
                                        out.size, sizes.ctypes.data_as(C.c_void_p), adlers.ctypes.data_as(C.c_void_p), nthreads)
    assert rc == 0, _lib.lib().dbm_last_error(None)
    segs, pos = [], 0
    for k in range(count):
        segs.append(out[pos:pos + int(sizes[k])].tobytes())
        pos += (int(sizes[k]) + 1) & ~1
    return segs, [int(a) for a in adlers[:count]]


@pytest.mark.parametrize("filter", [0, 1, 2])
@pytest.mark.parametrize("name,band_rows", [("relief", 5), ("relief", 1), ("relief", 37), ("constant", 5), ("noise", 5), ("tiny", 1), ("rgb", 2),
                                            ("grey", 7), ("window", 96)])
def test_segments_make_one_zlib_stream_of_the_filtered_scanlines(name, band_rows, filter):
    image = images()[name]
    H, W, ch = image.shape
    lines = rr.filtered_scanlines(image, filter)
    segs, adlers = host_segments(image, filter, band_rows)
    assert len(segs) == -(-H // band_rows)
    adler = 1
    for b, seg in enumerate(segs):
        band = lines[b * band_rows:(b + 1) * band_rows].tobytes()
        assert adlers[b] == zlib.adler32(band)
        adler = rr.adler32_combine(adler, adlers[b], len(band))
        assert len(seg) <= relief.deflate_slot(len(band))
        if b < len(segs) - 1:
            assert seg[-4:] == b"\x00\x00\xff\xff" and seg[0] & 7 == 0b010          # BFINAL 0, BTYPE 01; the empty stored block
            assert zlib.decompressobj(-15).decompress(seg) == band                    # a segment stands alone: no reference in front of it
        else:
            assert seg[0] & 7 == 0b011                                               # BFINAL 1, BTYPE 01
    assert adler == zlib.adler32(lines.tobytes())
    stream = b"\x78\x01" + b"".join(segs) + struct.pack(">I", adler)
    assert zlib.decompress(stream) == lines.tobytes()
    # a range of bands is the same bytes as those bands of the whole
    if len(segs) >= 3:
        part, part_adlers = host_segments(image, filter, band_rows, first=1, count=len(segs) - 1, nthreads=1)
        assert part == segs[1:] and part_adlers == adlers[1:]


def test_framing_zero_is_unchanged_and_the_noise_band_outgrows_its_input():
    """dbm_deflate_encode_blocks (framing 0) still writes 78 01 ... Adler-32; a band of uniform noise grows, within the slot."""
    rng = np.random.default_rng(3)
    block = rng.integers(0, 256, 4000, dtype=np.uint8)
    out = np.zeros(relief.deflate_slot(block.size), dtype=np.uint8)
    size = C.c_size_t(0)
    assert _lib.lib().dbm_deflate_encode_blocks(block.ctypes.data_as(C.c_void_p), block.size, 1, out.ctypes.data_as(C.c_void_p), out.size,
                                                C.byref(size), 1) == 0
    stream = out[:size.value].tobytes()
    assert stream[:2] == b"\x78\x01" and stream[2] & 7 == 0b011 and stream[-4:] == struct.pack(">I", zlib.adler32(block.tobytes()))
    assert zlib.decompress(stream) == block.tobytes()
    noise = images()["noise"]
    segs, _ = host_segments(noise, 0, 37)
    assert len(segs[0]) > 37 * (29 * 4 + 1)


def test_host_entry_refusals():
    lib = _lib.lib()
    image = np.zeros((4, 4, 4), dtype=np.uint8)
    out, sizes, adlers = np.zeros(4096, dtype=np.uint8), np.zeros(4, dtype=np.uintp), np.zeros(4, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(H=4, W=4, ch=4, filter=1, rows=2, first=0, n=2, cap=4096, img=image):
        return lib.dbm_png_encode_host(p(img) if img is not None else None, H, W, ch, filter, rows, first, n, p(out), cap, p(sizes), p(adlers), 1)

    assert call() == 0
    for kw in (dict(img=None), dict(H=0), dict(ch=2), dict(filter=3), dict(filter=-1), dict(rows=0), dict(first=1, n=2), dict(n=-1), dict(cap=10)):
        assert call(**kw) == 1, kw
        assert b"dbm_png_encode_host" in lib.dbm_last_error(None)
    assert call(n=0) == 0


@pytest.mark.parametrize("filter", [0, 1, 2])
@pytest.mark.parametrize("name,band_rows", [("relief", 5), ("relief", None), ("noise", 1), ("tiny", None), ("rgb", 2), ("grey", 7), ("window", 96)])
def test_save_png_files_decode_to_the_image(tmp_path, name, band_rows, filter):
    image = images()[name]
    path = relief.save_png(str(tmp_path / "a.png"), image, filter=filter, band_rows=band_rows, idat_bytes=1000)
    back = relief.read_png(path)
    assert np.array_equal(back.reshape(image.shape), image)
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n" and blob[12:16] == b"IHDR" and blob[-8:-4] == b"IEND"
    assert struct.unpack(">IIBBBBB", blob[16:29]) == (image.shape[1], image.shape[0], 8, {1: 0, 3: 2, 4: 6}[image.shape[2]], 0, 0, 0)
    assert relief.save_png(str(tmp_path / "b.png"), image, filter=filter, band_rows=band_rows) == str(tmp_path / "b.png")
    assert np.array_equal(relief.read_png(str(tmp_path / "b.png")).reshape(image.shape), image)   # (one IDAT chunk)


@pytest.mark.parametrize("filter", [0, 1, 2])
def test_pil_reads_the_files(tmp_path, filter):
    Image = pytest.importorskip("PIL.Image")
    for name, image in images().items():
        path = relief.save_png(str(tmp_path / f"{name}.png"), image if image.shape[2] > 1 else image[:, :, 0], filter=filter, band_rows=5,
                               idat_bytes=777)
        with Image.open(path) as im:
            assert np.array_equal(np.asarray(im).reshape(image.shape), image), name
        # the container of the restatement: bands deflated by zlib itself, stitched the same way
        stitched = tmp_path / f"{name}_zlib.png"
        stitched.write_bytes(rr.stitched_png(image, filter, 5, idat_bytes=777))
        with Image.open(stitched) as im:
            assert np.array_equal(np.asarray(im).reshape(image.shape), image), name
        assert np.array_equal(relief.read_png(stitched).reshape(image.shape), image)


def test_read_png_checks_what_it_reads(tmp_path):
    path = relief.save_png(str(tmp_path / "a.png"), images()["relief"])
    blob = bytearray(open(path, "rb").read())
    blob[40] ^= 1
    (tmp_path / "bad.png").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="CRC-32"):
        relief.read_png(tmp_path / "bad.png")
    (tmp_path / "short.png").write_bytes(bytes(blob[:30]))
    with pytest.raises(ValueError, match="truncated"):
        relief.read_png(tmp_path / "short.png")
    with pytest.raises(ValueError, match="uint8"):
        relief.save_png(str(tmp_path / "f.png"), np.zeros((2, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="filter"):
        relief.save_png(str(tmp_path / "f.png"), np.zeros((2, 2), dtype=np.uint8), filter=4)
    with pytest.raises(ValueError, match="band_rows"):
        relief.save_png(str(tmp_path / "f.png"), np.zeros((2, 2), dtype=np.uint8), band_rows=0)


def test_world_file(tmp_path):
    geometry = GridGeometry(x0=-2700125.0, y0=2299875.0, dx=250.0, dy=-250.0, registration="pixel")
    path = relief.save_png(str(tmp_path / "dem.png"), images()["rgb"], world_file=geometry)
    lines = open(os.path.splitext(path)[0] + ".pgw").read().split("\n")
    assert lines[6:] == [""] and [float(v) for v in lines[:6]] == [250.0, 0.0, 0.0, -250.0, -2700125.0, 2299875.0]
    reduced = relief.reduced_geometry(geometry, 2)
    assert (reduced.dx, reduced.dy, reduced.x0, reduced.y0) == (1000.0, -1000.0, -2700125.0 + 375.0, 2299875.0 - 375.0)
    assert relief.default_band_rows(22000, 4) == 1 and relief.default_band_rows(5500, 4) == 5 and relief.default_band_rows(29, 4) == 1120


@pytest.mark.parametrize("shape", rr.SHAPES)
@pytest.mark.parametrize("name", ["oleron", "hinge", "bands", "one", "wide"])
def test_relief_image_host_equals_the_restatement(oleron, name, shape):
    table = package_tables(oleron)[name]
    z = rr.plane_of(name, shape)
    want, _ = rr.reference(name, shape)
    for channels in (3, 4):
        assert np.array_equal(relief.relief_image_host(z, table, channels=channels), want[:, :, :channels])
    g, ok = rr.gradient_of(name, shape)
    n, mean, sigma = rr.stats(g, ok)
    sin_a, cos_a, k = rr.shading_constants()
    assert relief.shading_parameters("+d") == (sin_a, cos_a, k) == relief.shading_parameters(rr.SHADING)
    hg, hok = relief.gradient_host(z, sin_a, cos_a, 1.0)
    assert np.array_equal(hok, ok) and np.array_equal(hg[ok], g[ok])
    hn, hmean, hsigma = relief.shade_stats_host(hg, hok)
    assert hn == n and abs(hmean - mean) <= n * 2.0 ** -52 * max(np.abs(g[ok]).mean() if n else 0.0, 0.0)
    assert abs(hsigma - sigma) <= 2 * n * 2.0 ** -52 * sigma
    if n < 2 or sigma == 0:   # (1, 1), (1, 7), (7, 1): g is undefined everywhere, the intensity is 0
        assert n == 0 and np.array_equal(relief.relief_image_host(z, table, shading="+d"), want)
        return
    want, pre = rr.reference(name, shape, (mean, sigma))
    # the inputs the GPU test uses satisfy its exclusion cap by the restatement alone: no byte within 1e-9 of a tie
    assert rr.near_tie(pre).sum() == 0
    for channels in (3, 4):
        got = relief.relief_image_host(z, table, shading=rr.SHADING, channels=channels, stats=(n, mean, sigma))
        assert np.array_equal(got, want[:, :, :channels])
    assert not np.array_equal(want, rr.reference(name, shape)[0])   # (the shading changes the picture)


def test_the_planes_hold_what_the_rule_branches_on():
    for name, t in rr.tables().items():
        z = rr.plane_of(name, (150, 210))
        lo, hi = t[5], t[6]
        assert np.isnan(z).sum() == 20 and np.isposinf(z).sum() == 1 and np.isneginf(z).sum() == 1
        finite = z[np.isfinite(z)]
        assert (finite == lo).any() and (finite == hi).any() and (finite == 0).any() and (finite < lo).any() and (finite > hi).any()
        if t[7] is not None:
            assert (finite == np.float32(t[7])).any()
    assert rr.tables()["bands"][0][17] == 600.0 and rr.tables()["wide"][0][512] == -2250.0 and rr.tables()["hinge"][0][128] == 0.0


def test_relief_host_refusals(oleron):
    z = np.zeros((3, 3), dtype=np.float32)
    for kw, match in [(dict(channels=2), "channels"), (dict(shading="+x"), "shading"), (dict(shading=(0, 2)), "amplitude"),
                      (dict(aspect=np.inf), "aspect"), (dict(cpt="oleron"), "ColorTable")]:
        args = dict(cpt=oleron)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            relief.relief_image_host(z, **args)
    with pytest.raises(ValueError, match="not empty"):
        relief.relief_image_host(np.zeros((0, 3), dtype=np.float32), oleron)


def test_the_header_and_the_bindings_name_the_new_entry_points():
    text = open(os.path.join(os.path.dirname(HERE), "include", "dbm.h")).read()
    for name in ("dbm_grid_relief", "dbm_grid_shade_stats", "dbm_png_encode", "dbm_png_encode_host"):
        i = text.index("int " + name + "(")
        assert "deepbedmap.py:758-775" in text[max(0, i - 8000):i] and "paper_figures.py:692-699" in text[max(0, i - 8000):i], name
        assert name in _lib.SIGNATURES
    import deepbedmap_amd as dbm

    for name in ("ColorTable", "read_cpt", "make_cpt", "grey_cpt", "relief_image", "relief_image_host", "render_dem", "save_png",
                 "write_png_resident", "read_png", "adler32_combine"):
        assert hasattr(dbm, name), name
