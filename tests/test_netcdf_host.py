"""`deepbedmap_amd.netcdf` on the host (no GPU): `open_netcdf` against the manifest libhdf5's generator wrote, `read_netcdf` against
the values libhdf5 read back (tests/golden/netcdf/expected/*.npy, made by tests/golden/make_netcdf_fixtures.py) taken through the NumPy
restatement of the value rule, bit for bit; classic files written here by scipy; geometry; every refusal by its name."""
import json
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import netcdf_restatement as rs  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "netcdf")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
READABLE = [(e["file"], e["variable"]) for e in MANIFEST if len(e["shape"]) == 2]
FLIPPED = {"gmt_z.nc"}

# The contraction sample (found by construction on the CPU, checked below with exact rational arithmetic): v * scale rounds DOWN to
# float64 by 3616 * 2^-52, and the offset puts the rounded product exactly on the midpoint 4 + 2^-22 of two float32 neighbours.
# Rounded twice (NumPy, this project's rule) the sum is the tie and goes to the even neighbour 4.0; fused, the sum lies above the
# midpoint and goes to 4.0000005.
CONTRACTION_V = 20000
CONTRACTION_SCALE = float.fromhex("0x1.0000000000001p+0")
CONTRACTION_OFFSET = float.fromhex("-0x1.386ffffff0001p+14")
CONTRACTION_TWO_ROUNDINGS = np.uint32(0x40800000)   # 4.0
CONTRACTION_FUSED = np.uint32(0x40800001)           # 4.0000005


@pytest.fixture(scope="module")
def nc():
    from deepbedmap_amd import netcdf

    return netcdf


def entry(file, variable):
    return next(e for e in MANIFEST if e["file"] == file and e["variable"] == variable)


def stored(file, variable):
    return np.load(os.path.join(GOLDEN, "expected", f"{file[:-3]}.{variable}.npy"))


def rule_of(e):
    a = e["attrs"]
    return a.get("_FillValue", a.get("missing_value")), a.get("scale_factor"), a.get("add_offset")


def test_fixture_sizes():
    total = 0
    for d, _, names in os.walk(GOLDEN):
        for n in names:
            size = os.path.getsize(os.path.join(d, n))
            assert size < 64 * 1024, n
            total += size
    assert total < 300 * 1024


@pytest.mark.parametrize("file,variable", READABLE)
def test_open_agrees_with_the_manifest(nc, file, variable):
    e = entry(file, variable)
    v = nc.open_netcdf(os.path.join(GOLDEN, file), variable)
    assert v.shape == tuple(e["shape"]) and v.dtype == np.dtype(e["dtype"]) and v.dtype.byteorder in (np.dtype(e["dtype"]).byteorder, "=", "|")
    assert (v.dtype.byteorder == ">") == e["dtype"].startswith(">")
    assert v.layout == e["layout"] and v.filters == tuple(e["filters"])
    assert v.chunk_shape == (None if e["chunks"] is None else tuple(e["chunks"]))
    fill, scale, offset = rule_of(e)
    assert (v.fill is None) == (fill is None) and (fill is None or np.array_equal(np.float64(v.fill), np.float64(fill), equal_nan=True))
    assert v.scale == scale and v.offset == offset
    assert v.flipped == (file in FLIPPED)
    x, y = stored(file, "x"), stored(file, "y")
    g = v.geometry
    assert g.x0 == x[0] and g.dx == (x[-1] - x[0]) / (x.size - 1) and g.dy < 0 and g.y0 == max(y[0], y[-1]) and g.registration == "pixel"


def test_variable_none_picks_the_only_plane_or_lists_them(nc):
    assert nc.open_netcdf(os.path.join(GOLDEN, "gmt_z.nc")).name == "z"
    assert nc.open_netcdf(os.path.join(GOLDEN, "packed_be.nc")).name == "thickness"
    with pytest.raises(ValueError, match=r"2 variables of rank 2 \(VX, VY\)"):
        nc.open_netcdf(os.path.join(GOLDEN, "vel_chunked.nc"))
    with pytest.raises(ValueError, match=r"\(bed, mask\)"):
        nc.open_netcdf(os.path.join(GOLDEN, "old_style.nc"))
    with pytest.raises(ValueError, match="no variable 'nope'"):
        nc.open_netcdf(os.path.join(GOLDEN, "gmt_z.nc"), "nope")


def test_what_the_fixtures_exercise(nc):
    vx = nc.open_netcdf(os.path.join(GOLDEN, "vel_chunked.nc"), "VX")
    assert len(vx._chunks) == 11 and 2 not in vx._chunks                      # chunk (0, 2) was never written
    assert sorted(m for _, _, m in vx._chunks.values())[-2:] == [0, 2]        # one chunk skipped deflate
    assert vx.applied(2) == ("shuffle",) and vx.applied(0) == ("shuffle", "deflate") and vx.storage_fill == np.float32(-9999.0)
    # that chunk, (1, 1), lies in the file shuffled and not deflated: the restatement's un-shuffle alone gives what libhdf5 read
    offset, nbytes, mask = vx._chunks[5]
    raw = open(os.path.join(GOLDEN, "vel_chunked.nc"), "rb").read()
    chunk = rs.samples(rs.unshuffle(raw[offset:offset + nbytes], 4), 4, False).reshape(32, 16)
    assert mask == 2 and nbytes == 32 * 16 * 4 and np.array_equal(chunk.view(np.uint32), stored("vel_chunked.nc", "VX")[32:64, 16:32].view(np.uint32))
    assert raw[8] == 0 and b"OHDR" in raw                                     # superblock 0, version-2 object headers (tracked order)
    raw = open(os.path.join(GOLDEN, "packed_be.nc"), "rb").read()
    assert raw[8] == 2
    raw = open(os.path.join(GOLDEN, "old_style.nc"), "rb").read()
    assert raw[:8] != b"\x89HDF\r\n\x1a\n" and raw[512:520] == b"\x89HDF\r\n\x1a\n" and raw[520] == 0      # behind a user block
    assert b"OHDR" not in raw and b"SNOD" in raw and b"TREE" in raw and b"HEAP" in raw
    bed = nc.open_netcdf(os.path.join(GOLDEN, "old_style.nc"), "bed")
    assert bed.chunk_shape == (1, 13) and nc.open_netcdf(os.path.join(GOLDEN, "old_style.nc"), "mask").fill == 255
    with np.errstate(all="ignore"):
        vy = stored("vel_chunked.nc", "VY")
    assert (np.signbit(vy) & (vy == 0)).any() and np.isnan(stored("vel_chunked.nc", "VX")).any()


@pytest.mark.parametrize("file,variable", READABLE)
def test_read_equals_libhdf5_through_the_restatement(nc, file, variable):
    e = entry(file, variable)
    fill, scale, offset = rule_of(e)
    path = os.path.join(GOLDEN, file)
    got, info = nc.read_netcdf(path, variable)
    want = rs.expected(stored(file, variable), fill, scale, offset, flipped=file in FLIPPED)
    assert got.dtype == np.float32 and rs.same(got, want) and np.isnan(want).any()
    if np.dtype(e["dtype"]) == np.dtype("<f4") and fill is None:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    plain, _ = nc.read_netcdf(path, variable, mask_and_scale=False)
    assert rs.same(plain, rs.expected(stored(file, variable), flipped=file in FLIPPED))
    # windows agree with slices of the whole: one cutting through chunks, one pixel, the last row and column
    g = info["geometry"]
    H, W = got.shape
    for row0, col0, h, w in [(3, 5, H - 7, W - 9), (H // 2, W // 2, 1, 1), (H - 1, W - 1, 1, 1), (0, 0, 2, W)]:
        wb = (g.x0 + (col0 - 0.5) * g.dx, g.y0 + (row0 + h - 0.5) * g.dy, g.x0 + (col0 + w - 0.5) * g.dx, g.y0 + (row0 - 0.5) * g.dy)
        part, pinfo = nc.read_netcdf(path, variable, window_bound=wb)
        assert pinfo["window"] == (row0, col0, h, w)
        assert rs.same(part, got[row0:row0 + h, col0:col0 + w])
        assert pinfo["geometry"].x0 == col0 * g.dx + g.x0 and pinfo["geometry"].y0 == row0 * g.dy + g.y0
        v = nc.open_netcdf(path, variable)
        plan = v.plan(wb)
        if v.layout == "chunked":
            want_plan = [p for p in rs.chunk_plan(v.shape, v.chunk_shape, (row0, col0, h, w), v.flipped) if p[0] in v._chunks]
            assert [tuple(b[[5, 2, 3, 4, 6]]) for b in plan.blocks.tolist() for b in [np.array(b)]] == want_plan
        else:
            assert plan.blocks[:, 2].sum() == h and (plan.blocks[:, 6] == (-1 if v.flipped else 1)).all()


def test_a_chunk_never_written_reads_as_the_storage_fill(nc):
    got, _ = nc.read_netcdf(os.path.join(GOLDEN, "vel_chunked.nc"), "VX")
    assert np.isnan(got[:32, 32:48]).all()          # storage fill -9999 == _FillValue -> NaN
    plain, _ = nc.read_netcdf(os.path.join(GOLDEN, "vel_chunked.nc"), "VX", mask_and_scale=False)
    assert (plain[:32, 32:48] == np.float32(-9999.0)).all()


def test_contraction_sample_literals():
    v, s, o = CONTRACTION_V, CONTRACTION_SCALE, CONTRACTION_OFFSET
    two = rs.values(np.array([v], dtype=np.int16), None, s, o)
    fused = np.float32(float(Fraction(v) * Fraction(s) + Fraction(o)))     # one correct rounding to float64, then one to float32
    assert two.view(np.uint32)[0] == CONTRACTION_TWO_ROUNDINGS and fused.view(np.uint32) == CONTRACTION_FUSED
    from deepbedmap_amd import netcdf

    assert netcdf.convert(np.array([v], dtype=np.int16), None, s, o).view(np.uint32)[0] == CONTRACTION_TWO_ROUNDINGS


# ---- classic files, written by scipy ----
CLASSIC_TYPES = [("b", -128), ("h", -32768), ("i", -2147483647), ("f", -9999.0), ("d", np.nan)]


def write_classic(path, version, code, fill, scaled, ascending=False, H=11, W=7, record=False):
    from scipy.io import netcdf_file

    rng = np.random.default_rng(H * 100 + W + version)
    dt = np.dtype({"b": "i1", "h": "i2", "i": "i4", "f": "f4", "d": "f8"}[code])
    if dt.kind == "i":
        info = np.iinfo(dt)
        data = rng.integers(info.min, info.max, (H, W), endpoint=True).astype(dt)
    else:
        data = (rng.normal(0, 1000, (H, W))).astype(dt)
        data[1, 2] = -0.0
    data[2, 3] = data[H - 1, W - 1] = fill
    with netcdf_file(str(path), "w", version=version) as f:
        f.createDimension("y", None if record else H)
        f.createDimension("x", W)
        x = f.createVariable("x", "d", ("x",))
        x[:] = 100.0 + 25.0 * np.arange(W)
        y = f.createVariable("y", "d", ("y",))
        y[:] = (-50.0 + 25.0 * np.arange(H)) if ascending else (500.0 - 25.0 * np.arange(H))
        v = f.createVariable("band", code, ("y", "x"))
        v[:] = data
        v._FillValue = np.array([fill], dtype=dt)
        if scaled:
            v.scale_factor = np.float64(0.01)
            v.add_offset = np.float32(3.5)
        v.long_name = "a band"
    with netcdf_file(str(path), "r", mmap=False) as f:
        return np.array(f.variables["band"][:]).astype(dt)


@pytest.mark.parametrize("code,fill", CLASSIC_TYPES)
@pytest.mark.parametrize("version", [1, 2])
def test_classic_files_from_scipy(nc, tmp_path, version, code, fill):
    for scaled, ascending in [(False, False), (True, True)]:
        path = tmp_path / f"c{version}{code}{int(scaled)}.nc"
        raw = write_classic(path, version, code, fill, scaled, ascending)
        assert open(path, "rb").read(4) == b"CDF" + bytes([version])
        v = nc.open_netcdf(path)
        assert v.name == "band" and v.layout == "classic" and v.dtype == raw.dtype.newbyteorder(">") and v.flipped == ascending
        assert v.geometry.dy == -25.0 and v.geometry.x0 == 100.0 and v.geometry.y0 == (-50.0 + 25.0 * 10 if ascending else 500.0)
        got, info = nc.read_netcdf(path)
        want = rs.expected(raw, fill, 0.01 if scaled else None, 3.5 if scaled else None, flipped=ascending)
        assert rs.same(got, want) and np.isnan(got).sum() >= 2
        g = info["geometry"]
        part, pinfo = nc.read_netcdf(path, window_bound=(g.x0 + 0.5 * g.dx, g.y0 + 4.5 * g.dy, g.x0 + 3.5 * g.dx, g.y0 + 1.5 * g.dy))
        assert pinfo["window"] == (2, 1, 3, 3) and rs.same(part, got[2:5, 1:4])


def test_classic_bands_split(nc, tmp_path, monkeypatch):
    raw = write_classic(tmp_path / "b.nc", 1, "h", -32768, True, ascending=True)
    whole, _ = nc.read_netcdf(tmp_path / "b.nc")
    monkeypatch.setattr(nc, "BAND_BYTES", 3 * 7 * 2)     # bands of three rows: 3, 3, 3, 2
    v = nc.open_netcdf(tmp_path / "b.nc")
    assert v.plan().block_shape == (3, 7) and v.plan().blocks[:, 2].tolist() == [3, 3, 3, 2] and v.plan().blocks[:, 3].tolist() == [10, 7, 4, 1]
    got, _ = nc.read_netcdf(tmp_path / "b.nc")
    assert rs.same(got, whole) and rs.same(got, rs.expected(raw, -32768, 0.01, 3.5, flipped=True))


# ---- geometry ----
def test_geometry(nc, tmp_path):
    g = nc.open_netcdf(os.path.join(GOLDEN, "gmt_z.nc")).geometry           # ascending y: flipped, north-up, node_offset = 1
    y = stored("gmt_z.nc", "y")
    assert y[1] > y[0] and g.dy == -2.0 and g.y0 == y[-1] and g.registration == "pixel"
    g = nc.open_netcdf(os.path.join(GOLDEN, "vel_chunked.nc"), "VX").geometry    # descending y: as it lies; no node_offset: pixel
    assert (g.x0, g.y0, g.dx, g.dy, g.registration) == (-1000000.0, 500000.0, 450.0, -450.0, "pixel")
    # node_offset = 0: gridline (the attribute's int32 value patched in a copy)
    data = bytearray(open(os.path.join(GOLDEN, "gmt_z.nc"), "rb").read())
    f = nc._File(os.path.join(GOLDEN, "gmt_z.nc"))
    root = nc._Object(f, nc._open_hdf5(f, 0)[0], 8, 8, "/")
    one = next(at + len(body) - 4 for typ, body, at, _ in root.find(0x0C) if b"node_offset" in body)   # (the value ends the message)
    assert struct.unpack_from("<i", data, one)[0] == 1
    data[one:one + 4] = struct.pack("<i", 0)
    (tmp_path / "grid.nc").write_bytes(bytes(data))
    assert nc.open_netcdf(tmp_path / "grid.nc").geometry.registration == "gridline"
    data[one:one + 4] = struct.pack("<i", 2)
    (tmp_path / "bad.nc").write_bytes(bytes(data))
    with pytest.raises(ValueError, match="node_offset"):
        nc.open_netcdf(tmp_path / "bad.nc")
    # absent coordinates: None, and a window cannot be placed
    v = nc.open_netcdf(os.path.join(GOLDEN, "gmt_z.nc"), coords=("lon", "lat"))
    assert v.geometry is None and not v.flipped
    assert rs.same(nc.read_netcdf(os.path.join(GOLDEN, "gmt_z.nc"), coords=("lon", "lat"))[0], rs.expected(stored("gmt_z.nc", "z"), np.nan))
    with pytest.raises(ValueError, match="no coordinates"):
        v.plan((0, 0, 1, 1))
    # uneven coordinates: refused
    from scipy.io import netcdf_file

    with netcdf_file(str(tmp_path / "uneven.nc"), "w") as f:
        f.createDimension("y", 3)
        f.createDimension("x", 3)
        f.createVariable("x", "d", ("x",))[:] = [0.0, 1.0, 3.0]
        f.createVariable("y", "d", ("y",))[:] = [2.0, 1.0, 0.0]
        f.createVariable("z", "f", ("y", "x"))[:] = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError, match="not evenly spaced"):
        nc.open_netcdf(tmp_path / "uneven.nc")
    with netcdf_file(str(tmp_path / "lengths.nc"), "w") as f:
        f.createDimension("y", 3)
        f.createDimension("x", 3)
        f.createDimension("n", 4)
        f.createVariable("x", "d", ("n",))[:] = [0.0, 1.0, 2.0, 3.0]
        f.createVariable("y", "d", ("y",))[:] = [2.0, 1.0, 0.0]
        f.createVariable("z", "f", ("y", "x"))[:] = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError, match="do not match"):
        nc.open_netcdf(tmp_path / "lengths.nc")


# ---- refusals ----
@pytest.mark.parametrize("file,match", [
    ("refused_dense_links.nc", "dense link storage"),
    ("refused_latest_index.nc", "version-4 data layout with a chunk index.*h5format_convert"),
    ("refused_fletcher32.nc", r"filter 3 \(fletcher32\)"),
    ("refused_rank3.nc", "'v' has rank 3.*only rank 2"),
    ("refused_uint32.nc", "datatype uint32"),
    ("refused_dense_attrs.nc", "dense attribute storage"),
    ("refused_external.nc", "external storage"),
])
def test_refusal_fixtures(nc, file, match):
    with pytest.raises(ValueError, match=match):
        nc.open_netcdf(os.path.join(GOLDEN, file))
    with pytest.raises(ValueError, match=match):
        nc.read_netcdf(os.path.join(GOLDEN, file), "v0" if "dense_links" in file else "v")


def patched(tmp_path, file, name, edit):
    data = bytearray(open(os.path.join(GOLDEN, file), "rb").read())
    data = edit(data) or data
    (tmp_path / name).write_bytes(bytes(data))
    return tmp_path / name


def test_patched_refusals(nc, tmp_path):
    def four_byte_offsets(d):
        assert d[512 + 13] == 8
        d[512 + 13] = 4
    with pytest.raises(ValueError, match="offsets of 4 bytes"):
        nc.open_netcdf(patched(tmp_path, "old_style.nc", "o4.nc", four_byte_offsets), "bed")

    def superblock_9(d):
        d[8] = 9
    with pytest.raises(ValueError, match="superblock version 9"):
        nc.open_netcdf(patched(tmp_path, "gmt_z.nc", "s9.nc", superblock_9))

    # virtual storage: the layout class of a version-4 layout message made 3
    def virtual(d):
        at = d.index(bytes([4, 2]), d.index(b"OHDR", 200))      # (version 4, class 2: the first such pair behind the dataset's header)
        d[at + 1] = 3
    with pytest.raises(ValueError, match="virtual storage"):
        nc.open_netcdf(patched(tmp_path, "refused_latest_index.nc", "virtual.nc", virtual))

    (tmp_path / "cdf5.nc").write_bytes(b"CDF\x05" + bytes(60))
    with pytest.raises(ValueError, match="CDF-5"):
        nc.open_netcdf(tmp_path / "cdf5.nc")
    (tmp_path / "junk.nc").write_bytes(b"II*\0" + bytes(600))
    with pytest.raises(ValueError, match="neither a classic netCDF file"):
        nc.open_netcdf(tmp_path / "junk.nc")

    write_classic(tmp_path / "rec.nc", 1, "f", -9999.0, False, record=True)
    with pytest.raises(ValueError, match="record variable"):
        nc.open_netcdf(tmp_path / "rec.nc", "band", coords=("lon", "lat"))

    # a chunk address past the end of the file: the address in the B-tree's key of chunk 4 replaced
    v = nc.open_netcdf(os.path.join(GOLDEN, "packed_be.nc"))
    address = struct.pack("<Q", v._chunks[4][0])

    def far_chunk(d):
        assert d.count(address) == 1
        at = d.index(address)
        d[at:at + 8] = struct.pack("<Q", len(d) + 1000)
    far = patched(tmp_path, "packed_be.nc", "far.nc", far_chunk)
    with pytest.raises(ValueError, match=r"chunk 4 of 'thickness' \(address \d+, \d+ bytes\) lies outside the file"):
        nc.read_netcdf(far)
    g = v.geometry   # ... and a window that does not touch chunk 4 still reads
    part, _ = nc.read_netcdf(far, window_bound=(g.x0 - 0.5 * g.dx, g.y0 + 7.5 * g.dy, g.x0 + 7.5 * g.dx, g.y0 - 0.5 * g.dy))
    assert part.shape == (8, 8)

    # truncated headers
    (tmp_path / "t1.nc").write_bytes(open(os.path.join(GOLDEN, "gmt_z.nc"), "rb").read()[:300])
    with pytest.raises(ValueError, match="lies outside the file .300 bytes.: truncated"):
        nc.open_netcdf(tmp_path / "t1.nc")
    write_classic(tmp_path / "full.nc", 2, "h", -32768, True)
    (tmp_path / "t2.nc").write_bytes(open(tmp_path / "full.nc", "rb").read()[:90])
    with pytest.raises(ValueError, match="truncated header"):
        nc.open_netcdf(tmp_path / "t2.nc")
    (tmp_path / "t3.nc").write_bytes(open(tmp_path / "full.nc", "rb").read()[:-20])
    with pytest.raises(ValueError, match=r"row band 0 of '\w+' .*lies outside the file"):
        nc.read_netcdf(tmp_path / "t3.nc")

    # the shuffle filter's element size (its one client value, behind its name) differs from the type's
    def shuffle_8(d):
        at = d.index(b"shuffle\0")
        assert struct.unpack_from("<I", d, at + 8)[0] == 4
        d[at + 8:at + 12] = struct.pack("<I", 8)
    with pytest.raises(ValueError, match="shuffle filter's element size 8 differs from the type's 4"):
        nc.open_netcdf(patched(tmp_path, "vel_chunked.nc", "sh.nc", shuffle_8), "VX")

    # a needed attribute of a type that is not decoded: _FillValue's datatype class made 'opaque'
    def opaque_fill(d):
        at = d.index(b"_FillValue\0")
        k = d.index(bytes([0x11]), at + 11)     # class 1 (floating point), version 1
        assert k - at < 24
        d[k] = 0x15
    with pytest.raises(ValueError, match="attribute '_FillValue' of variable 'z' is opaque"):
        nc.open_netcdf(patched(tmp_path, "gmt_z.nc", "op.nc", opaque_fill))


def test_a_malformed_stream_on_the_host(nc, tmp_path):
    from deepbedmap_amd import DbmError

    v = nc.open_netcdf(os.path.join(GOLDEN, "packed_be.nc"))
    offset = v._chunks[0][0]

    def garbage(d):
        d[offset + 2:offset + 6] = b"\xff\xff\xff\xff"
    with pytest.raises(DbmError, match="block 0 of 'thickness': malformed deflate stream"):
        nc.read_netcdf(patched(tmp_path, "packed_be.nc", "bad.nc", garbage))


def test_raster_open_keeps_its_message_for_other_paths():
    """`Raster.open` goes to netCDF only for `netcdf:FILE:VARIABLE`; a netCDF file under its plain name is still 'not a TIFF'."""
    from deepbedmap_amd import Raster

    with pytest.raises(ValueError, match="not a TIFF file"):
        Raster.open(os.path.join(GOLDEN, "gmt_z.nc"))
    with pytest.raises(ValueError, match="no variable 'nope'"):
        Raster.open("netcdf:" + os.path.join(GOLDEN, "gmt_z.nc") + ":nope")
    with pytest.raises(ValueError, match="netcdf:FILE:VARIABLE"):
        Raster.open("netcdf:" + os.path.join(GOLDEN, "gmt_z.nc"))
