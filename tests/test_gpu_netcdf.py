"""-m gpu: dbm_chunk_decode (nc_chunks.hip: un-shuffle, byte order, fill, scale, placement in one kernel; deflate through the inflater of
tiff_inflate.hip) against the NumPy restatement on blocks built here with NumPy and zlib; `read_netcdf_resident` and `Raster.open`
against the host reader on the committed fixtures.  Nothing is approximate: every comparison is on the float32 bits, NaNs at the same
positions (a NaN's payload is compared where the rule keeps it: float32 samples without fill and scale).

Shapes: 1 x 1, 1 x 67, 3 x 5, 16 x 16, 32 x 16 and 64 x 65 (more than one workgroup: a workgroup takes 4 x 256 elements), and block
widths 255, 256, 257 around the workgroup size of 256 threads."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import netcdf_restatement as rs  # noqa: E402
import test_netcdf_host as host  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = host.GOLDEN
WORKGROUP = 256     # NC_THREADS of nc_chunks.hip
SHAPES = [(1, 1), (1, 67), (3, 5), (16, 16), (32, 16), (64, 65), (2, WORKGROUP - 1), (2, WORKGROUP), (2, WORKGROUP + 1)]
SENTINEL = np.float32(-123456.0)


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


def bits_of(value, sample_type):
    dt = np.dtype(rs.SAMPLE_TYPES[sample_type])
    return int(np.asarray(value, dtype=dt).reshape(1).view(np.dtype("u%d" % dt.itemsize))[0])


def call(dbm, payload, table, compression, shuffle, sample_type, big, bw, bh, fill, scale, offset, out, n_blocks=None):
    from deepbedmap_amd.resident import devptr

    ctx = out.ctx
    payload = np.frombuffer(bytes(payload) or b"\0", dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.int64)
    has_scale = scale is not None or offset is not None
    ctx.call("dbm_chunk_decode", devptr(payload), payload.size, devptr(table), len(table) if n_blocks is None else n_blocks, compression,
             int(shuffle), sample_type, int(big), bw, bh, 0 if fill is None else 1, 0 if fill is None else bits_of(fill, sample_type),
             int(has_scale), 1.0 if scale is None else scale, 0.0 if offset is None else offset, devptr(out), out.shape[0], out.shape[1])
    out.written()


def pack(blocks, placements, sample_type, big, shuffle, compression):
    """The payload and the table of `blocks` (native (bh, bw) arrays) placed at `placements` = (rows held, out_row, out_col, step)."""
    itemsize = np.dtype(rs.SAMPLE_TYPES[sample_type]).itemsize
    payload, table = b"", []
    for k, (block, (rows, orow, ocol, step)) in enumerate(zip(blocks, placements)):
        data = rs.stored_bytes(block, sample_type, big)
        if shuffle:
            data = rs.shuffle(data, itemsize)
        if compression == 8:
            data = zlib.compress(data, 6)
        else:
            payload += b"\0" * (-len(payload) % 8)
        table.append([len(payload), len(data), rows, orow, ocol, 100 + k, step, 0])
        payload += data
    return payload, table


def decode(dbm, blocks, placements, plane_shape, sample_type, big, shuffle, compression, fill=None, scale=None, offset=None):
    """(got, want): the plane from the device and from the restatement, both started from the sentinel."""
    from deepbedmap_amd import DeviceArray

    bh, bw = blocks[0].shape
    payload, table = pack(blocks, placements, sample_type, big, shuffle, compression)
    out = DeviceArray(plane_shape).set(np.full(plane_shape, SENTINEL, np.float32))
    call(dbm, payload, table, compression, shuffle, sample_type, big, bw, bh, fill, scale, offset, out)
    want = np.full(plane_shape, SENTINEL, np.float32)
    for block, (rows, orow, ocol, step) in zip(blocks, placements):
        rs.place(want, rs.values(block, fill, scale, offset), rows, orow, ocol, step)
    return out.get(), want


def random_block(rng, shape, sample_type, fill):
    dt = np.dtype(rs.SAMPLE_TYPES[sample_type])
    if dt.kind == "f":
        a = rng.normal(0.0, 1000.0, shape).astype(dt)
        a.flat[rng.integers(0, a.size, max(1, a.size // 9))] = np.nan
        a.flat[rng.integers(0, a.size, max(1, a.size // 9))] = -0.0
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, shape, endpoint=True).astype(dt)
    if fill is not None:
        a.flat[rng.integers(0, a.size, max(1, a.size // 7))] = fill
    return a


FILLS = {0: 255, 1: -32768, 2: 65535, 3: -2147483648, 4: -9999.0, 5: -9999.0, 6: -128}


@pytest.mark.parametrize("compression", [1, 8])
@pytest.mark.parametrize("shuffle", [0, 1])
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("sample_type", range(7))
def test_blocks_against_the_restatement(dbm, sample_type, big, shuffle, compression):
    rng = np.random.default_rng(1000 * sample_type + 100 * big + 10 * shuffle + compression)
    for k, (bh, bw) in enumerate(SHAPES):
        fill = FILLS[sample_type] if k % 3 != 2 else None
        scale, offset = ((0.1, -3.25), (None, None), (None, 7.5), (2.5, None))[k % 4]
        blocks = [random_block(rng, (bh, bw), sample_type, fill) for _ in range(4)]
        H, W = 2 * bh + 3, 2 * bw + 3
        short = max(1, bh - 1)
        # inside, top down; bottom up from the last row with fewer rows held; hanging over the top right corner; running past the
        # bottom left corner, bottom up.  No two of them meet: blocks of one call may be written in any order
        placements = [(bh, 1, 1, 1), (short, H - 1, bw + 2, -1), (bh, -(bh // 2), W - bw // 2 - 1, 1), (bh, H + bh // 2 - 1, -(bw // 2), -1)]
        got, want = decode(dbm, blocks, placements, (H, W), sample_type, big, shuffle, compression, fill, scale, offset)
        assert rs.same(got, want), (bh, bw, fill, scale, offset)
        assert (want == SENTINEL).any() and (want != SENTINEL).any()          # untouched cells stay, placed cells changed
        if sample_type == 4 and fill is None and scale is None and offset is None:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # payloads too


def test_fills_by_value(dbm):
    nan_a = np.array([0x7FC00000, 0xFFC12345, 0x7F800001], np.uint32).view(np.float32)
    # float32: a NaN fill matches every NaN, whatever its payload; without a fill the payloads pass through untouched
    block = np.array([[1.5, nan_a[0], nan_a[1], nan_a[2], -0.0, 0.0, np.inf, -np.inf]], np.float32)
    for big in (0, 1):
        for shuffle in (0, 1):
            got, want = decode(dbm, [block], [(1, 0, 0, 1)], (1, 8), 4, big, shuffle, 8, fill=np.float32(np.nan))
            assert rs.same(got, want) and np.isnan(got[0, 1:4]).all() and not np.isnan(got[0, [0, 4, 5, 6, 7]]).any()
            got, want = decode(dbm, [block], [(1, 0, 0, 1)], (1, 8), 4, big, shuffle, 1)
            assert np.array_equal(got.view(np.uint32), block.view(np.uint32)) and np.array_equal(want.view(np.uint32), block.view(np.uint32))
            # 0.0 against -0.0, both ways
            for fill in (np.float32(0.0), np.float32(-0.0)):
                got, want = decode(dbm, [block], [(1, 0, 0, 1)], (1, 8), 4, big, shuffle, 1, fill=fill)
                assert rs.same(got, want) and np.isnan(got[0, 4]) and np.isnan(got[0, 5]) and got[0, 0] == 1.5
    block64 = np.array([[1.5, np.nan, -0.0, 0.0, 1e300, -1e-300, np.float64(np.float32(3.1)), 2.0 ** -130]], np.float64)
    for fill in (np.nan, 0.0, -0.0, 1e300):
        got, want = decode(dbm, [block64], [(1, 0, 0, 1)], (1, 8), 5, 1, 1, 8, fill=np.float64(fill))
        assert rs.same(got, want)
    got, want = decode(dbm, [block64], [(1, 0, 0, 1)], (1, 8), 5, 0, 0, 1)
    assert rs.same(got, want) and np.isinf(got[0, 4]) and got[0, 7] == np.float32(2.0 ** -130)      # overflow to inf, a float32 subnormal
    for sample_type, fill in FILLS.items():        # every type: the fill and its neighbours
        dt = np.dtype(rs.SAMPLE_TYPES[sample_type])
        if dt.kind == "f":
            block = np.array([[fill, np.nextafter(dt.type(fill), dt.type(0)), 0.0, -fill]], dt)
        else:
            block = np.array([[fill, fill + 1 if fill < 0 else fill - 1, 0, 1]], dt)
        got, want = decode(dbm, [block], [(1, 0, 0, 1)], (1, 4), sample_type, 1, 1, 1, fill=fill, scale=0.5, offset=1.0)
        assert rs.same(got, want) and np.isnan(got[0, 0]) and not np.isnan(got[0, 1:]).any()


def test_the_scale_is_not_contracted(dbm):
    v, s, o = host.CONTRACTION_V, host.CONTRACTION_SCALE, host.CONTRACTION_OFFSET
    block = np.array([[v, v, -v, 1]], np.int16)
    got, want = decode(dbm, [block], [(1, 0, 0, 1)], (1, 4), 1, 1, 1, 8, scale=s, offset=o)
    assert want.view(np.uint32)[0, 0] == host.CONTRACTION_TWO_ROUNDINGS
    assert got.view(np.uint32)[0, 0] == host.CONTRACTION_TWO_ROUNDINGS != host.CONTRACTION_FUSED
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_status_11_leaves_the_plane_untouched(dbm):
    from deepbedmap_amd import DeviceArray

    good = np.arange(32, dtype=np.int16).reshape(4, 8)
    raw = rs.stored_bytes(good, 1, 0)
    cases = {
        "malformed deflate stream": zlib.compress(raw)[:2] + b"\xff\xff\xff\xff" + zlib.compress(raw)[6:],
        "does not decode to the block's size": zlib.compress(raw[:-2]),
        "does not decode to the block's size ": zlib.compress(raw[:48]),      # only the three rows held: an HDF5 chunk is stored whole
    }
    for what, bad in cases.items():
        streams = [zlib.compress(raw), bad]
        payload = b"".join(streams)
        rows = 3 if what.endswith(" ") else 4
        table = [[0, len(streams[0]), 4, 0, 0, 40, 1, 0], [len(streams[0]), len(bad), rows, 4, 0, 41, 1, 0]]
        out = DeviceArray((8, 8)).set(np.full((8, 8), SENTINEL, np.float32))
        with pytest.raises(dbm.DbmError, match="block 41.*" + what.strip() + ".*nothing of this call was written") as e:
            call(dbm, payload, table, 8, 0, 1, 0, 8, 4, None, None, None, out)
        assert e.value.code == 11 and (out.get() == SENTINEL).all()
        call(dbm, payload, table[:1], 8, 0, 1, 0, 8, 4, None, None, None, out)      # the good block alone goes through
        assert np.array_equal(out.get()[:4], good.astype(np.float32)) and (out.get()[4:] == SENTINEL).all()


def test_refusals_and_the_empty_call(dbm):
    from deepbedmap_amd import DeviceArray
    from deepbedmap_amd.resident import devptr

    out = DeviceArray((8, 8)).set(np.full((8, 8), SENTINEL, np.float32))
    ctx = out.ctx
    payload = np.zeros(64, np.uint8)
    base = dict(n=1, compression=1, shuffle=0, sample_type=1, big=0, bw=8, bh=4, has_fill=0, fill_bits=0, has_scale=0, out=devptr(out),
                out_h=8, out_w=8, payload=devptr(payload), table=None, row=[0, 64, 4, 0, 0, 9, 1, 0], bytes=64)

    def run(**kw):
        a = dict(base, **kw)
        table = np.array([a["row"]], dtype=np.int64)
        ctx.call("dbm_chunk_decode", a["payload"], a["bytes"], devptr(table) if a["table"] is None else a["table"], a["n"], a["compression"],
                 a["shuffle"], a["sample_type"], a["big"], a["bw"], a["bh"], a["has_fill"], a["fill_bits"], a["has_scale"], 1.0, 0.0, a["out"],
                 a["out_h"], a["out_w"])

    refused = [
        dict(n=-1), dict(compression=5), dict(compression=0), dict(shuffle=2), dict(big=2), dict(has_fill=2), dict(has_scale=-1),
        dict(sample_type=7), dict(sample_type=-1), dict(has_fill=1, fill_bits=1 << 16), dict(bw=0), dict(bh=0),
        dict(bw=1 << 16, bh=1 << 14), dict(out_h=0), dict(out_w=0), dict(payload=None), dict(out=None), dict(table=C.c_void_p(None)),
        dict(row=[8, 64, 4, 0, 0, 9, 1, 0]), dict(row=[-8, 64, 4, 0, 0, 9, 1, 0]), dict(row=[0, 64, 0, 0, 0, 9, 1, 0]),
        dict(row=[0, 64, 5, 0, 0, 9, 1, 0]), dict(row=[0, 64, 4, 0, 0, 9, 0, 0]), dict(row=[0, 64, 4, 0, 0, 9, 2, 0]),
        dict(row=[4, 60, 3, 0, 0, 9, 1, 0]), dict(row=[0, 62, 4, 0, 0, 9, 1, 0]), dict(row=[0, 48, 3, 0, 0, 9, 1, 0], shuffle=1),
        dict(row=[0, 64, 4, 1 << 41, 0, 9, 1, 0]), dict(row=[0, 64, 4, 0, -(1 << 41), 9, 1, 0]),
    ]
    for kw in refused:
        with pytest.raises(dbm.DbmError, match="dbm_chunk_decode") as e:
            run(**kw)
        assert e.value.code == 1, kw
    assert (out.get() == SENTINEL).all()
    run(row=[0, 48, 3, 0, 0, 9, 1, 0])                       # (not shuffled: the rows held are enough)
    run(n=0, payload=None, table=C.c_void_p(None), out=None)  # n_blocks = 0 succeeds, whatever the pointers
    got = out.get()
    assert (got[:3] == 0).all() and (got[3:] == SENTINEL).all()


# ---- the files ----
@pytest.mark.parametrize("file,variable", host.READABLE)
def test_fixtures_resident_equals_host(dbm, file, variable):
    path = os.path.join(GOLDEN, file)
    want, winfo = dbm.read_netcdf(path, variable)
    dev, info = dbm.read_netcdf_resident(path, variable)
    assert isinstance(dev, dbm.DeviceArray) and rs.same(dev.get(), want) and np.isnan(want).any()
    assert info["window"] == winfo["window"] and info["geometry"] == winfo["geometry"] and info["filters"] == winfo["filters"]
    for kw in (dict(inflate="host"), dict(inflate="device"), dict(workspace_limit=1, inflate="device"), dict(workspace_limit=1, inflate="host"),
               dict(mask_and_scale=False, inflate="device"), dict(mask_and_scale=False, inflate="host")):
        dev, _ = dbm.read_netcdf_resident(path, variable, **kw)
        ref = dbm.read_netcdf(path, variable, mask_and_scale=False)[0] if "mask_and_scale" in kw else want
        assert rs.same(dev.get(), ref), kw
    g = winfo["geometry"]
    H, W = want.shape
    for row0, col0, h, w in [(3, 5, H - 7, W - 9), (H // 2, W // 2, 1, 1), (H - 1, W - 1, 1, 1)]:
        wb = (g.x0 + (col0 - 0.5) * g.dx, g.y0 + (row0 + h - 0.5) * g.dy, g.x0 + (col0 + w - 0.5) * g.dx, g.y0 + (row0 - 0.5) * g.dy)
        for where in ("device", "host"):
            dev, info = dbm.read_netcdf_resident(path, variable, window_bound=wb, inflate=where)
            assert info["window"] == (row0, col0, h, w) and rs.same(dev.get(), want[row0:row0 + h, col0:col0 + w])


def test_only_the_chunks_of_the_window_are_uploaded(dbm, monkeypatch):
    from deepbedmap_amd import _lib

    ctx = _lib.default_context()
    calls = []
    real = ctx.call

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(ctx, "call", spy)     # (on the context itself: an attribute of the object wins over the class's)
    path = os.path.join(GOLDEN, "vel_chunked.nc")
    v = dbm.open_netcdf(path, "VX")
    g = v.geometry
    wb = (g.x0 + 15.5 * g.dx, g.y0 + 63.5 * g.dy, g.x0 + 31.5 * g.dx, g.y0 + 31.5 * g.dy)     # rows 32..63, columns 16..31: chunk (1, 1)
    plan = v.plan(wb)
    assert plan.blocks[:, 5].tolist() == [5] and plan.blocks[0, 7] == 2
    dbm.read_netcdf_resident(path, "VX", window_bound=wb, inflate="device", ctx=ctx)
    decodes = [a for n, a in calls if n == "dbm_chunk_decode"]
    assert len(decodes) == 1 and decodes[0][1] == 32 * 16 * 4 and decodes[0][4] == 1 and decodes[0][5] == 1     # stored, shuffled, not deflated
    calls.clear()
    dbm.read_netcdf_resident(path, "VX", inflate="device", ctx=ctx)
    decodes = [a for n, a in calls if n == "dbm_chunk_decode"]
    assert sorted((a[3], a[4]) for a in decodes) == [(1, 1), (10, 8)]     # one call per filter mask
    assert sum(a[1] for a in decodes) == sum(nbytes for _, nbytes, _ in v._chunks.values())


def test_a_malformed_chunk_names_the_file_and_the_block(dbm, tmp_path):
    v = dbm.open_netcdf(os.path.join(GOLDEN, "packed_be.nc"))
    offset = v._chunks[3][0]

    def garbage(d):
        d[offset + 2:offset + 6] = b"\xff\xff\xff\xff"
    bad = host.patched(tmp_path, "packed_be.nc", "bad.nc", garbage)
    with pytest.raises(dbm.DbmError, match=r"bad\.nc.*block 3.*malformed deflate stream") as e:
        dbm.read_netcdf_resident(bad, inflate="device")
    assert e.value.code == 11
    with pytest.raises(dbm.DbmError, match="block 3: malformed deflate stream"):
        dbm.read_netcdf_resident(bad, inflate="host")


def test_w2_from_netcdf_equals_w2_from_host_arrays(dbm):
    """The reference's W2 path: `netcdf:FILE:VX` / `:VY` opened on the GPU, through selective_tile and get_deepbedmap_model_inputs,
    against the same calls on Rasters built from the host reader's arrays and geometry."""
    path = os.path.join(GOLDEN, "vel_chunked.nc")
    opened = {v: dbm.Raster.open(f"netcdf:{path}:{v}") for v in ("VX", "VY")}
    hosted = {}
    for v in ("VX", "VY"):
        a, info = dbm.read_netcdf(path, v)
        hosted[v] = dbm.Raster(a, info["geometry"], nodata=np.nan)
        assert opened[v].geometry == info["geometry"] and np.isnan(opened[v].nodata) and opened[v].shape == a.shape
        assert rs.same(opened[v].device().get(), a)
    rng = np.random.default_rng(3)
    bound = (-995000.0, 474000.0, -986000.0, 492000.0)
    coarse = dbm.Raster(rng.normal(0, 500, (60, 60)).astype(np.float32), dbm.GridGeometry(-1009500.0, 509500.0, 1000.0, -1000.0, "pixel"), nodata=-9999.0)
    rema = dbm.Raster(rng.normal(0, 500, (300, 300)).astype(np.float32), dbm.GridGeometry(-1004950.0, 499950.0, 100.0, -100.0, "pixel"))
    for raster in (opened, hosted):
        raster["tile"] = dbm.selective_tile(raster["VX"], [bound], padding=1000, resolution=500, gapfiller=0.0).get()
        raster["inputs"] = [t.get() for t in dbm.get_deepbedmap_model_inputs(bound, coarse, rema, raster["VX"], raster["VY"], coarse)]
    assert opened["tile"].shape == (1, 1, 40, 22) and rs.same(opened["tile"], hosted["tile"]) and np.isfinite(opened["tile"]).any()
    assert opened["inputs"][2].shape == (1, 2, 40, 22)
    for a, b in zip(opened["inputs"], hosted["inputs"]):
        assert rs.same(a, b)
    win = dbm.Raster.open(f"netcdf:{path}:VY", window_bound=(bound[0] - 2000, bound[1] - 2000, bound[2] + 2000, bound[3] + 2000))
    assert win.shape[0] < 70 and rs.same(dbm.selective_tile(win, [bound], padding=1000, resolution=500, gapfiller=0.0).get(),
                                         dbm.selective_tile(hosted["VY"], [bound], padding=1000, resolution=500, gapfiller=0.0).get())
