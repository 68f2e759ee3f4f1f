"""`deepbedmap_amd.block_reads` on the host (no GPU): what `read_geotiff_resident` and `read_netcdf_resident` share -- the window rule,
the batching cost rule, the two staging layouts and the host inflater -- each against a statement written out by hand."""
import zlib

import numpy as np
import pytest

from deepbedmap_amd import DbmError, GridGeometry

BOUND = (-1000.0, 2000.0, 51000.0, 32000.0)   # 520 x 300 pixels of 100 m (tests/test_geotiff_open_host.py)


@pytest.fixture(scope="module")
def br():
    from deepbedmap_amd import block_reads

    return block_reads


def test_batches_cost_rule(br):
    stored = [100, 5, 300, 40, 7]
    for uploaded in (False, True):
        for limit in (1, 47, 48, 200, 1 << 40):
            runs = br.batches(stored, 32, limit, uploaded)
            assert all(stop > start for start, stop in runs)                                     # never an empty run
            assert [s for s, _ in runs] == [0] + [e for _, e in runs[:-1]] and runs[-1][1] == 5   # consecutive, complete
        assert br.batches(stored, 32, 1, uploaded) == [(k, k + 1) for k in range(5)]
        assert br.batches(stored, 32, 1 << 40, uploaded) == [(0, 5)]
    # host-decoded blocks cost 32 + 16 = 48 each, whatever is stored: 96 holds two, 95 one
    assert br.batches(stored, 32, 96, False) == [(0, 2), (2, 4), (4, 5)]
    assert br.batches(stored, 32, 95, False) == [(k, k + 1) for k in range(5)]
    # uploaded streams cost 32 + stored: 132, 37, 332, 72, 39 -- within 169: {132, 37}, {332} alone (one block always goes), {72, 39}
    assert br.batches(stored, 32, 169, True) == [(0, 2), (2, 3), (3, 5)]
    assert br.batches(stored, 32, 168, True) == [(0, 1), (1, 2), (2, 3), (3, 5)]


def test_stage_uploaded_layout(br):
    streams = [b"abc", b"", b"defgh", b"i"]
    payload, offsets, sizes = br.stage(streams, None, 32, True, True, [0, 1, 2, 3], "f")
    assert payload.dtype == np.uint8 and payload.tobytes() == b"abcdefghi"
    assert sizes.tolist() == [3, 0, 5, 1] and offsets.tolist() == [0, 3, 3, 8]   # the exclusive cumulative sum


def test_stage_slot_layout(br):
    blocks = [bytes(range(1, 6)), bytes(range(10, 26)), bytes(range(30, 47))]   # 5, 16 and 17 bytes
    ids = [7, 8, 9]
    for exact in (True, False):
        payload, offsets, sizes = br.stage(blocks, np.array([5, 16, 17]), 32, False, exact, ids, "f")
        assert payload.size == 96 and offsets.tolist() == [0, 32, 64] and sizes.tolist() == [5, 16, 17]
        for k, b in enumerate(blocks):
            assert payload[32 * k:32 * k + len(b)].tobytes() == b and not payload[32 * k + len(b):32 * (k + 1)].any()
        with pytest.raises(DbmError, match=r"^f: block 8: 15 decoded bytes, 16 expected$"):
            br.stage([blocks[0], blocks[1][:15], blocks[2]], np.array([5, 16, 17]), 32, False, exact, ids, "f")
    with pytest.raises(DbmError, match=r"^f: block 8: 17 decoded bytes, 16 expected$"):
        br.stage([blocks[0], blocks[2], blocks[2]], np.array([5, 16, 17]), 32, False, True, ids, "f")
    payload, _, sizes = br.stage([blocks[0], blocks[2], blocks[2]], np.array([5, 16, 17]), 32, False, False, ids, "f")
    assert sizes.tolist() == [5, 16, 17] and payload[32:48].tobytes() == blocks[2][:16] and not payload[48:64].any()   # cut to 16


def former_window(g, H, W, window_bound):
    """The rule as GeoTiffFile.window and NetcdfVariable.window both stated it."""
    minx, miny, maxx, maxy = (float(v) for v in window_bound)
    xc = np.arange(W, dtype=np.float64) * g.dx + g.x0
    yc = np.arange(H, dtype=np.float64) * g.dy + g.y0
    cols = np.flatnonzero((xc >= minx) & (xc < maxx))
    rows = np.flatnonzero((yc > miny) & (yc <= maxy))
    return int(rows[0]), int(cols[0]), int(rows[-1] - rows[0] + 1), int(cols[-1] - cols[0] + 1)


def test_pixel_window(br):
    g = GridGeometry.from_bounds(BOUND, 300, 520)
    minx, miny, maxx, maxy = BOUND
    for wb, want in (((minx + 30000, maxy - 2000, minx + 31000, maxy - 1000), (10, 300, 10, 10)),       # inside one tile
                     ((minx + 25000, maxy - 30000, minx + 27000, maxy - 25000), (250, 250, 50, 20)),    # across four
                     ((minx + 25050, maxy - 27030, minx + 26949, maxy - 24999), (250, 250, 20, 19)),    # unaligned bounds
                     ((maxx - 1000, miny - 5000, maxx + 5000, miny + 1000), (290, 510, 10, 10))):       # over the image edge
        assert br.pixel_window(lambda: g, 300, 520, wb, "f", "the raster") == want == former_window(g, 300, 520, wb)
    assert br.pixel_window(None, 300, 520, None, "f", "the raster") == (0, 0, 300, 520)

    def missing():
        raise ValueError("no geometry")
    with pytest.raises(ValueError, match="no geometry"):
        br.pixel_window(missing, 300, 520, BOUND, "f", "the raster")
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="^window_bound must be finite$"):     # before the geometry is asked for
            br.pixel_window(missing, 300, 520, (minx, miny, bad, maxy), "f", "the raster")
    with pytest.raises(ValueError, match=r"^f: window_bound \(60000\.0, 2000\.0, 61000\.0, 32000\.0\) holds no pixel centre of 'VX'$"):
        br.pixel_window(lambda: g, 300, 520, (60000, miny, 61000, maxy), "f", repr("VX"))
    assert br.window_geometry(None, 3, 4) is None
    assert br.window_geometry(g, 250, 20) == GridGeometry(x0=20 * g.dx + g.x0, y0=250 * g.dy + g.y0, dx=g.dx, dy=g.dy, registration="pixel")


def test_inflate_on_host_names_the_block_and_the_path(br):
    raw = [bytes([k]) * 100 for k in range(3)]
    streams = [zlib.compress(r) for r in raw]
    assert br.inflate_on_host(streams, [4, 5, 6], "some/file.nc") == raw
    streams[1] = streams[1][:2] + b"\xff\xff\xff\xff" + streams[1][6:]
    with pytest.raises(DbmError, match=r"^some/file\.nc: block 5: malformed deflate stream \("):
        br.inflate_on_host(streams, [4, 5, 6], "some/file.nc")


def test_read_options(br):
    assert br.read_options(None, "device", "r") == br.WORKSPACE_DEFAULT == 1 << 30 and br.read_options(7.9, "host", "r") == 7
    with pytest.raises(ValueError, match="^workspace_limit must be positive$"):
        br.read_options(0, "device", "r")
    with pytest.raises(ValueError, match="^r: inflate 'gpu': 'device' or 'host'$"):
        br.read_options(1, "gpu", "r")
