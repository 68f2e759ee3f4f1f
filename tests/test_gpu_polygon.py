"""-m gpu: dbm_grid_polygon_mask (polygon.hip) and deepbedmap_amd/polygons.py against the float64 NumPy restatement of the definition
(tests/polygon_restatement.py, itself checked against matplotlib and closed forms in tests/test_polygon_host.py); reference
data_prep.py:582-616.

Every comparison is bit for bit, without tolerance: the mask is a pure function of identically rounded float64 operations, and culling,
binning and the parity shortcut may never change it.  Grids and edge counts sit on the kernel's own boundaries (T = polygons.TILE,
K = polygons.EDGE_CHUNK)."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polygon_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu

from deepbedmap_amd import polygons as _pg  # noqa: E402

T, K = _pg.TILE, _pg.EDGE_CHUNK
PX = 250.0
GEOM = (-1_600_000.0, -200_000.0, PX, -PX)                  # continental coordinates, north-up
GEOM_SOUTH_UP = (-1_600_000.0, -230_000.0, PX, PX)          # dy > 0
GEOM_EAST_FIRST = (-1_570_000.0, -200_000.0, -PX, -PX)      # dx < 0
SHAPES = [(1, 1), (1, T + 1), (T - 1, T), (T, T), (T + 1, 2 * T + 1), (33, 47), (97, 131)]
BUFFERS = [0.0, -0.0, 3 * PX, 40 * PX, -2 * PX]


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(scope="module")
def ctx(dbm):
    return dbm.default_context()


def xy(geom, c, r):
    """Coordinates of the (possibly fractional) node position (c, r)."""
    return geom[0] + c * geom[2], geom[1] + r * geom[3]


def zoo(geom, shape):
    """The geometry cases in one polygon set, laid out in node units so that they scale with the grid: a rectangle on nodes (horizontal
    and vertical edges, vertices on nodes, nodes on edges) with a triangular hole; a second part, a diamond on half-nodes that leaves the
    grid; a sliver whose long edge runs exactly through the nodes of the diagonal; a polygon entirely east of the grid (parity from edges
    that are never near); a ring far away (culled)."""
    H, W = shape
    c0, c1, r0, r1 = round(0.2 * W), max(round(0.6 * W), round(0.2 * W) + 2), round(0.2 * H), max(round(0.7 * H), round(0.2 * H) + 2)
    n = max(min(H, W) - 1, 2)
    rings = [
        [xy(geom, c0, r0), xy(geom, c1, r0), xy(geom, c1, r1), xy(geom, c0, r1)],
        [xy(geom, c0 + 0.3 * (c1 - c0), r0 + 0.25 * (r1 - r0)), xy(geom, c0 + 0.71 * (c1 - c0), r0 + 0.4 * (r1 - r0)),
         xy(geom, c0 + 0.45 * (c1 - c0), r0 + 0.8 * (r1 - r0))],
        [xy(geom, 0.8 * W + 0.5, 0.15 * H), xy(geom, 1.1 * W, 0.5 * H + 0.5), xy(geom, 0.8 * W + 0.5, 0.9 * H), xy(geom, 0.68 * W, 0.5 * H + 0.5)],
        [xy(geom, 0, 0), xy(geom, n, n), xy(geom, n - 1.5, n)],
        [xy(geom, W + 5, -5), xy(geom, W + 20, -5), xy(geom, W + 20, 0.5 * H + 0.25), xy(geom, W + 5, 0.5 * H + 0.25)],
        [xy(geom, W + 4000, -3000), xy(geom, W + 4100, -3000), xy(geom, W + 4050, -2900)],
    ]
    return pr.ring_edges(rings)


def far_ring(geom, k):
    """A small triangle a few thousand kilometres away: culling must drop it."""
    x, y = geom[0] + 3.0e6 + 1000.0 * k, geom[1] - 2.5e6 - 700.0 * k
    return [(x, y), (x + 300.0, y + 100.0), (x + 50.0, y + 400.0)]


def padded(geom, shape, count):
    """Exactly `count` edges: the zoo first, then zero-length edges and far-away rings in turn."""
    if count == 0:
        return np.zeros((0, 4))
    if count == 1:
        return np.array([[*xy(geom, -2.5, 0.3 * shape[0]), *xy(geom, shape[1] + 1.25, 0.8 * shape[0])]])
    e = [zoo(geom, shape)]
    have, k = len(e[0]), 0
    assert have <= count
    while have < count:
        if k % 2 == 0 or count - have < 3:
            p = xy(geom, (7 * k) % shape[1] + 0.37, (3 * k) % shape[0])
            e.append(np.array([[p[0], p[1], p[0], p[1]]]))
        else:
            e.append(pr.ring_edges([far_ring(geom, k)]))
        have += len(e[-1])
        k += 1
    out = np.concatenate(e)
    assert len(out) == count
    return out


class Abi:
    """dbm_grid_polygon_mask called directly, the outputs pre-filled so that an untouched output can be told from a written one."""

    def __init__(self, dbm, ctx):
        self.lib, self.L, self.ctx = dbm._lib.lib(), dbm._lib, ctx

    def upload(self, a):
        a = np.ascontiguousarray(a)
        ptr = self.ctx.malloc(max(a.nbytes, 32))
        if a.nbytes:
            self.L.check(self.lib.dbm_memcpy_h2d(self.ctx.handle, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes), self.ctx.handle)
        return ptr

    def download(self, ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self.L.check(self.lib.dbm_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes), self.ctx.handle)
        return out

    def __call__(self, edges, shape, geom, buffer, grid=None, want_mask=True, limit=0, device_edges=False, handle="ctx", geom_null=False,
                 edges_null=False, n_edges=None):
        H, W = shape
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1, 4)
        n = len(e) if n_edges is None else n_edges
        size = max(abs(H * W), 1) if abs(H * W) < 2 ** 26 else 1
        mptr = self.upload(np.full(size, 7, np.uint8)) if want_mask else None
        gptr = self.upload(np.asarray(grid, np.float32)) if grid is not None else None
        eptr = self.upload(e) if device_edges else None
        g = np.asarray(geom, dtype=np.float64)
        try:
            earg = None if edges_null else (C.c_void_p(eptr) if device_edges else e.ctypes.data_as(C.c_void_p))
            rc = self.lib.dbm_grid_polygon_mask(self.ctx.handle if handle == "ctx" else None, earg, n, H, W,
                                                None if geom_null else g.ctypes.data_as(C.POINTER(C.c_double)), buffer,
                                                C.c_void_p(mptr) if mptr else None, C.c_void_p(gptr) if gptr else None, limit,
                                                self.L.DEVICE_PTRS if device_edges else 0)
            m = self.download(mptr, (size,), np.uint8) if mptr else None
            gout = self.download(gptr, np.asarray(grid).shape, np.float32) if gptr else None
        finally:
            for p in (mptr, gptr, eptr):
                if p:
                    self.ctx.free(p)
        return rc, m, gout


@pytest.fixture(scope="module")
def abi(dbm, ctx):
    return Abi(dbm, ctx)


def check(abi, edges, shape, geom, buffer, **kw):
    want = pr.mask(geom, shape, edges, buffer)
    rc, m, _ = abi(edges, shape, geom, buffer, **kw)
    assert rc == 0
    m = m.reshape(shape)
    assert set(np.unique(m)) <= {0, 1}
    assert np.array_equal(m.astype(bool), want), (shape, buffer, int((m.astype(bool) != want).sum()), np.argwhere(m.astype(bool) != want)[:5])
    return want


@pytest.mark.parametrize("buffer", BUFFERS, ids=lambda b: f"b{b!r}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_equals_the_restatement(abi, shape, buffer):
    want = check(abi, zoo(GEOM, shape), shape, GEOM, buffer)
    if shape == (97, 131) and buffer in (0.0, 3 * PX, -2 * PX):
        assert want.any() and not want.all()


@pytest.mark.parametrize("geom", [GEOM_SOUTH_UP, GEOM_EAST_FIRST], ids=["dy_positive", "dx_negative"])
@pytest.mark.parametrize("buffer", [3 * PX, -2 * PX])
def test_flipped_axes(abi, geom, buffer):
    for shape in ((T + 1, 2 * T + 1), (97, 131)):
        want = check(abi, zoo(geom, shape), shape, geom, buffer)
        assert want.any() and not want.all()


@pytest.mark.parametrize("count", [0, 1, K - 1, K, K + 1, 3 * K + 5])
def test_edge_counts_around_the_chunk(abi, count):
    shape = (T + 1, 2 * T + 1)
    edges = padded(GEOM, shape, count)
    for buffer in (3 * PX, -2 * PX, 0.0):
        for limit in (0, 1):     # binned, and every tile over the culled lists
            want = check(abi, edges, shape, GEOM, buffer, limit=limit)
            if count == 0:
                assert not want.any()


def test_an_edge_spanning_many_tiles_and_polygons_around_and_away(abi):
    shape = (97, 131)
    H, W = shape
    long_sliver = pr.ring_edges([[xy(GEOM, -30.5, 3.25), xy(GEOM, W + 40.0, H - 7.5), xy(GEOM, W + 40.0, H - 5.0)]])
    for buffer in (0.0, 3 * PX, -2 * PX):
        want = check(abi, long_sliver, shape, GEOM, buffer)
        assert buffer < 0 or want.any()
    around = pr.ring_edges([[xy(GEOM, -50, -50), xy(GEOM, W + 50, -60), xy(GEOM, W + 70, H + 50), xy(GEOM, -40, H + 45)]])
    for buffer in (0.0, 3 * PX, -2 * PX, 40 * PX):
        assert check(abi, around, shape, GEOM, buffer).all()
    away = pr.ring_edges([far_ring(GEOM, 1), far_ring(GEOM, 2)])
    for buffer in (0.0, 40 * PX, -2 * PX):
        assert not check(abi, away, shape, GEOM, buffer).any()
    # entirely east of the grid: the parity of every node comes from edges that are never near
    east = pr.ring_edges([[xy(GEOM, W + 3, -4.5), xy(GEOM, W + 30, 0.5 * H), xy(GEOM, W + 3, H + 3.5)]])
    assert not check(abi, east, shape, GEOM, 0.0).any()
    assert check(abi, east, shape, GEOM, 4 * PX).any()
    # overlapping parts cancel, orientation does not matter (no node lies on an edge here: ON an edge, d2 depends on the edge's direction)
    a = [xy(GEOM, 10.25, 10.25), xy(GEOM, 60.25, 10.25), xy(GEOM, 60.25, 50.25), xy(GEOM, 10.25, 50.25)]
    b = [xy(GEOM, 40.5, 30.5), xy(GEOM, 100.5, 30.5), xy(GEOM, 100.5, 80.5), xy(GEOM, 40.5, 80.5)]
    m1 = check(abi, pr.ring_edges([a, b]), shape, GEOM, 0.0)
    m2 = check(abi, pr.ring_edges([a[::-1], b]), shape, GEOM, 0.0)
    assert np.array_equal(m1, m2) and not m1[40, 50] and m1[20, 20] and m1[70, 90]


def margin_case():
    """A vertical edge east of the grid whose exact distance from the last column is ABOVE the buffer while x - xa rounds to the buffer
    itself: its box lies outside |buffer| of every tile and of the raster, and d2 still compares <=.  Searched for, deterministically."""
    shape, b = (T + 1, 2 * T + 1), 40 * PX
    for k in range(4000):
        geom = (-1000.1 - 0.013 * k, 3000.0, PX, -PX)
        xs, ys = pr.node_axes(geom, shape)
        x = xs[-1]
        for xa in (np.nextafter(x + b, np.inf), np.nextafter(np.nextafter(x + b, np.inf), np.inf), x + b):
            if Fraction(float(xa)) - Fraction(float(x)) > Fraction(b) and (x - xa) == -b:
                lo, hi = ys[-1] - 77.7, ys[0] + 33.3
                edge = np.array([[xa, lo, xa, hi], [xa, hi, xa, lo]])     # (there and back: the parity cancels)
                return geom, shape, b, edge
    raise AssertionError("no margin case found")


def test_constructed_margin_case(abi):
    geom, shape, b, edge = margin_case()
    inside, near = pr.inside_near(geom, shape, edge, b)
    assert near[:, -1].all() and not near[:, :-1].any() and not inside.any()      # (the restatement says: the last column is near)
    for limit in (0, 1):
        check(abi, edge, shape, geom, b, limit=limit)
        check(abi, edge, shape, geom, -b, limit=limit)
    # ... and among many edges, so that the bins are in play
    edges = np.concatenate([edge, padded(geom, shape, K + 1)])
    check(abi, edges, shape, geom, b)


def test_every_path_gives_the_same_bytes(dbm, ctx, abi):
    shape, small = (97, 131), (33, 47)
    edges = padded(GEOM, shape, 3 * K + 5)
    buffer = 3 * PX
    want = pr.mask(GEOM, shape, edges, buffer)
    assert want.any() and not want.all()
    results = {}
    results["host"] = abi(edges, shape, GEOM, buffer)
    results["device"] = abi(edges, shape, GEOM, buffer, device_edges=True)
    results["again"] = abi(edges, shape, GEOM, buffer)
    results["unbinned"] = abi(edges, shape, GEOM, buffer, limit=1)
    assert dbm.polygons.last_stats(ctx)["schedule"] == 0
    perm = np.random.default_rng(5).permutation(len(edges))
    results["permuted"] = abi(edges[perm], shape, GEOM, buffer, device_edges=True)
    stats = dbm.polygons.last_stats(ctx)
    assert stats["schedule"] == 1 and stats["edges"] == len(edges)
    assert 0 < stats["proximity_edges"] < len(edges) and 0 < stats["parity_edges"] < len(edges)       # the far rings were dropped
    assert stats["tile_entries"] > 0 and stats["band_entries"] > 0
    for name, (rc, m, _) in results.items():
        assert rc == 0, name
        assert np.array_equal(m.reshape(shape), want.astype(np.uint8)), name
    # Python, one resident table on two grids
    poly = dbm.Polygons(edges, n_rings=1)
    g = dbm.GridGeometry(*GEOM)
    first = poly.device(ctx)
    got = dbm.polygon_mask(g, shape, poly, buffer)
    assert got.dtype == bool and got.shape == shape and np.array_equal(got, want)
    got_small = dbm.polygon_mask(g, small, poly, buffer)
    assert np.array_equal(got_small, pr.mask(GEOM, small, edges, buffer))
    assert poly.device(ctx) == first
    dev = dbm.polygon_mask(g, shape, poly, buffer, download=False, workspace_limit=1)
    assert dev.dtype == np.uint8 and dev.shape == shape and np.array_equal(dev.get(), want.astype(np.uint8))


def test_statistics_belong_to_the_context(dbm):
    """dbm_grid_polygon_stats reports the context's own last mask: a context created after another was shut down starts from zeros
    (wherever the allocator puts it), and the same mask on it gives the same statistics."""
    shape, g = (8, 8), dbm.GridGeometry(*GEOM)
    ring = [xy(GEOM, 1.5, 1.5), xy(GEOM, 5.5, 1.5), xy(GEOM, 5.5, 5.5), xy(GEOM, 1.5, 5.5)]
    want = pr.mask(GEOM, shape, pr.ring_edges([ring]), 0.0)
    assert want.sum() == 16

    def masked(c):
        square = dbm.Polygons.from_rings([ring])     # (its device table is freed with it, while the context lives)
        assert np.array_equal(dbm.polygon_mask(g, shape, square, ctx=c), want)
        return dbm.polygons.last_stats(c)

    a = dbm.Context()
    stats_a = masked(a)
    assert stats_a["edges"] == 4
    dbm._lib.check(dbm._lib.lib().dbm_shutdown(a.handle))
    b = dbm.Context()
    try:
        assert set(dbm.polygons.last_stats(b).values()) == {0}
        assert masked(b) == stats_a
    finally:
        dbm._lib.check(dbm._lib.lib().dbm_shutdown(b.handle))


def test_grid_output_keeps_every_other_bit(abi):
    shape = (T + 1, 2 * T + 1)
    edges = zoo(GEOM, shape)
    r = np.random.default_rng(11)
    grid = r.standard_normal(shape).astype(np.float32)
    grid[::3, ::4] = -0.0
    grid.view(np.uint32)[1::5, 2::3] = 0xFFC12345       # a NaN with its own sign and payload
    grid[2::7, 1::6] = np.inf
    for buffer in (0.0, 3 * PX, -2 * PX):
        want = pr.mask(GEOM, shape, edges, buffer)
        rc, m, g = abi(edges, shape, GEOM, buffer, grid=grid)
        assert rc == 0
        assert np.array_equal(m.reshape(shape).astype(bool), want)
        assert np.array_equal(g.view(np.uint32), pr.mask_grid(grid, want).view(np.uint32))
        assert np.array_equal(g.view(np.uint32)[want], grid.view(np.uint32)[want]) and (g.view(np.uint32)[~want] == 0x7FC00000).all()
        rc, m2, g2 = abi(edges, shape, GEOM, buffer, grid=grid, want_mask=False)
        assert rc == 0 and m2 is None and np.array_equal(g2.view(np.uint32), g.view(np.uint32))
        rc, m3, _ = abi(edges, shape, GEOM, buffer)
        assert rc == 0 and np.array_equal(m3, m)


def test_refusals_leave_the_outputs_untouched(abi):
    shape = (T + 1, 2 * T + 1)
    edges = zoo(GEOM, shape)
    grid = np.arange(shape[0] * shape[1], dtype=np.float32).reshape(shape)
    nan_edge, inf_edge = edges.copy(), edges.copy()
    nan_edge[len(edges) // 2, 1] = np.nan
    inf_edge[-1, 2] = -np.inf
    cases = {
        "null ctx": dict(handle=None),
        "null geom": dict(geom_null=True),
        "H 0": dict(shape=(0, shape[1])),
        "W negative": dict(shape=(shape[0], -3)),
        "H W 2^31": dict(shape=(65536, 32768)),
        "n_edges 2^31": dict(n_edges=2 ** 31),
        "geom nan": dict(geom=(np.nan, GEOM[1], PX, -PX)),
        "geom inf": dict(geom=(GEOM[0], np.inf, PX, -PX)),
        "dx zero": dict(geom=(GEOM[0], GEOM[1], 0.0, -PX)),
        "dy zero": dict(geom=(GEOM[0], GEOM[1], PX, 0.0)),
        "dy nan": dict(geom=(GEOM[0], GEOM[1], PX, np.nan)),
        "buffer nan": dict(buffer=np.nan),
        "buffer inf": dict(buffer=np.inf),
        "host nan edge": dict(edges=nan_edge),
        "host inf edge": dict(edges=inf_edge),
        "device nan edge": dict(edges=nan_edge, device_edges=True),
        "device inf edge": dict(edges=inf_edge, device_edges=True),
        "null edges": dict(edges_null=True),
    }
    for name, kw in cases.items():
        args = dict(edges=edges, shape=shape, geom=GEOM, buffer=3 * PX, grid=grid)
        args.update(kw)
        rc, m, g = abi(args.pop("edges"), args.pop("shape"), args.pop("geom"), args.pop("buffer"), **args)
        assert rc == 1, name
        assert (m == 7).all(), name
        assert np.array_equal(g, grid), name
    rc, m, g = abi(edges, shape, GEOM, 3 * PX, want_mask=False)      # both outputs NULL
    assert rc == 1
    # NULL edges are fine without edges
    rc, m, _ = abi(np.zeros((0, 4)), shape, GEOM, 3 * PX, edges_null=True)
    assert rc == 0 and not m.any()


# ---- tile selection ----
def star_scene():
    """A 90 x 110 raster with a NaN patch, and a star polygon with a hole: 40 points, radii alternating 38 and 17 pixels, hole radius 6."""
    shape = (90, 110)
    cx, cy = xy(GEOM, 55, 45)
    ang = 2 * np.pi * np.arange(40) / 40
    rad = np.where(np.arange(40) % 2 == 0, 38.0, 17.0) * PX
    outer = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)
    hang = 2 * np.pi * np.arange(12) / 12
    hole = np.stack([cx + 6 * PX * np.cos(hang), cy + 6 * PX * np.sin(hang)], axis=1)
    r = np.random.default_rng(2)
    grid = r.standard_normal(shape).astype(np.float32) * 100
    grid[60:66, 20:31] = np.nan
    return shape, grid, [outer, hole]


def test_select_tiles(dbm, ctx):
    from deepbedmap_amd.tiling import bounds_from_flags

    shape, grid, rings = star_scene()
    g = dbm.GridGeometry(GEOM[0], GEOM[1], GEOM[2], GEOM[3], registration="pixel")
    poly = dbm.Polygons.from_rings(rings)
    edges = pr.ring_edges(rings)
    assert np.array_equal(poly.edges, edges) and poly.n_rings == 2
    raster = dbm.Raster(grid, g)
    kept = {}
    for buffer in (10 * PX, 0.0):
        m = pr.mask(GEOM, shape, edges, buffer)
        ok = m & np.isfinite(grid)
        flags = np.zeros(((shape[0] - 36) // 3 + 1, (shape[1] - 36) // 3 + 1), np.uint8)
        for i, j in pr.filled_windows(ok, 36, 3):
            flags[i, j] = 1
        want = bounds_from_flags(flags, g, shape, 36, 3)
        got = dbm.select_tiles(raster, poly, buffer=buffer)
        assert got == want, (buffer, len(got), len(want))
        host_masked = dbm.Raster(pr.mask_grid(grid, m), g)
        assert got == dbm.get_window_bounds(host_masked, 36, 36, 3)
        kept[buffer] = got
        # mask_outside: a new raster, the argument untouched
        out = dbm.mask_outside(raster, poly, buffer)
        assert out is not raster and out.geometry == g and out.nodata == raster.nodata
        assert np.array_equal(out.device().get().view(np.uint32), pr.mask_grid(grid, m).view(np.uint32))
        assert np.array_equal(raster.device().get().view(np.uint32), grid.view(np.uint32))
    print("windows kept:", {b: len(v) for b, v in kept.items()})
    assert len(kept[10 * PX]) > 0 and len(kept[0.0]) == 0
    # the chain runs through tile_training_set on the kept windows
    wins = kept[10 * PX]
    r = np.random.default_rng(4)

    def low(res, scale):
        n_r, n_c = int(35_000 // res) + 1, int(40_000 // res) + 1
        geom = dbm.GridGeometry(GEOM[0] - 3000.0 + res / 2, GEOM[1] + 3000.0 - res / 2, res, -res, registration="pixel")
        return dbm.Raster(r.standard_normal((n_r, n_c)).astype(np.float32) * scale, geom)

    filled = dbm.Raster(np.where(np.isfinite(grid), grid, 0.0).astype(np.float32), g)
    out = dbm.tile_training_set([(filled, wins)], low(1000.0, 500.0), low(100.0, 300.0), low(500.0, 50.0), low(500.0, 50.0), low(1000.0, 1.0))
    n = len(wins)
    assert out["Y"].shape == (n, 1, 36, 36) and out["X"].shape == (n, 1, 11, 11) and out["W1"].shape == (n, 1, 110, 110)
    assert out["W2"].shape == (n, 2, 22, 22) and out["W3"].shape == (n, 1, 11, 11)
    y = out["Y"].get()
    assert np.isfinite(y).all()
    west, north = GEOM[0] - PX / 2, GEOM[1] + PX / 2
    c, rr = int(round((wins[0][0] - west) / PX)), int(round((north - wins[0][3]) / PX))
    assert np.array_equal(y[0, 0], grid[rr:rr + 36, c:c + 36])


def test_device_array_of_every_dtype(dbm, ctx):
    """The array type under the masks and every other resident plane (deepbedmap_amd/resident.py): set -> get is the identity on the
    bits for each supported dtype, the sizes and the typestr follow the dtype, and `written()` -- what a stage calls after the library
    wrote into an array -- moves training's content token of a batch that holds the array."""
    from deepbedmap_amd import training

    r = np.random.default_rng(7)
    typestr = {np.float32: "<f4", np.float64: "<f8", np.int32: "<i4", np.uint8: "|u1"}
    for dtype, want in typestr.items():
        for shape in [(1,), (3, 5), (7, 1, 2)]:
            host = r.integers(0, 2 ** 32, size=int(np.prod(shape)) * np.dtype(dtype).itemsize // 4 + 1, dtype=np.uint32)
            host = host.view(np.uint8)[:int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)   # any bits, NaNs too
            a = dbm.DeviceArray(shape, ctx, dtype=dtype)
            assert a.dtype == np.dtype(dtype) and a.shape == shape and a.nbytes == host.nbytes
            assert a.__cuda_array_interface__["typestr"] == want and a.__cuda_array_interface__["data"] == (a.ptr, False)
            got = a.set(host).get()
            assert got.dtype == host.dtype and got.shape == shape and got.tobytes() == host.tobytes()
    plain = dbm.DeviceArray((2, 2), ctx)
    assert plain.dtype == np.float32 and plain.nbytes == 16 and plain.__cuda_array_interface__["typestr"] == "<f4"
    mask = _pg.MaskArray((3, 5), ctx)
    assert isinstance(mask, dbm.DeviceArray) and mask.dtype == np.uint8 and mask.nbytes == 15
    batch = {k: dbm.DeviceArray((1,), ctx) for k in ("X", "W1", "W2", "W3", "Y")}
    before = training._content_token(batch)
    assert training._content_token(batch) == before
    assert batch["W2"].written() is batch["W2"]
    assert training._content_token(batch) != before
