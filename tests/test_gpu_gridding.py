"""-m gpu: dbm_points_polar_stereographic, dbm_points_region and dbm_points_blockmedian (reference data_prep.py:322-334, 353-378,
406-407) through the C ABI and through deepbedmap_amd/gridding.py, against the float64 NumPy restatement
(tests/gridding_restatement.py, pinned to published and hand-computed answers and to pandas in tests/test_gridding_host.py).

Block medians and the region are compared BIT FOR BIT: a median is a selection or one IEEE halving of a sum, a block index is one
subtraction, one division, one addition and a floor in the same order on both sides, min / max are exact.  No tolerance.
Projection: |delta| <= 1e-6 m -- device tan, sin, cos, pow in float64 are a few ulp, rho <= 3.4e6 m, so the expected error is of order
1e-8 m; the bound leaves two orders of margin and lies four orders below the data's centimetre precision.  Derived, not measured (the
measured worst case is printed and recorded in DESIGN.md 6e)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gridding_restatement as gr  # noqa: E402

pytestmark = pytest.mark.gpu

INC = 250.0
X0, Y0 = -2000000.0, 150000.0   # the north-west node of every test grid: coordinates of the order of the continent's
GN72 = (6378137.0, 298.257223563, -71.0, 70.0, 6000000.0, 6000000.0)


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def region_of_shape(shape):
    H, W = shape
    return (X0, X0 + (W - 1) * INC, Y0 - (H - 1) * INC, Y0)


def block_points(r, c, k, rng, z=None):
    """k rows inside block (r, c): centimetre coordinates strictly inside the block, z of both signs around +-3000 m"""
    x = X0 + c * INC + np.round(rng.uniform(-124.0, 124.0, k), 2)
    y = Y0 - r * INC + np.round(rng.uniform(-124.0, 124.0, k), 2)
    if z is None:
        z = np.round(rng.normal(0.0, 3000.0, k), 3)
    return np.stack([x, y, np.asarray(z, dtype=np.float64)], axis=1)


def class_populations(dbm):
    from deepbedmap_amd import gridding

    pops = [1, 2, 3, 4, 63, 64, 65]
    for b in gridding.BLOCKMEDIAN_CLASS_BOUNDARIES:
        pops += [b - 1, b, b + 1]
    return sorted(set(p for p in pops if p >= 1)), max(70000, 8 * gridding.BLOCKMEDIAN_LDS)   # the last: past any on-chip class


def classes_cloud(dbm, shape=(37, 211), seed=5):
    """every size class at its edges, one block beyond the on-chip classes, duplicates, constant blocks, one-ulp middles, zeros of both
    signs; full blocks sit on every third node, the rest stays empty"""
    rng = np.random.default_rng(seed)
    H, W = shape
    pops, huge = class_populations(dbm)
    slots = [(r, c) for r in range(0, H, 3) for c in range(1, W, 3)]
    rng.shuffle(slots)
    slots = iter(slots)
    parts = []
    for k in pops + [huge]:
        parts.append(block_points(*next(slots), k, rng))
        dup = block_points(*next(slots), k, rng)          # heavy duplication: values from a pool of three
        dup[:, 2] = rng.choice([-12.5, 0.25, 3000.0], k)
        dup[:, 0] = dup[0, 0]
        parts.append(dup)
    for k in (1, 2, 5, 8, 40, 64, 100):
        parts.append(block_points(*next(slots), k, rng, z=np.full(k, -2875.125)))             # every z equal
        parts.append(block_points(*next(slots), k, rng, z=rng.choice([-0.0, 0.0], k)))        # zeros of both signs
        mixed = np.concatenate([[-0.0, 0.0], rng.choice([-1.0, 1.0, 0.0, -0.0], k)])[:k]
        parts.append(block_points(*next(slots), k, rng, z=mixed))
    for k in (2, 4, 30, 64, 66, 2050):   # even counts whose two middle values differ by one ulp
        mid = 1234.5678
        z = np.concatenate([np.full(k // 2, mid), np.full(k // 2, np.nextafter(mid, np.inf))])
        z[: k // 2 - 1] -= rng.uniform(1.0, 100.0, k // 2 - 1)
        z[k // 2 + 1:] += rng.uniform(1.0, 100.0, k // 2 - 1)
        parts.append(block_points(*next(slots), k, rng, z=z))
    pts = np.concatenate(parts)
    # rows that must be dropped, and rows outside the region
    junk = block_points(0, 1, 12, rng)
    junk[0:2, 0] = [np.nan, np.inf]
    junk[2:4, 1] = [np.nan, -np.inf]
    junk[4:6, 2] = [np.nan, np.inf]
    junk[6:9, 0] = [X0 - 125.01, X0 + (W - 1) * INC + 125.0, X0 + (W - 1) * INC + 1e7]
    junk[9:12, 1] = [Y0 + 125.01, Y0 - (H - 1) * INC - 125.0, -1e300]
    pts = np.concatenate([pts, junk])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def small_cloud(shape, n, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    x = X0 + np.round(rng.uniform(-0.6, W - 0.4, n) * INC, 2)
    y = Y0 - np.round(rng.uniform(-0.6, H - 0.4, n) * INC, 2)
    return np.ascontiguousarray(np.stack([x, y, np.round(rng.normal(0, 3000, n), 3)], axis=1))


CLOUDS = {
    "classes": lambda d: ((37, 211), classes_cloud(d)),
    "1x1": lambda d: ((1, 1), small_cloud((1, 1), 77, 1)),
    "1x7": lambda d: ((1, 7), small_cloud((1, 7), 301, 2)),
    "5x1": lambda d: ((5, 1), small_cloud((5, 1), 90, 3)),
    "sparse": lambda d: ((2000, 3000), small_cloud((2000, 3000), 1000, 4)),
    "dense": lambda d: ((37, 211), small_cloud((37, 211), 300000, 6)),
    "n255": lambda d: ((5, 9), small_cloud((5, 9), 255, 7)),
    "n256": lambda d: ((5, 9), small_cloud((5, 9), 256, 8)),
    "n257": lambda d: ((5, 9), small_cloud((5, 9), 257, 9)),
    # the spacing does not divide the region (ymax - ymin = 3.4 inc, xmax - xmin = 5.3 inc): the north edge is the fitted one
    "fitted": lambda d: ((4, 6), small_cloud((4, 6), 2000, 10)),
}
REGIONS = {"fitted": (X0, X0 + 5.3 * INC, Y0 - 3.4 * INC, Y0)}
_cache = {}


def cloud(dbm, name):
    """(shape, region, points, restated (table, grid, counts)): built and restated once per session, never modified"""
    if name not in _cache:
        shape, pts = CLOUDS[name](dbm)
        region = REGIONS.get(name) or region_of_shape(shape)
        assert gr.block_shape(region, INC) == shape
        pts.setflags(write=False)
        _cache[name] = (shape, region, pts, gr.blockmedian(pts, region, INC))
    return _cache[name]


def abi_blockmedian(dbm, pts, region, inc=INC, capacity=None, device=False, n=None, fill=None):
    """-> (status, m, table[:capacity], grid, counts); fill = (table, grid, counts) sentinels written into the outputs first"""
    from deepbedmap_amd import _lib

    lib, ctx = _lib.lib(), _lib.default_context()
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts) if n is None else n
    try:
        H, W = gr.block_shape(region, inc)
        assert H > 0 and W > 0 and H * W < 2 ** 27
    except (ValueError, AssertionError, OverflowError, ZeroDivisionError):
        H, W = 2, 2   # refused calls: any small output
    capacity = max(min(len(pts), H * W), 1) if capacity is None else capacity
    table = np.full((max(capacity, 1), 3), fill[0] if fill else np.nan)
    grid = dbm.to_device(np.full((H, W), fill[1] if fill else 0.0, dtype=np.float32))
    chost = np.full((H, W), fill[2] if fill else 0, dtype=np.int32)
    cdev = ctx.malloc(chost.nbytes)
    _lib.check(lib.dbm_memcpy_h2d(ctx.handle, C.c_void_p(cdev), chost.ctypes.data_as(C.c_void_p), chost.nbytes), ctx.handle)
    r4 = np.array(region, dtype=np.float64)
    m = C.c_int64(-1)
    try:
        if device:
            dp = dbm.DevicePoints(pts if len(pts) else np.zeros((0, 3)), ctx)
            tdev = ctx.malloc(table.nbytes)
            _lib.check(lib.dbm_memcpy_h2d(ctx.handle, C.c_void_p(tdev), table.ctypes.data_as(C.c_void_p), table.nbytes), ctx.handle)
            rc = lib.dbm_points_blockmedian(ctx.handle, C.c_void_p(dp.ptr), n, r4.ctypes.data_as(C.POINTER(C.c_double)), inc, C.c_void_p(tdev),
                                            capacity, C.byref(m), C.c_void_p(grid.ptr), C.c_void_p(cdev), _lib.DEVICE_PTRS)
            _lib.check(lib.dbm_memcpy_d2h(ctx.handle, table.ctypes.data_as(C.c_void_p), C.c_void_p(tdev), table.nbytes), ctx.handle)
            ctx.free(tdev)
        else:
            rc = lib.dbm_points_blockmedian(ctx.handle, pts.ctypes.data_as(C.c_void_p), n, r4.ctypes.data_as(C.POINTER(C.c_double)), inc,
                                            table.ctypes.data_as(C.c_void_p), capacity, C.byref(m), C.c_void_p(grid.ptr), C.c_void_p(cdev), 0)
        _lib.check(lib.dbm_memcpy_d2h(ctx.handle, chost.ctypes.data_as(C.c_void_p), C.c_void_p(cdev), chost.nbytes), ctx.handle)
    finally:
        ctx.free(cdev)
    return rc, int(m.value), table, grid.get(), chost


def assert_same(got, want):
    rc, m, table, grid, counts = got
    wt, wg, wc = want
    assert rc == 0 and m == len(wt), (rc, m, len(wt))
    assert np.array_equal(counts, wc)
    assert np.array_equal(bits(grid), bits(wg))            # NaN mask included
    assert np.array_equal(bits(table[:m]), bits(wt))


@pytest.mark.parametrize("name", list(CLOUDS))
def test_blockmedian_bit_for_bit(dbm, name):
    shape, region, pts, want = cloud(dbm, name)
    assert_same(abi_blockmedian(dbm, pts, region), want)
    assert int(want[2].sum()) > 0
    if name == "classes":   # the cloud does reach every class and the global-memory path
        pops, huge = class_populations(dbm)
        have = set(want[2].ravel().tolist())
        assert set(pops) <= have and huge in have


def test_blockmedian_edge_rules(dbm):
    shape = (4, 6)
    region = region_of_shape(shape)
    xmax, ymin = region[1], region[2]
    z = iter(np.arange(1.0, 100.0))
    rows = []
    for k in range(5):   # exactly on interior boundaries: x = xmin + (k + 1/2) 250 is exact
        rows.append([X0 + (k + 0.5) * INC, Y0, next(z)])
    for k in range(3):
        rows.append([X0, Y0 - (k + 0.5) * INC, next(z)])
    rows += [[X0 - 125.0, Y0, next(z)], [xmax + 125.0, Y0, next(z)], [X0, Y0 + 125.0, next(z)], [X0, ymin - 125.0, next(z)]]
    for eps in (1e-9, 0.01):   # just outside / just inside
        rows += [[X0 - 125.0 - eps, Y0, next(z)], [xmax + 125.0 - eps, Y0, next(z)], [X0, Y0 + 125.0 + eps, next(z)],
                 [X0, ymin - 125.0 + eps, next(z)]]
    for bad in (np.nan, np.inf, -np.inf):
        rows += [[bad, Y0, next(z)], [X0, bad, next(z)], [X0, Y0, bad]]
    pts = np.array(rows)
    blk = gr.assign(pts, region, INC)
    assert blk[:5].tolist() == [1, 2, 3, 4, 5] and blk[5:8].tolist() == [6, 12, 18]   # ties go east and south
    assert blk[8:12].tolist() == [0, -1, 0, -1]    # xmin - 125 and ymax + 125 fall to the first block; xmax + 125, ymin - 125 are out
    assert (blk[-9:] == -1).all()
    assert_same(abi_blockmedian(dbm, pts, region), gr.blockmedian(pts, region, INC))


def test_blockmedian_empty_tables(dbm):
    shape = (3, 4)
    region = region_of_shape(shape)
    for pts in (np.zeros((0, 3)), np.full((300, 3), np.nan)):
        for device in (False, True):
            rc, m, table, grid, counts = abi_blockmedian(dbm, pts, region, device=device, fill=(5.0, 5.0, 5))
            assert rc == 0 and m == 0
            assert np.isnan(grid).all() and grid.shape == shape and (counts == 0).all()
            assert (table == 5.0).all()


def test_blockmedian_is_deterministic_and_permutation_invariant(dbm):
    shape, region, pts, want = cloud(dbm, "classes")
    first = abi_blockmedian(dbm, pts, region)
    assert_same(first, want)
    rng = np.random.default_rng(11)
    for trial in range(4):   # the same rows again, then three permutations of them
        again = abi_blockmedian(dbm, pts if trial == 0 else pts[rng.permutation(len(pts))], region)
        assert again[:2] == first[:2]
        for a, b in zip(again[2:], first[2:]):
            assert bits(a).tobytes() == bits(b).tobytes()


def test_blockmedian_calling_forms_agree(dbm):
    shape, region, pts, want = cloud(dbm, "classes")
    assert_same(abi_blockmedian(dbm, pts, region, device=True), want)
    rstr = "/".join(repr(float(v)) for v in region)
    table = dbm.blockmedian(pts, rstr, spacing=250)
    assert np.array_equal(bits(table), bits(want[0]))
    dp = dbm.DevicePoints(pts)
    assert np.array_equal(bits(dbm.blockmedian(dp, region)), bits(want[0]))
    grid, geom, counts = dbm.blockmedian_grid(dp, region, counts=True)
    assert np.array_equal(bits(grid), bits(want[1])) and np.array_equal(counts, want[2])
    assert (geom.x0, geom.y0, geom.dx, geom.dy, geom.registration) == (X0, Y0, INC, -INC, "gridline")
    try:
        import pandas as pd
    except ImportError:
        pd = None
    if pd is not None:
        df = dbm.blockmedian(pd.DataFrame(pts, columns=["x", "y", "z"]), region)
        assert list(df.columns) == ["x", "y", "z"] and np.array_equal(bits(df.to_numpy()), bits(want[0]))


def test_blockmedian_grid_feeds_grdtrack_in_place(dbm):
    shape, region, pts, want = cloud(dbm, "dense")
    dgrid, geom = dbm.blockmedian_grid(pts, region, download=False)
    assert isinstance(dgrid, dbm.DeviceArray) and dgrid.shape == shape
    r, c = np.nonzero(want[2])
    centres = np.stack([geom.x0 + c * geom.dx, geom.y0 + r * geom.dy], axis=1)
    z, _ = dbm.grdtrack(centres, dgrid, geom, interpolation="nearest")
    assert np.array_equal(z, want[1][r, c].astype(np.float64))
    rough = dbm.standard_deviation_2d(dgrid, 3)
    assert rough.shape == shape
    raster = dbm.Raster(dgrid, geom)
    assert (raster.H, raster.W) == shape


def test_blockmedian_north_edge_fitted_to_the_spacing(dbm):
    shape, region, pts, want = cloud(dbm, "fitted")
    north = region[2] + 3 * INC
    assert gr.north_edge(region, INC) == north != region[3]
    # rows are anchored at the fitted edge: the restatement anchored at the region's own ymax would bin differently
    assert not np.array_equal(gr.assign(pts, region, INC), gr.assign(pts, (region[0], region[1], region[3] - 3 * INC, region[3]), INC))
    assert_same(abi_blockmedian(dbm, pts, region, device=True), want)
    grid, geom, counts = dbm.blockmedian_grid(pts, region, counts=True)
    assert (geom.x0, geom.y0, geom.dx, geom.dy) == (region[0], north, INC, -INC)
    assert np.array_equal(bits(grid), bits(want[1])) and np.array_equal(counts, want[2])
    assert np.array_equal(bits(dbm.blockmedian(pts, region)), bits(want[0]))


# ---- region ----
def abi_region(dbm, pts, inc, device=False):
    from deepbedmap_amd import _lib

    lib, ctx = _lib.lib(), _lib.default_context()
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    region, count = np.full(4, 99.0), C.c_int64(-1)
    if device:
        dp = dbm.DevicePoints(pts.reshape(-1, 3), ctx)
        out = ctx.malloc(64)
        rc = lib.dbm_points_region(ctx.handle, C.c_void_p(dp.ptr), len(pts), pts.shape[1], inc, C.c_void_p(out), C.c_void_p(out + 32),
                                   _lib.DEVICE_PTRS)
        host = np.empty(5)
        _lib.check(lib.dbm_memcpy_d2h(ctx.handle, host.ctypes.data_as(C.c_void_p), C.c_void_p(out), 40), ctx.handle)
        ctx.free(out)
        return rc, host[:4].copy(), int(host[4:].view(np.int64)[0])
    rc = lib.dbm_points_region(ctx.handle, pts.ctypes.data_as(C.c_void_p), len(pts), pts.shape[1], inc, region.ctypes.data_as(C.c_void_p),
                               C.byref(count), 0)
    return rc, region, int(count.value)


@pytest.mark.parametrize("name", list(CLOUDS))
def test_region_bit_for_bit(dbm, name):
    _, _, pts, _ = cloud(dbm, name)
    for inc in (250.0, 1000.0, 0.3):
        want, wcount = gr.region(pts, inc)
        for device in (False, True):
            rc, region, count = abi_region(dbm, pts, inc, device)
            assert rc == 0 and count == wcount
            assert np.array_equal(bits(region), bits(want)), (region, want)
        again = abi_region(dbm, pts, inc)
        assert bits(again[1]).tobytes() == bits(want).tobytes()


def test_region_signs_multiples_and_empty(dbm):
    pts = np.array([[-1.0, -251.0, 0.0], [250.0, 500.0, 0.0], [np.nan, 9e9, 0.0], [9e9, 1.0, np.inf], [-0.5, -0.25, -np.inf]])
    rc, region, count = abi_region(dbm, pts, 250.0)
    assert rc == 0 and count == 2 and region.tolist() == [-250.0, 250.0, -500.0, 500.0]
    rc, region, count = abi_region(dbm, pts[:, :2].copy(), 250.0)   # without a z column rows 3 and 4 count
    want, wcount = gr.region(pts[:, :2], 250.0)
    assert rc == 0 and count == wcount == 4 and np.array_equal(bits(region), bits(want))
    one = np.array([[-750.0, 1250.0, 3.0]])          # multiples of the increment do not move
    rc, region, count = abi_region(dbm, one, 250.0)
    assert rc == 0 and count == 1 and region.tolist() == [-750.0, -750.0, 1250.0, 1250.0]
    for empty in (np.zeros((0, 3)), np.full((513, 3), np.nan)):
        for device in (False, True):
            rc, region, count = abi_region(dbm, empty, 250.0, device)
            assert rc == 0 and count == 0 and np.isnan(region).all()
    cloud10 = 10000 * np.random.RandomState(seed=42).rand(30).reshape(10, 3)
    assert dbm.get_region(cloud10) == "500/8500/0/9750"
    assert dbm.get_region(dbm.DevicePoints(cloud10), round_increment=250) == "500/8500/0/9750"
    assert dbm.get_region(pts) == "-250/250/-500/500"
    assert dbm.region_of(np.full((3, 3), np.nan))[1] == 0


# ---- projection ----
def abi_project(dbm, pts, proj=gr.EPSG3031, in_place=False):
    from deepbedmap_amd import _lib

    lib, ctx = _lib.lib(), _lib.default_context()
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    p = np.array(proj, dtype=np.float64)
    out = pts.copy() if in_place else np.full_like(pts, -1.0)
    src = out if in_place else pts
    rc = lib.dbm_points_polar_stereographic(ctx.handle, src.ctypes.data_as(C.c_void_p), pts.shape[0], pts.shape[1],
                                            p.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.c_void_p), 0)
    assert rc == 0, lib.dbm_last_error(ctx.handle)
    return out


def test_projection_against_the_restatement(dbm):
    rng = np.random.default_rng(3)
    n = 100000
    pts = np.stack([rng.uniform(-180.0, 180.0, n), rng.uniform(-90.0, -60.0, n), rng.normal(0, 3000, n), rng.normal(0, 1, n)], axis=1)
    pts[:6, 0] = [0.0, 77.0, 180.0, -180.0, 0.0, -45.0]
    pts[:6, 1] = [-90.0, -90.0, -80.0, -80.0, -71.0, -71.0]   # the pole, the date line, the standard parallel
    pts[6, 0], pts[7, 1], pts[8, :2] = np.nan, np.inf, (-np.inf, np.nan)
    want = gr.polar_stereographic(pts)
    got = abi_project(dbm, pts)
    assert np.array_equal(bits(got[:, 2:]), bits(pts[:, 2:]))      # further columns pass through
    assert np.isnan(got[6:9, :2]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want[:, 0])
    worst = np.abs(got[ok, :2] - want[ok, :2]).max()
    print(f"projection: worst |delta| against the float64 restatement over {int(ok.sum())} points: {worst:.3e} m")
    assert worst <= 1e-6
    assert np.array_equal(got[:2, :2], np.zeros((2, 2)))           # the pole, exactly
    # in place == out of place; a two-column table; a DevicePoints converted where it lies
    assert bits(abi_project(dbm, pts, in_place=True)).tobytes() == bits(got).tobytes()
    two = abi_project(dbm, pts[:, :2].copy())
    assert bits(two).tobytes() == bits(got[:, :2]).tobytes()
    dp = dbm.DevicePoints(pts[:, :3].copy())
    assert dbm.reproject(dp) is dp
    from deepbedmap_amd import _lib
    back = np.empty((n, 3))
    _lib.check(_lib.lib().dbm_memcpy_d2h(dp.ctx.handle, back.ctypes.data_as(C.c_void_p), C.c_void_p(dp.ptr), back.nbytes), dp.ctx.handle)
    assert bits(back).tobytes() == bits(got[:, :3]).tobytes()
    via = dbm.reproject(pts[9:, :3])
    assert isinstance(via, np.ndarray) and bits(via).tobytes() == bits(got[9:, :3]).tobytes()


def test_projection_published_answers(dbm):
    out = abi_project(dbm, np.array([[120.0, -75.0]]), GN72)     # EPSG Guidance Note 7-2, variant B example
    assert abs(out[0, 0] - 7255380.79) <= 0.005 and abs(out[0, 1] - 7053389.56) <= 0.005, out
    a, f = 6378137.0, 1.0 / 298.257223563
    e2 = 2 * f - f * f
    s71 = np.sin(np.deg2rad(71.0))
    closed = a * np.cos(np.deg2rad(71.0)) / np.sqrt(1.0 - e2 * s71 * s71)
    lons = np.array([-180.0, -135.0, -90.0, -45.0, 0.0, 45.0, 90.0, 135.0])
    pts = np.concatenate([[[0.0, -90.0], [0.0, -71.0], [-110.25, -75.5]], np.stack([lons, np.full(8, -77.25)], axis=1)])
    out = dbm.reproject(pts)
    assert out[0].tolist() == [0.0, 0.0]
    assert out[1, 0] == 0.0 and abs(out[1, 1] - closed) <= 1e-6
    assert out[2, 0] < 0 and out[2, 1] < 0
    rho = np.hypot(out[3:, 0], out[3:, 1])
    assert np.all(np.abs(rho - rho[0]) <= 1e-6)


def test_projection_true_scale_at_the_pole(dbm):
    """phi_F = -90: k0 = 1 (variant A), rho = 2 a t / sqrt((1+e)^(1+e) (1-e)^(1-e)), written out here"""
    a, f = 6378137.0, 1.0 / 298.257223563
    e = np.sqrt(2 * f - f * f)
    lat = np.array([-90.0, -85.0, -71.0, -60.0])
    phi = np.deg2rad(lat)
    t = np.tan(np.pi / 4 + phi / 2) / ((1 + e * np.sin(phi)) / (1 - e * np.sin(phi))) ** (e / 2)
    rho = 2 * a * t / np.sqrt((1 + e) ** (1 + e) * (1 - e) ** (1 - e))
    proj = (a, 298.257223563, -90.0, 0.0, 0.0, 0.0)
    pts = np.stack([np.full(4, 90.0), lat], axis=1)     # on the 90 E meridian: E = rho, N = 0
    want = gr.polar_stereographic(pts, proj)
    assert np.all(np.abs(want[:, 0] - rho) <= 1e-8) and np.all(np.abs(want[:, 1]) <= 1e-8)
    got = abi_project(dbm, pts, proj)
    assert np.all(np.abs(got - want) <= 1e-6) and got[0].tolist() == [0.0, 0.0]


def test_reproject_refuses_northern_latitudes_of_a_resident_table(dbm):
    from deepbedmap_amd import _lib

    for bad in (1e-300, 10.0, -90.000001):
        pts = np.array([[10.0, -80.0, 1.0], [20.0, bad, 2.0], [np.nan, np.inf, 3.0]])
        dp = dbm.DevicePoints(pts)
        with pytest.raises(ValueError, match="latitude"):
            dbm.reproject(dp)
        back = np.empty_like(pts)
        _lib.check(_lib.lib().dbm_memcpy_d2h(dp.ctx.handle, back.ctypes.data_as(C.c_void_p), C.c_void_p(dp.ptr), back.nbytes), dp.ctx.handle)
        assert bits(back).tobytes() == bits(pts).tobytes()     # nothing was converted
    ok = dbm.DevicePoints(np.array([[10.0, -90.0, 1.0], [20.0, 0.0, 2.0], [20.0, -0.0, 2.0]]))
    assert dbm.reproject(ok) is ok


# ---- refusals ----
def test_refusals_name_the_entry_point_and_write_nothing(dbm):
    from deepbedmap_amd import _lib

    lib, ctx = _lib.lib(), _lib.default_context()

    def refused(rc, name):
        assert rc == 1, rc
        assert name in lib.dbm_last_error(ctx.handle).decode()

    shape, region, pts, want = cloud(dbm, "n257")
    m = len(want[0])
    fill = (12345.0, 7.0, -7)

    def untouched(got):
        rc, mm, table, grid, counts = got
        refused(rc, "dbm_points_blockmedian")
        assert mm == -1 and (table == fill[0]).all() and (grid == fill[1]).all() and (counts == fill[2]).all()

    for device in (False, True):
        untouched(abi_blockmedian(dbm, pts, region, capacity=m - 1, device=device, fill=fill))   # one row short: m is computed first
        for inc in (0.0, -250.0, np.nan, np.inf):
            untouched(abi_blockmedian(dbm, pts, region, inc=inc, device=device, fill=fill))
        for bad in ((np.nan, 0.0, 0.0, 0.0), (0.0, np.inf, 0.0, 0.0), (0.0, 0.0, -np.inf, 0.0), (250.0, 0.0, 0.0, 0.0), (0.0, 0.0, 250.0, 0.0)):
            untouched(abi_blockmedian(dbm, pts, bad, device=device, fill=fill))
        untouched(abi_blockmedian(dbm, pts, (0.0, 50000 * INC, 0.0, 50000 * INC), device=device, fill=fill))   # 50 001^2 >= 2^31 blocks
        untouched(abi_blockmedian(dbm, pts, (0.0, 1e300, 0.0, 1.0), device=device, fill=fill))
        untouched(abi_blockmedian(dbm, pts, region, n=2 ** 31, device=device, fill=fill))
    # the same call with one more row of capacity succeeds: nothing was left behind
    assert_same(abi_blockmedian(dbm, pts, region, capacity=m), want)

    r4 = np.array(region)
    mm = C.c_int64(-1)
    rp = r4.ctypes.data_as(C.POINTER(C.c_double))
    refused(lib.dbm_points_blockmedian(ctx.handle, None, 5, rp, INC, None, 0, C.byref(mm), None, None, 0), "dbm_points_blockmedian")
    refused(lib.dbm_points_blockmedian(ctx.handle, pts.ctypes.data_as(C.c_void_p), 5, rp, INC, None, 5, C.byref(mm), None, None, 0),
            "dbm_points_blockmedian")
    refused(lib.dbm_points_blockmedian(ctx.handle, pts.ctypes.data_as(C.c_void_p), 5, None, INC, None, 0, C.byref(mm), None, None, 0),
            "dbm_points_blockmedian")
    refused(lib.dbm_points_blockmedian(ctx.handle, pts.ctypes.data_as(C.c_void_p), 5, rp, INC, None, 0, None, None, None, 0),
            "dbm_points_blockmedian")
    assert mm.value == -1

    out, count = np.full(4, 99.0), C.c_int64(-1)
    pp, op = pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for inc in (0.0, -1.0, np.nan, np.inf):
        refused(lib.dbm_points_region(ctx.handle, pp, len(pts), 3, inc, op, C.byref(count), 0), "dbm_points_region")
    refused(lib.dbm_points_region(ctx.handle, pp, len(pts), 1, INC, op, C.byref(count), 0), "dbm_points_region")
    refused(lib.dbm_points_region(ctx.handle, pp, 2 ** 31, 3, INC, op, C.byref(count), 0), "dbm_points_region")
    refused(lib.dbm_points_region(ctx.handle, None, 3, 3, INC, op, C.byref(count), 0), "dbm_points_region")
    refused(lib.dbm_points_region(ctx.handle, pp, 3, 3, INC, None, C.byref(count), 0), "dbm_points_region")
    refused(lib.dbm_points_region(ctx.handle, pp, 3, 3, INC, op, None, 0), "dbm_points_region")
    assert (out == 99.0).all() and count.value == -1

    lonlat = np.array([[10.0, -80.0, 1.0], [20.0, -70.0, 2.0]])
    res = np.full_like(lonlat, 99.0)
    lp, rp2 = lonlat.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)

    def proj(*v):
        return np.array(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))

    name = "dbm_points_polar_stereographic"
    for bad in ((0.0, 298.0, -71.0, 0, 0, 0), (np.nan, 298.0, -71.0, 0, 0, 0), (6378137.0, 1.0, -71.0, 0, 0, 0), (6378137.0, np.inf, -71.0, 0, 0, 0),
                (6378137.0, 298.0, 71.0, 0, 0, 0), (6378137.0, 298.0, 0.0, 0, 0, 0), (6378137.0, 298.0, -91.0, 0, 0, 0),
                (6378137.0, 298.0, np.nan, 0, 0, 0), (6378137.0, 298.0, -71.0, np.nan, 0, 0), (6378137.0, 298.0, -71.0, 0, np.inf, 0),
                (6378137.0, 298.0, -71.0, 0, 0, np.nan)):
        refused(lib.dbm_points_polar_stereographic(ctx.handle, lp, 2, 3, proj(*bad), rp2, 0), name)
    good = gr.EPSG3031
    refused(lib.dbm_points_polar_stereographic(ctx.handle, lp, 2, 1, proj(*good), rp2, 0), name)
    refused(lib.dbm_points_polar_stereographic(ctx.handle, lp, 2 ** 31, 3, proj(*good), rp2, 0), name)
    refused(lib.dbm_points_polar_stereographic(ctx.handle, None, 2, 3, proj(*good), rp2, 0), name)
    refused(lib.dbm_points_polar_stereographic(ctx.handle, lp, 2, 3, proj(*good), None, 0), name)
    refused(lib.dbm_points_polar_stereographic(ctx.handle, lp, 2, 3, None, rp2, 0), name)
    assert (res == 99.0).all()
    # nothing was launched, the context still works
    assert np.array_equal(bits(abi_project(dbm, lonlat)), bits(abi_project(dbm, lonlat, in_place=True)))
