"""-m gpu: dbm_track_error_quantiles and dbm_track_error_histogram (the quartile rows of the reference's error table and its error
histogram, deepbedmap.py:550-563, 575-608) against the NumPy restatement of their rules (tests/track_dist_restatement.py) and against
np.quantile, pandas' describe() and np.histogram themselves: exact equality of values (a zero's sign is not compared), through the C
entry points in both pointer forms and through describe_errors, error_histogram and describe_on_tracks."""
import ctypes as C
import dataclasses
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import track_dist_restatement as td  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS, BLOCKS = 256, 1024          # DBM_TRACK_DIST_THREADS, DBM_TRACK_DIST_BLOCKS (checked against the header below)
Q16 = (0.5, 0.0, 1.0, 0.25, 0.75, 0.25, 0.999, 0.001, 0.5, 0.1, 0.9, 1.0 / 3.0, 0.66, 1.0, 0.0, 0.47)   # unsorted, duplicates, both ends


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


def _same(got, want):
    """equal values (0.0 == -0.0), NaN in the same places"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (got, want)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Resident:
    """a points table and its z_interpolated column in HBM, with room for a result and a workspace"""

    def __init__(self, dbm, pts, zi):
        self.ctx = dbm.default_context()
        self.n = len(zi)
        self.bufs = [self.ctx.malloc(max(a.nbytes, 8)) for a in (pts, zi)] + [self.ctx.malloc(8 * 4100), self.ctx.malloc(dbm.evaluation.DIST_WORKSPACE)]
        self.ctx.upload(self.bufs[0], pts)
        self.ctx.upload(self.bufs[1], zi)

    def close(self):
        for b in self.bufs:
            self.ctx.free(b)


def _call(dbm, which, pts, zi, arg, dev, workspace=True, expect=0):
    """dbm_track_error_quantiles (arg: probabilities) or _histogram (arg: edges) -> (status, result); dev: the device-pointer form;
    workspace False: NULL, the call allocates its own"""
    from deepbedmap_amd import _lib

    pts, zi = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(zi, dtype=np.float64)
    arg = np.ascontiguousarray(arg, dtype=np.float64)
    quant = which == "quantiles"
    count = arg.size if quant else arg.size - 1
    out = np.full(max(count, 1), -77.0) if quant else np.full(max(count, 1), -77, dtype=np.int64)
    fn = getattr(_lib.lib(), "dbm_track_error_" + which)
    res = Resident(dbm, pts, zi)
    try:
        ws = C.c_void_p(res.bufs[3]) if workspace else None
        parg = arg.ctypes.data_as(C.POINTER(C.c_double))
        if dev:
            res.ctx.upload(res.bufs[2], out)
            rc = fn(res.ctx.handle, C.c_void_p(res.bufs[0]), C.c_void_p(res.bufs[1]), res.n, parg, count, C.c_void_p(res.bufs[2]), ws,
                    _lib.DEVICE_PTRS)
            res.ctx.download(res.bufs[2], out=out)
        else:
            rc = fn(res.ctx.handle, _ptr(pts), _ptr(zi), res.n, parg, count, _ptr(out), ws, 0)
    finally:
        res.close()
    assert rc == expect, (rc, _lib.lib().dbm_last_error(res.ctx.handle))
    return out[:max(count, 0)]


def _table(e, seed=0):
    """a points table and a z_interpolated column whose errors are exactly `e` (z = 0: e - 0 = e, -0.0 included)"""
    e = np.asarray(e, dtype=np.float64)
    pts = np.zeros((e.size, 3))
    pts[:, :2] = np.random.default_rng(seed).normal(size=(e.size, 2))
    return pts, e.copy()


def _normal(n, seed):
    """errors in metres with gaps: 1 % NaN in z_interpolated (outside the grid), 1 % NaN in z, a few infinities"""
    r = np.random.default_rng(seed)
    pts = np.zeros((n, 3))
    pts[:, 2] = r.normal(900.0, 300.0, n)
    zi = pts[:, 2] + r.normal(-20.0, 60.0, n)
    zi[r.random(n) < 0.01] = np.nan
    pts[r.random(n) < 0.01, 2] = np.nan
    if n > 10:
        zi[3], pts[7, 2] = np.inf, -np.inf
    return pts, zi


def _low_byte():
    base = np.array([1234.5]).view(np.uint64)[0]
    k = np.random.default_rng(5).permutation(np.concatenate([np.arange(256), np.arange(0, 256, 7)])).astype(np.uint64)
    return (base + k).view(np.float64)


CASES = {
    "n0": lambda: _normal(0, 1),
    "n1": lambda: _table([3.25]),
    "n2": lambda: _table([2.0, -7.5]),
    "all_nan": lambda: _table(np.full(300, np.nan)),
    "share_minus_1": lambda: _normal(THREADS - 1, 2),
    "share": lambda: _normal(THREADS, 3),
    "share_plus_1": lambda: _normal(THREADS + 1, 4),
    "round_plus_1": lambda: _normal(THREADS * BLOCKS + 1, 5),
    "near_1e6": lambda: _normal(1_000_003, 6),
    "low_byte": lambda: _table(_low_byte()),
    "sign_only": lambda: _table(np.concatenate([v := np.random.default_rng(7).normal(0, 100, 50), -v])),
    "denormals_zeros": lambda: _table([5e-324, -5e-324, 0.0, -0.0, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0,
                                       -0.0, -0.0]),
    "three_values": lambda: _table(np.random.default_rng(8).choice([-1.5, 0.0, 2.25], 1000)),
    "top_digit_2": lambda: _table([1.0, -1.0]),
    "top_digit_4": lambda: _table([1e300, -1.0, 1.0, -1e300]),
    "all_equal": lambda: _table(np.full(70, -12.125)),
    "excluded": lambda: (np.array([[0, 0, 1.0], [0, 0, np.nan], [0, 0, 2.0], [0, 0, np.inf], [0, 0, 5.0], [0, 0, 3.0]]),
                         np.array([1.5, 1.0, np.nan, 1.0, -np.inf, 7.0])),
}


def test_constants_of_the_header(dbm):
    import re

    text = open(os.path.join(os.path.dirname(HERE), "include", "dbm.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"\b(DBM_TRACK_[A-Z_]+)\s*=\s*(\d+)", text)}
    assert (flags["DBM_TRACK_DIST_THREADS"], flags["DBM_TRACK_DIST_BLOCKS"]) == (THREADS, BLOCKS)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(CASES))
def test_cases_through_the_c_abi(dbm, name, dev):
    pts, zi = CASES[name]()
    e = td.errors(pts, zi)
    got = _call(dbm, "quantiles", pts, zi, Q16, dev)
    _same(got, td.quantiles(e, Q16))
    if e.size:
        _same(got, np.quantile(e, Q16, method="linear"))
        assert got[1] == e.min() and got[2] == e.max()
    else:
        assert np.isnan(got).all()
    _same(_call(dbm, "quantiles", pts, zi, [0.5], dev), td.quantiles(e, [0.5]))   # one probability: the same passes
    st = dbm.TrackStats(e.size, 0.0, 0.0, e.min() if e.size else np.nan, e.max() if e.size else np.nan, 0.0)
    for bins, rng in ((25, None), (1, None), (25, (-150, 100)), (7, (-1e-309, 1e-309))):
        edges = dbm.evaluation.histogram_edges(st, bins, rng)
        counts = _call(dbm, "histogram", pts, zi, edges, dev)
        _same(counts, td.histogram(e, edges))
        _same(counts, np.histogram(e, bins=bins, range=rng)[0])
        if rng is None:
            assert counts.sum() == e.size


def _lerp_cases():
    """(a, b, g) with m = 2, q = g, where a fused multiply-add would round the interpolation differently: one below g = 0.5 (a + d g)
    and one at or above it (b - d (1 - g))"""
    r, found = np.random.default_rng(77), {}
    for _ in range(10_000):
        a, b = np.sort(r.normal(size=2))
        g = r.random()
        d = b - a
        if g >= 0.5:
            plain, fused = b - d * (1.0 - g), float(Fraction(b) - Fraction(d) * Fraction(1.0 - g))
        else:
            plain, fused = a + d * g, float(Fraction(a) + Fraction(d) * Fraction(g))
        if plain != fused:
            found.setdefault(bool(g >= 0.5), (a, b, g, plain, fused))
        if len(found) == 2:
            return found
    raise AssertionError("no case found")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_interpolation_is_not_fused(dbm, dev):
    for upper, (a, b, g, plain, fused) in sorted(_lerp_cases().items()):
        pts, zi = _table([b, a])
        got = _call(dbm, "quantiles", pts, zi, [g], dev)[0]
        assert got == plain == np.quantile([a, b], g) and got != fused, (upper, got, plain, fused)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_histogram_edges_and_their_neighbours(dbm, dev):
    e = np.arange(-200.0, 151.0)                                     # integer errors: every edge of range (-150, 100), 25 bins is hit
    pts, zi = _table(e)
    pts[:, 2] = 1000.0
    zi = zi + 1000.0                                                  # (exact: the errors are the integers again)
    edges = np.linspace(-150.0, 100.0, 26)
    counts = _call(dbm, "histogram", pts, zi, edges, dev)
    _same(counts, np.histogram(e, bins=25, range=(-150, 100))[0])
    assert counts.sum() == 251 and counts[-1] == 11 and np.all(counts[:-1] == 10)   # outside: dropped; the right edge: the last bin
    edges = np.linspace(-0.7, 0.9, 26)
    beside = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-5.0, 5.0, np.nan]])
    pts, zi = _table(beside)
    counts = _call(dbm, "histogram", pts, zi, edges, dev)
    _same(counts, np.histogram(beside[np.isfinite(beside)], bins=25, range=(-0.7, 0.9))[0])
    _same(counts, td.histogram(td.errors(pts, zi), edges))
    assert counts.sum() == 3 * 26 - 2                                 # all but the two values a step outside the range
    pts, zi = _normal(20_000, 9)
    e = td.errors(pts, zi)
    for bins, rng in ((1, None), (25, None), (4096, None), (4096, (-30.0, 10.0)), (300, (e.min(), 0.0))):
        want, edges = np.histogram(e, bins=bins, range=rng)
        _same(_call(dbm, "histogram", pts, zi, edges, dev, workspace=bins != 25), want)


def test_same_bytes_from_call_to_call_and_in_any_order(dbm):
    pts, zi = _normal(300_000, 10)
    e = td.errors(pts, zi)
    edges = np.histogram_bin_edges(e, bins=25)
    perm = np.random.default_rng(11).permutation(len(zi))
    runs = [(_call(dbm, "quantiles", p, z, Q16, dev, workspace=ws), _call(dbm, "histogram", p, z, edges, dev, workspace=ws))
            for p, z, dev, ws in ((pts, zi, True, True), (pts, zi, True, True), (pts[perm], zi[perm], True, False), (pts, zi, False, True),
                                  (pts, zi, False, False))]
    for q, c in runs[1:]:
        assert q.tobytes() == runs[0][0].tobytes() and c.tobytes() == runs[0][1].tobytes()
    _same(runs[0][0], np.quantile(e, Q16))
    _same(runs[0][1], np.histogram(e, bins=25)[0])


def test_refusals_launch_nothing(dbm):
    from deepbedmap_amd import _lib

    pts, zi = _normal(100, 12)
    last = lambda: _lib.lib().dbm_last_error(dbm.default_context().handle)   # noqa: E731
    for dev in (False, True):
        for bad in ([], [0.5] * 17, [np.nan], [0.5, -0.1], [1.0000001], [0.5, np.inf]):
            out = _call(dbm, "quantiles", pts, zi, bad, dev, expect=1)
            assert b"dbm_track_error_quantiles" in last() and np.all(out == -77.0)   # nothing written
        good = np.linspace(-100.0, 100.0, 26)
        for bad in ([0.0], np.linspace(0.0, 1.0, 4098), [0.0, np.nan, 1.0], [0.0, 0.5, np.inf], [-np.inf, 0.0, 1.0], [0.0, 0.6, 0.5, 1.0],
                    [1.0, 1.0, 1.0], [2.0, 1.0], good[::-1]):
            out = _call(dbm, "histogram", pts, zi, bad, dev, expect=1)
            assert b"dbm_track_error_histogram" in last() and np.all(out == -77)
    # NULL tables with n > 0, NULL probabilities / edges / results
    ctx, L = dbm.default_context(), _lib.lib()
    q, out, cnt = np.array([0.5]), np.zeros(1), np.zeros(25, dtype=np.int64)
    qp, gp = q.ctypes.data_as(C.POINTER(C.c_double)), good.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dbm_track_error_quantiles(ctx.handle, None, _ptr(zi), 100, qp, 1, _ptr(out), None, 0) == 1 and b"NULL" in last()
    assert L.dbm_track_error_quantiles(ctx.handle, _ptr(pts), None, 100, qp, 1, _ptr(out), None, 0) == 1
    assert L.dbm_track_error_quantiles(ctx.handle, _ptr(pts), _ptr(zi), 100, None, 1, _ptr(out), None, 0) == 1
    assert L.dbm_track_error_quantiles(ctx.handle, _ptr(pts), _ptr(zi), 100, qp, 1, None, None, 0) == 1
    assert L.dbm_track_error_quantiles(ctx.handle, _ptr(pts), _ptr(zi), 1 << 40, qp, 1, _ptr(out), None, 0) == 1 and b"2^40" in last()
    assert L.dbm_track_error_histogram(ctx.handle, None, _ptr(zi), 100, gp, 25, _ptr(cnt), None, 0) == 1 and b"NULL" in last()
    assert L.dbm_track_error_histogram(ctx.handle, _ptr(pts), None, 100, gp, 25, _ptr(cnt), None, 0) == 1
    assert L.dbm_track_error_histogram(ctx.handle, _ptr(pts), _ptr(zi), 100, None, 25, _ptr(cnt), None, 0) == 1
    assert L.dbm_track_error_histogram(ctx.handle, _ptr(pts), _ptr(zi), 100, gp, 25, None, None, 0) == 1
    # ... and NULL tables are fine without points
    assert L.dbm_track_error_quantiles(ctx.handle, None, None, 0, qp, 1, _ptr(out), None, 0) == 0 and np.isnan(out[0])
    assert L.dbm_track_error_histogram(ctx.handle, None, None, 0, gp, 25, _ptr(cnt), None, 0) == 0 and not cnt.any()


# ---- the Python layer ----
def _scene(dbm, seed, n=20_000):
    """a grid with holes, and survey points over it: some outside, some without z"""
    r = np.random.default_rng(seed)
    H, W = 64, 96
    grid = (r.normal(0.0, 300.0, (H, W)) + 1000.0).astype(np.float32)
    grid[r.random((H, W)) < 0.03] = np.nan
    geom = dbm.GridGeometry(-1000.0, 5000.0, 250.0, -125.0, "pixel")
    t, s = r.uniform(-1.0, W, n), r.uniform(-1.0, H, n)              # (a band outside the domain: NaN in z_interpolated)
    z = r.normal(950.0, 300.0, n)
    z[r.random(n) < 0.01] = np.nan
    return grid, geom, np.ascontiguousarray(np.stack([geom.x0 + t * geom.dx, geom.y0 + s * geom.dy, z], axis=1))


def _bits(st):
    return np.array(dataclasses.astuple(st), dtype=np.float64).tobytes()


def test_describe_errors_is_describe_of_grdtracks_errors(dbm):
    pd = pytest.importorskip("pandas")
    grid, geom, pts = _scene(dbm, 21)
    for interp in ("bicubic", "nearest"):
        z, st = dbm.grdtrack(pts, grid, geom, interpolation=interp)
        e = z - pts[:, 2]
        assert np.isnan(z).sum() > 100 and np.isnan(pts[:, 2]).sum() > 100
        e = e[np.isfinite(e)]
        want = pd.Series(e).describe()
        for points in (pts, pd.DataFrame(pts, columns=["x", "y", "z"]), dbm.DevicePoints(pts)):
            d = dbm.describe_errors(points, grid, geom, interpolation=interp)
            assert _bits(d.stats) == _bits(st) and d.percentiles == (0.25, 0.5, 0.75) and d.histogram is None
            got = d.as_dict()
            assert list(got) == list(want.index)
            for k in ("count", "min", "25%", "50%", "75%", "max"):
                assert got[k] == want[k], (k, got[k], want[k])
            for k in ("mean", "std"):   # TrackStats' own (bitwise grdtrack's, above); pandas sums in another order
                assert abs(got[k] - want[k]) <= 1e-10 * abs(want[k]), k
        d16 = dbm.describe_errors(pts, dbm.to_device(grid), geom, interpolation=interp, percentiles=Q16)
        _same(d16.quantiles, np.quantile(e, Q16))
        _same(d16.quantiles, td.quantiles(e, Q16))
        assert d16.percentiles == Q16


def test_error_histogram_is_numpys_histogram_of_grdtracks_errors(dbm):
    grid, geom, pts = _scene(dbm, 22)
    z, st = dbm.grdtrack(pts, grid, geom)
    e = z - pts[:, 2]
    e = e[np.isfinite(e)]
    dp = dbm.DevicePoints(pts)
    for bins, rng in ((25, None), (25, (-150, 100)), (1, None), (4096, None), (10, (0.0, 1e-3))):
        want, want_edges = np.histogram(e, bins=bins, range=rng)
        for points in (pts, dp):
            counts, edges = dbm.error_histogram(points, grid, geom, bins=bins, range=rng)
            assert counts.dtype == np.int64 and edges.dtype == np.float64
            _same(edges, want_edges)
            _same(counts, want)
    # the sampled values and the statistics of a later grdtrack on the same DevicePoints are untouched by the calls in between
    z2, st2 = dbm.grdtrack(dp, grid, geom)
    assert z2.tobytes() == z.tobytes() and _bits(st2) == _bits(st)


def test_no_finite_error_and_no_point(dbm):
    grid, geom, pts = _scene(dbm, 23, n=500)
    for table in (pts[:0], np.column_stack([pts[:, :2], np.full(len(pts), np.nan)])):
        d = dbm.describe_errors(table, grid, geom)
        assert d.stats.count == 0 and np.isnan(d.quantiles).all() and np.isnan(d.stats.mean)
        counts, edges = dbm.error_histogram(table, grid, geom)
        _same(edges, np.linspace(0.0, 1.0, 26))
        assert counts.shape == (25,) and not counts.any()
    flat = np.zeros((8, 8), np.float32)                              # every error equal: NumPy's -+ 0.5 range
    table = np.column_stack([pts[:50, :2] * 0.0 + [[-500.0, 4800.0]], np.full(50, 2.5)])
    counts, edges = dbm.error_histogram(table, flat, geom, bins=4)
    want, want_edges = np.histogram(np.full(50, -2.5), bins=4)
    _same(edges, want_edges)
    _same(counts, want)
    assert dbm.describe_errors(table, flat, geom).quantiles == (-2.5, -2.5, -2.5)
    with pytest.raises(ValueError, match="z column"):
        dbm.describe_errors(pts[:, :2], grid, geom)


def test_describe_on_tracks(dbm):
    grid, geom, pts = _scene(dbm, 24)
    other = np.nan_to_num(grid, nan=900.0) + np.float32(35.0)
    grids = {"deepbedmap3": (dbm.to_device(grid), geom), "cubicbedmap": (other, geom)}
    plain = dbm.compare_on_tracks(pts, grids)
    table = dbm.describe_on_tracks(pts, grids)
    both = dbm.describe_on_tracks(dbm.DevicePoints(pts), grids, bins=25, range=(-150, 100), percentiles=(0.5,))
    assert list(table) == list(both) == list(grids)
    for name, (g, _) in grids.items():
        alone = dbm.describe_errors(pts, g, geom)
        assert table[name] == alone and _bits(table[name].stats) == _bits(plain[name]) and table[name].histogram is None
        counts, edges = dbm.error_histogram(pts, g, geom, bins=25, range=(-150, 100))
        _same(both[name].histogram[0], counts)
        _same(both[name].histogram[1], edges)
        assert both[name].quantiles == (alone.quantiles[1],) and counts.sum() > 0
    own = dbm.describe_on_tracks(pts, grids, bins=25)                 # range None: every grid's own (min, max)
    for name in grids:
        counts, edges = own[name].histogram
        assert (edges[0], edges[-1]) == (own[name].stats.min, own[name].stats.max) and counts.sum() == own[name].stats.count
