"""-m gpu: dbm_grid_rescale and dbm_grid_rolling_std (the bicubic BEDMAP2 baseline, the synthetic grid at 250 m, the roughness grids;
reference deepbedmap.py:323-356, paper_figures.py:847-867) through the C ABI and through deepbedmap_amd/comparison.py, against the
float64 NumPy restatement (tests/comparison_restatement.py, pinned to scipy in tests/test_comparison_host.py) rounded to float32.

Bound for rescale: 2^-23 * max|input| absolute on every output -- float64 arithmetic in another order and a recursion warm-up cut at
|pole|^32 = 5e-19 sit far below half a float32 ulp at the data's magnitude, so only the final rounding can differ.
Bound for roughness: one float32 ulp of the expected value, exactly 0 on a constant plateau, NaN exactly where the restatement has NaN.
Derived, not measured; every output is compared (the large-plane test compares the corner that lies past 2^31 elements)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import comparison_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = [4, 2, 1 / 2.5, (3, 0.5)]
ORDERS = [1, 3]
# (1100, 700): several chunks of the prefilter in both axes (256 rows, 128 columns), multiples of no tile or chunk size;
# the others: odd sizes and axes shorter than the recursion's warm-up
SHAPES = [(1100, 700), (37, 53), (2, 3), (3, 5), (5, 2), (5, 301)]


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


def _grid(shape, kind, seed):
    r = np.random.default_rng(seed)
    g = r.random(shape) if kind == "unit" else r.uniform(-2000.0, 2000.0, shape)
    return g.astype(np.float32)


def _abi_rescale(dbm, x, out_shape, order, anti_aliasing=True, clip=True, as_int=False):
    from deepbedmap_amd import _lib

    src = dbm.to_device(x)
    out = dbm.DeviceArray(out_shape, src.ctx)
    rc = _lib.lib().dbm_grid_rescale(src.ctx.handle, C.c_void_p(src.ptr), x.shape[0], x.shape[1], out_shape[0], out_shape[1], order,
                                     int(anti_aliasing), int(clip), int(as_int), C.c_void_p(out.ptr))
    assert rc == 0, _lib.lib().dbm_last_error(src.ctx.handle)
    return out.get()


def _abi_std(dbm, x, window):
    from deepbedmap_amd import _lib

    src = dbm.to_device(x)
    out = dbm.DeviceArray(x.shape, src.ctx)
    rc = _lib.lib().dbm_grid_rolling_std(src.ctx.handle, C.c_void_p(src.ptr), x.shape[0], x.shape[1], window, C.c_void_p(out.ptr))
    assert rc == 0, _lib.lib().dbm_last_error(src.ctx.handle)
    return out.get()


def _rescale_close(got, want, x):
    bound = 2.0 ** -23 * float(np.abs(x).max())
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("max error", err.max(), "bound", bound, "values", err.size, "differing", int((err > 0).sum()))
    assert np.all(err <= bound), (err.max(), bound)


def _std_close(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    m = ~np.isnan(want)
    err = np.abs(got[m].astype(np.float64) - want[m].astype(np.float64))
    ulp = np.spacing(np.abs(want[m])).astype(np.float64)
    print("max error in ulps", (err / ulp).max() if err.size else 0.0, "values", int(m.sum()))
    assert np.all(err <= ulp), (err / ulp).max()


def _cases():
    for shape in SHAPES:
        for scale in SCALES:
            if min(cr.output_shape(shape, scale)) < 1:
                continue
            for order in ORDERS:
                yield shape, scale, order


@pytest.mark.parametrize("kind", ["unit", "dem"])
@pytest.mark.parametrize("shape,scale,order", list(_cases()))
def test_rescale_matches_the_restatement(dbm, shape, scale, order, kind):
    x = _grid(shape, kind, seed=shape[0] + 7 * shape[1] + order)
    out_shape = cr.output_shape(shape, scale)
    want = cr.rescale(x, scale, order)
    _rescale_close(_abi_rescale(dbm, x, out_shape, order), want, x)
    got = dbm.rescale(x, scale, order=order)
    assert isinstance(got, dbm.DeviceArray) and got.shape == out_shape
    _rescale_close(got.get(), want, x)


@pytest.mark.parametrize("shape", [(37, 53), (300, 417)])
@pytest.mark.parametrize("order", ORDERS)
def test_rescale_switches(dbm, shape, order):
    x = _grid(shape, "dem", seed=order)
    for scale in (4, 1 / 2.5):
        out_shape = cr.output_shape(shape, scale)
        for anti_aliasing, clip, as_int in [(True, False, False), (True, True, True), (False, True, False), (False, False, True)]:
            want = cr.rescale(x, scale, order, anti_aliasing=anti_aliasing, clip=clip, as_int=as_int)
            _rescale_close(_abi_rescale(dbm, x, out_shape, order, anti_aliasing, clip, as_int), want, x)
            _rescale_close(dbm.rescale(x, scale, order=order, anti_aliasing=anti_aliasing, clip=clip, as_int=as_int).get(), want, x)
    free = dbm.rescale(x, 4, order=3, clip=False).get()
    held = dbm.rescale(x, 4, order=3, clip=True).get()
    assert free.max() > x.max() and held.max() <= x.max() and held.min() >= x.min()   # the clip is not a formality


def test_repeat_calls_ranks_and_device_inputs_give_the_same_bits(dbm):
    x = _grid((530, 390), "dem", seed=3)
    first = dbm.rescale(x, 4, order=3).get()
    assert first.shape == (2120, 1560)
    dbm.rescale(_grid((90, 1200), "unit", seed=4), 1 / 2.5, order=1)   # another shape in between: the workspace is reused and regrown
    for _ in range(2):
        assert np.array_equal(dbm.rescale(x, 4, order=3).get(), first)
    dx = dbm.to_device(x)
    assert np.array_equal(dbm.rescale(dx, 4, order=3).get(), first)
    assert np.array_equal(dx.get(), x)                                  # read in place, left as it was
    for lead in ((1,), (1, 1)):
        got = dbm.rescale(dbm.to_device(x.reshape(lead + x.shape)), 4, order=3)
        assert got.shape == lead + (2120, 1560) and np.array_equal(got.get().reshape(2120, 1560), first)
        assert dbm.rescale(x.reshape(lead + x.shape), 4, order=3).shape == lead + (2120, 1560)
    r1 = dbm.standard_deviation_2d(x, 5).get()
    assert np.array_equal(dbm.standard_deviation_2d(x, 5).get(), r1)
    assert np.array_equal(dbm.standard_deviation_2d(dx, 5).get(), r1)
    got = dbm.standard_deviation_2d(dbm.to_device(x[None, None]), 5)
    assert got.shape == (1, 1) + x.shape and np.array_equal(got.get()[0, 0], r1)


def _rough_grid(shape, seed, frame=0):
    r = np.random.default_rng(seed)
    g = r.uniform(-2000.0, 2000.0, shape)
    g[r.random(shape) < 0.05] = np.nan
    g[shape[0] // 3:shape[0] // 3 + 70, shape[1] // 2:shape[1] // 2 + 80] = np.nan   # windows without a valid node (up to window 63)
    g[10:10 + 70, 5:5 + 70] = -321.25                                                 # a constant plateau
    if frame:
        g[:frame] = g[-frame:] = np.nan
        g[:, :frame] = g[:, -frame:] = np.nan
    return g.astype(np.float32)


@pytest.mark.parametrize("window", [1, 3, 5, 9, 63])
def test_roughness_matches_the_restatement(dbm, window):
    g = _rough_grid((203, 331), seed=window)     # multiples of no tile size
    want = cr.standard_deviation_2d(g, window)
    assert np.isnan(want).any() and np.all(want[10 + 32:10 + 38, 5 + 32:5 + 38] == 0.0)
    for got in (_abi_std(dbm, g, window), dbm.standard_deviation_2d(g, window).get()):
        _std_close(got, want)
        assert np.all(got[10 + 32:10 + 38, 5 + 32:5 + 38] == 0.0)   # exactly 0 on the plateau
    if window > 1:
        assert np.nanmax(want) > 100.0


@pytest.mark.parametrize("window", [3, 5])
def test_roughness_of_a_canvas_with_its_nan_frame(dbm, window):
    g = _rough_grid((76 * 2 + 350, 76 * 2 + 420), seed=10 + window, frame=76)   # predict_tiled's canvas: 76 pixels of NaN all round
    want = cr.standard_deviation_2d(g, window)
    assert np.isnan(want[:70]).all() and np.isfinite(want[76 - window // 2, 200])
    _std_close(dbm.standard_deviation_2d(g, window).get(), want)
    _std_close(_abi_std(dbm, g, window), want)
    unit = np.random.default_rng(2).random((64, 65)).astype(np.float32)
    _std_close(dbm.standard_deviation_2d(unit, window).get(), cr.standard_deviation_2d(unit, window))


def test_cubic_bedmap(dbm):
    X = np.random.default_rng(8).uniform(-2500.0, 1500.0, (1, 1, 22, 31)).astype(np.float32)
    want = cr.cubic_bedmap(X)
    assert want.shape == (1, 1, 80, 116)
    for arg in (X, dbm.to_device(X)):
        got = dbm.cubic_bedmap(arg)
        assert isinstance(got, dbm.DeviceArray) and got.shape == (1, 1, 80, 116)
        _rescale_close(got.get(), want, X)
    # the int32 cast is part of it, and the result stays inside the cast interior's range
    inner = X[0, 0, 1:-1, 1:-1].astype(np.int32)
    assert got.get().min() >= inner.min() and got.get().max() <= inner.max()
    assert np.abs(got.get() - cr.rescale(X[0, 0, 1:-1, 1:-1], 4, order=3)[None, None]).max() > 0.01


def test_compare_on_tracks_equals_separate_grdtrack_calls(dbm):
    r = np.random.default_rng(12)
    X = r.uniform(-2000.0, 2000.0, (1, 1, 22, 31)).astype(np.float32)
    bound = (-1000.0, -2000.0, -1000.0 + 29 * 1000.0, -2000.0 + 20 * 1000.0)
    cubic = dbm.cubic_bedmap(X)
    H, W = cubic.shape[-2:]
    model = dbm.to_device(cubic.get() + r.normal(0.0, 30.0, cubic.shape).astype(np.float32))
    rough = dbm.standard_deviation_2d(model, 5)
    geom = dbm.GridGeometry.from_bounds(bound, H, W)
    low = X[0, 0, 1:-1, 1:-1]
    low_geom = dbm.GridGeometry.from_bounds(bound, 20, 29)
    pts = np.stack([r.uniform(bound[0] - 500.0, bound[2] + 500.0, 5000), r.uniform(bound[1] - 500.0, bound[3] + 500.0, 5000),
                    r.uniform(-2000.0, 2000.0, 5000)], axis=1)
    grids = {"deepbedmap3": (model, geom), "cubicbedmap": (cubic, geom), "roughness": (rough, geom), "bedmap2": (low, low_geom)}
    table = dbm.compare_on_tracks(pts, grids)
    assert list(table) == list(grids)
    for name, (g, gg) in grids.items():
        _, want = dbm.grdtrack(pts, g, gg, return_values=False)
        assert isinstance(table[name], dbm.TrackStats) and table[name].count > 3000
        bits = lambda st: np.array(dataclasses.astuple(st), dtype=np.float64).view(np.uint64)   # noqa: E731
        assert np.array_equal(bits(table[name]), bits(want)), (name, table[name], want)
    again = dbm.compare_on_tracks(dbm.DevicePoints(pts), grids, interpolation="bilinear")
    assert again["cubicbedmap"] == dbm.grdtrack(pts, cubic, geom, interpolation="bilinear", return_values=False)[1]
    assert np.isfinite(table["deepbedmap3"].rmse - table["cubicbedmap"].rmse)


def test_refusals_name_the_entry_point(dbm):
    from deepbedmap_amd import _lib

    lib = _lib.lib()
    ctx = _lib.default_context()
    a = dbm.to_device(np.zeros((8, 9), dtype=np.float32))
    b = dbm.DeviceArray((16, 18), ctx)
    p = lambda d: C.c_void_p(d.ptr)   # noqa: E731

    def refused(rc, name):
        assert rc == 1, rc
        assert name in lib.dbm_last_error(ctx.handle).decode()

    for order in (0, 2, 4, 5, -1):
        refused(lib.dbm_grid_rescale(ctx.handle, p(a), 8, 9, 16, 18, order, 1, 1, 0, p(b)), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, p(a), 1, 72, 16, 18, 1, 1, 1, 0, p(b)), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, p(a), 72, 1, 16, 18, 1, 1, 1, 0, p(b)), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, p(a), 8, 9, 0, 18, 1, 1, 1, 0, p(b)), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, p(a), 8, 9, 16, -1, 3, 1, 1, 0, p(b)), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, None, 8, 9, 16, 18, 3, 1, 1, 0, p(b)), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, p(a), 8, 9, 16, 18, 3, 1, 1, 0, None), "dbm_grid_rescale")
    refused(lib.dbm_grid_rescale(ctx.handle, p(a), 8, 9, 8, 9, 3, 1, 1, 0, p(a)), "dbm_grid_rescale")
    o = dbm.DeviceArray((8, 9), ctx)
    for window in (0, 2, 4, 64, 65, -3):
        refused(lib.dbm_grid_rolling_std(ctx.handle, p(a), 8, 9, window, p(o)), "dbm_grid_rolling_std")
    refused(lib.dbm_grid_rolling_std(ctx.handle, p(a), 0, 9, 3, p(o)), "dbm_grid_rolling_std")
    refused(lib.dbm_grid_rolling_std(ctx.handle, p(a), 8, 0, 3, p(o)), "dbm_grid_rolling_std")
    refused(lib.dbm_grid_rolling_std(ctx.handle, None, 8, 9, 3, p(o)), "dbm_grid_rolling_std")
    refused(lib.dbm_grid_rolling_std(ctx.handle, p(a), 8, 9, 3, None), "dbm_grid_rolling_std")
    refused(lib.dbm_grid_rolling_std(ctx.handle, p(a), 8, 9, 3, p(a)), "dbm_grid_rolling_std")
    # nothing was launched, the context still works
    assert lib.dbm_grid_rolling_std(ctx.handle, p(a), 8, 9, 3, p(o)) == 0
    assert np.all(o.get() == 0.0)


def test_planes_past_2_31_elements(dbm):
    """11 600 x 11 600 -> 46 400 x 46 400 (2.15e9 values, the last 118 rows lie past element 2^31), order 3, then the roughness of that
    output.  Compared: the last 400 rows x 400 columns of both, against the restatement on the input's last 300 x 300 nodes (the
    prefilter's influence decays as 0.268^k: the crop's far edge, 200 input nodes from the compared block, is immaterial; the clip's
    range is the whole input's).  Needs 20.3 GB of HBM (input 0.54, two float64 planes 2.15, output 8.61, roughness 8.61, the compared
    blocks) and 1.1 GB of host memory."""
    from deepbedmap_amd import _lib

    lib = _lib.lib()
    n, crop, block = 11600, 300, 400
    r = np.random.default_rng(99)
    x = r.uniform(-2000.0, 2000.0, (n, n)).astype(np.float32)
    dx = dbm.to_device(x)
    out = dbm.rescale(dx, 4, order=3)
    N = 4 * n
    assert out.shape == (N, N) and out.size > 2 ** 31
    rough = dbm.standard_deviation_2d(out, 5)

    def corner(d):
        piece = dbm.DeviceArray((block, block), d.ctx)
        off = 4 * ((N - block) * N + (N - block))
        _lib.check(lib.dbm_memcpy2d_d2d(d.ctx.handle, C.c_void_p(piece.ptr), 4 * block, C.c_void_p(d.ptr + off), 4 * N, 4 * block, block),
                   d.ctx.handle)
        return piece.get()

    got, got_rough = corner(out), corner(rough)
    del out, rough
    xc = x[-crop:, -crop:]
    want64 = np.clip(cr.rescale64(xc, 4, order=3, clip=False), float(x.min()), float(x.max()))
    want = want64.astype(np.float32)[-block:, -block:]
    _rescale_close(got, want, x)
    # the roughness of the GPU's own output block (its window reaches 2 nodes beyond the compared interior)
    _std_close(got_rough[2:, 2:], cr.standard_deviation_2d(got, 5)[2:, 2:])
