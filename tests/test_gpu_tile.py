"""-m gpu: dbm_grid_tile and dbm_grid_filled_windows (tiles cut from resident rasters, the fully filled windows of a grid) against
the float64 NumPy restatement of their semantics (tests/tile_restatement.py, itself checked against scipy's interpn in
tests/test_tile_host.py), and the layer built on them (deepbedmap_amd/tiling.py: selective_tile, get_window_bounds,
get_deepbedmap_model_inputs, tile_training_set; reference data_prep.py:501-741, 757-771, 880-911, deepbedmap.py:132-213).

Tolerance of a bilinear value against the restatement's float32 result: one float32 ulp plus 16 * 2^-53 * max|z| -- the float64
rounding of a four-term sum of products whose terms may cancel (three roundings per term, three per sum, on magnitudes up to max|z|).
Derived, not measured; every output is compared."""
import ctypes as C
import gc
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tile_restatement as tl  # noqa: E402
import track_restatement as tr  # noqa: E402
from test_tile_host import PAIRINGS, _raster, _windows  # noqa: E402  (geometries whose coordinates are exact in float64)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(autouse=True)
def _reset_config(dbm):
    dbm.global_config.train = True
    dbm.global_config.enable_backprop = True
    dbm.global_config.dtype = "float32"
    yield


def _close(got, want, zmax, extra=0.0):
    """identical NaN pattern; |got - want| <= one float32 ulp of want + 16 * 2^-53 * max|z| (+ extra) on EVERY other output"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    m = ~np.isnan(want)
    err = np.abs(got[m].astype(np.float64) - want[m].astype(np.float64))
    tol = np.spacing(np.abs(want[m])).astype(np.float64) + 16.0 * 2.0 ** -53 * zmax + extra
    print("max error", err.max() if err.size else 0.0, "of tolerance", (err / tol).max() if err.size else 0.0, "values", int(m.sum()))
    assert np.all(err <= tol), (err.max(), (err / tol).max())


def _zmax(g):
    return float(np.nanmax(np.abs(g)))


def _aligned_windows(geom, H, W, npix, n, seed):
    """n windows of npix x npix nodes that cut the grid at its nodes; the first and the last one touch opposite corners."""
    x0, y0, dx, dy = geom
    d = abs(dx)
    west, north = min(x0, x0 + (W - 1) * dx) - d / 2, max(y0, y0 + (H - 1) * dy) + d / 2
    r = np.random.default_rng(seed)
    cols = np.concatenate([[0], r.integers(0, W - npix + 1, n - 2), [W - npix]])
    rows = np.concatenate([[0], r.integers(0, H - npix + 1, n - 2), [H - npix]])
    return [(west + c * d, north - (rw + npix) * d, west + (c + npix) * d, north - rw * d) for rw, c in zip(rows, cols)]


@pytest.mark.parametrize("north_up", [True, False])
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_parity_with_the_restatement_in_both_modes(dbm, pairing, north_up):
    d, res = pairing
    H, W = 230, 310
    g, geom = _raster(H, W, d, seed=int(d) + 2 * north_up, north_up=north_up, nans=900)
    raster = dbm.Raster(g, dbm.GridGeometry(*geom))
    # bilinear: windows on and off the nodes, on the first and the last node, over every edge, one outside
    for npix in (7, 11):
        wins = _windows(geom, H, W, res, npix, seed=npix) + _windows(geom, H, W, res, npix, seed=npix + 100)
        got = dbm.selective_tile(raster, wins, resolution=res).get()
        want, _ = tl.tile(g, (H, W), geom, wins, resolution=res)
        assert got.shape == (len(wins), 1, npix, npix) and np.isnan(want).any() and (~np.isnan(want)).any()
        _close(got, want, _zmax(g))
    # slicing at the raster's own spacing: a pure copy, NaN nodes included
    wins = _aligned_windows(geom, H, W, 36, 40, seed=3)
    got = dbm.selective_tile(raster, wins, interpolate=False).get()
    want, _ = tl.tile(g, (H, W), geom, wins, interpolate=False)
    assert got.shape == (40, 1, 36, 36)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and the bilinear cut of the same windows samples the nodes themselves
    _close(dbm.selective_tile(raster, wins).get(), tl.tile(g, (H, W), geom, wins)[0], _zmax(g))


def test_parity_on_an_inexact_geometry(dbm):
    """dx = 0.1 at offsets of 10^6: node and sample coordinates are rounded.  No NaN, every sample at least 10^-6 of a cell away from
    every node and inside the raster, so the cell cannot differ; what remains is the rounding of t: each of (c - g[i]) and
    (g[i+1] - g[i]) carries the coordinates' rounding, 2^-52 |coordinate| relative to a cell of dx, in both directions."""
    H, W = 200, 260
    r = np.random.default_rng(77)
    g = r.normal(0.0, 300.0, (H, W)).astype(np.float32)
    geom = (1_000_000.03, 2_000_000.07, 0.1, -0.1)
    raster = dbm.Raster(g, dbm.GridGeometry(*geom))
    npix, wins = 9, []
    for _ in range(60):
        c, rw = r.integers(1, W - npix - 2), r.integers(1, H - npix - 2)
        fx, fy = r.uniform(0.2, 0.8, 2)
        left = geom[0] + (c + fx) * 0.1 - 0.05
        top = geom[1] - (rw + fy) * 0.1 + 0.05
        wins.append((left, top - npix * 0.1 - 1e-6, left + npix * 0.1 + 1e-6, top))    # (int() of the size must not truncate to 8)
    padded = tl.pad_windows(wins)
    gy, _ = tl.axis(geom[1], geom[3], H)
    gx, _ = tl.axis(geom[0], geom[2], W)
    for wb in padded:
        ys, xs = tl.window_coords(wb, 0.1, npix, npix)
        for c, ax in ((ys, gy), (xs, gx)):
            _, t, bad = tl.cells(c, ax)
            assert not bad.any() and t.min() >= 1e-6 and t.max() <= 1 - 1e-6
    assert tl.tile_shape(padded, 0.1) == (npix, npix)
    got = dbm.selective_tile(raster, wins).get()
    want, _ = tl.tile(g, (H, W), geom, wins)
    assert not np.isnan(want).any()
    extra = 4.0 * 2.0 ** -52 * (2_000_000.07 / 0.1) * float(g.max() - g.min())
    _close(got, want, _zmax(g), extra=extra)


def _training_rasters(dbm, seed=1):
    """Small synthetic stand-ins for the five rasters on one area of 60 km x 50 km: BEDMAP2 and accumulation at 1000 m, REMA at 100 m,
    velocities at 450 m, one groundtruth grid at 250 m with a NaN blob."""
    r = np.random.default_rng(seed)
    west, south, east, north = -1_600_000.0, -300_000.0, -1_540_000.0, -250_000.0

    def make(d, scale, pad=3000.0):
        W, H = int((east - west + 2 * pad) / d) + 2, int((north - south + 2 * pad) / d) + 2
        geom = dbm.GridGeometry(west - pad + d / 2 - (450.0 / 4 if d == 450.0 else 0.0), north + pad - d / 2, d, -d)
        return (r.random((H, W), dtype=np.float32) * scale).astype(np.float32), geom

    out = {}
    for name, d in (("bedmap2", 1000.0), ("rema", 100.0), ("velocity_x", 450.0), ("velocity_y", 450.0), ("accumulation", 1000.0)):
        g, geom = make(d, 1.0)
        out[name] = (g, geom)
    W, H = int((east - west) / 250.0), int((north - south) / 250.0)
    hi = r.random((H, W), dtype=np.float32)
    hi[60:95, 100:170] = np.nan
    hi[H - 1, W - 1] = np.nan
    out["highres"] = (hi, dbm.GridGeometry(west + 125.0, north - 125.0, 250.0, -250.0))
    return out


def test_training_set_shapes_and_one_minibatch(dbm):
    data = _training_rasters(dbm)
    rasters = {k: dbm.Raster(g, geom) for k, (g, geom) in data.items()}
    hi, higeom = data["highres"]
    bounds = dbm.get_window_bounds(rasters["highres"], step=12)
    flags = tl.filled_windows(hi, tuple(higeom.as_array()), 36, 12)
    assert bounds == dbm.tiling.bounds_from_flags(flags, higeom, hi.shape, 36, 12) and 0 < len(bounds) < flags.size
    n = len(bounds)
    half = n // 2
    # two groundtruth "grids" (the same raster twice, each with its share of the windows), concatenated like data_prep.py:757-761
    ds = dbm.tile_training_set([(rasters["highres"], bounds[:half]), (rasters["highres"], bounds[half:])], rasters["bedmap2"],
                               rasters["rema"], rasters["velocity_x"], rasters["velocity_y"], rasters["accumulation"])
    assert {k: v.shape for k, v in ds.items()} == {"X": (n, 1, 11, 11), "W1": (n, 1, 110, 110), "W2": (n, 2, 22, 22),
                                                    "W3": (n, 1, 11, 11), "Y": (n, 1, 36, 36)}
    assert all(isinstance(v, dbm.DeviceArray) for v in ds.values())

    def want(name, **kw):
        g, geom = data[name]
        return tl.tile(g, g.shape, tuple(geom.as_array()), bounds, **kw)[0]

    _close(ds["X"].get(), want("bedmap2", padding=1000), 1.0)
    _close(ds["W1"].get(), want("rema", padding=1000), 1.0)
    _close(ds["W3"].get(), want("accumulation", padding=1000), 1.0)
    w2 = ds["W2"].get()     # VX and VY written through the window stride into the two channels
    _close(np.ascontiguousarray(w2[:, :1]), want("velocity_x", padding=1000, resolution=500), 1.0)
    _close(np.ascontiguousarray(w2[:, 1:]), want("velocity_y", padding=1000, resolution=500), 1.0)
    y = ds["Y"].get()
    assert np.array_equal(y.view(np.uint32), want("highres", interpolate=False).view(np.uint32)) and not np.isnan(y).any()
    # one call each gives the same arrays (the reference's five selective_tile calls)
    one = dbm.selective_tile(rasters["rema"], bounds, padding=1000)
    assert one.shape == (n, 1, 110, 110) and np.array_equal(one.get().view(np.uint32), ds["W1"].get().view(np.uint32))
    out = dbm.DeviceArray((n, 2, 22, 22))
    for ch, name in enumerate(("velocity_x", "velocity_y")):
        assert dbm.selective_tile(rasters[name], bounds, padding=1000, resolution=500, out=out, channel=ch) is out
    assert np.array_equal(out.get().view(np.uint32), w2.view(np.uint32))
    with pytest.raises(ValueError, match="out has shape"):
        dbm.selective_tile(rasters["rema"], bounds, padding=1000, out=out)
    with pytest.raises(ValueError, match="channel 2"):
        dbm.selective_tile(rasters["velocity_x"], bounds, padding=1000, resolution=500, out=out, channel=2)
    # the dict is a dataset: split, iterate, train one minibatch
    np.random.seed(5)
    train_iter, n_train, dev_iter, n_dev = dbm.get_train_dev_iterators(ds, first_size=n - 4, batch_size=4, seed=42)
    assert n_train == n - 4 and n_dev == 4
    g, g_opt, d, d_opt = dbm.compile_srgan_model(num_residual_blocks=1, residual_scaling=0.3, learning_rate=5e-4)
    batch = dbm.device_batch(dbm.concat_examples(train_iter.dataset, train_iter.next()), g.ctx)
    metrics = dbm.train_minibatch(batch, g, g_opt, d, d_opt)
    assert len(metrics) == 5 and all(np.isfinite(metrics)), metrics


def test_masking_gap_filling_counts_and_the_warning(dbm):
    H, W = 60, 80
    r = np.random.default_rng(8)
    g = r.normal(1000.0, 300.0, (H, W)).astype(np.float32)
    nodata = -9999.0
    g[5:9, 5:30] = nodata                                   # a stretch of nodata: tiles inside it interpolate to exactly nodata
    g[20, 20] = np.float32(nodata * (1 + 5e-6))             # within the band
    g[22, 40] = np.float32(nodata * (1 + 2e-5))             # just outside, below
    g[24, 60] = np.float32(nodata * (1 - 2e-5))             # just outside, above
    g[40, 10] = np.nan
    geom = (500.0, 59500.0, 1000.0, -1000.0)
    wins = _aligned_windows(geom, H, W, 10, 60, seed=4) + [(-4000.0, 50000.0, 6000.0, 60000.0), (70000.0, -3000.0, 80000.0, 7000.0)]
    kinds = [dict(interpolate=False), dict(), dict(padding=500)]      # copies, on-node samples, mid-cell samples
    for kw in kinds:
        if kw.get("interpolate") is False:
            use = wins[:-2]
        else:
            use = wins
        for fill_nan in (False, True):
            for gapfiller in (None, -5000.0, 0.0):
                raster = dbm.Raster(g, dbm.GridGeometry(*geom), nodata=nodata)
                want, counts = tl.tile(g, (H, W), geom, use, nodata=nodata, gapfiller=gapfiller, fill_nan=fill_nan, **kw)
                assert counts.sum() > 0
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    got = dbm.selective_tile(raster, use, gapfiller=gapfiller, fill_nan=fill_nan, **kw).get()
                _close(got, want, _zmax(g))
                if gapfiller is None:   # the reference's WARN, with the affected tiles
                    assert len(caught) == 1 and "gapfiller" in str(caught[0].message)
                    assert str(np.flatnonzero(counts).tolist()) in str(caught[0].message)
                else:
                    assert not caught
                    masked = tl.tile(g, (H, W), geom, use, nodata=nodata, gapfiller=None, fill_nan=fill_nan, **kw)[0] != want
                    assert (got[masked & ~np.isnan(want)] == np.float32(gapfiller)).all()
                if fill_nan and gapfiller is not None:
                    assert not np.isnan(got).any()
                # the counts through the C entry point equal the restatement's, window by window
                assert np.array_equal(_counts(dbm, raster, use, gapfiller, fill_nan, **kw), counts)
    # the three hand-placed nodes, sliced: only the one within the band is masked
    raster = dbm.Raster(g, dbm.GridGeometry(*geom), nodata=nodata)
    whole = [(0.0, 0.0, 80000.0, 60000.0)]
    got = dbm.selective_tile(raster, whole, gapfiller=7.0, interpolate=False).get()[0, 0]
    assert got[20, 20] == 7.0 and got[22, 40] == g[22, 40] and got[24, 60] == g[24, 60] and np.isnan(got[40, 10]) and (got[5:9, 5:30] == 7.0).all()
    # no nodata, or a NaN nodata: nothing is masked, nothing warned; fill_nan alone fills the edge and the NaN node
    for nd in (None, float("nan")):
        raster = dbm.Raster(g, dbm.GridGeometry(*geom), nodata=nd)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = dbm.selective_tile(raster, wins, gapfiller=3.0).get()
        _close(got, tl.tile(g, (H, W), geom, wins, nodata=nd, gapfiller=3.0)[0], _zmax(g))
        assert np.isnan(got[-1]).any() and (got[0] == g[:10, :10]).all()
        got = dbm.selective_tile(raster, wins, gapfiller=3.0, fill_nan=True).get()
        _close(got, tl.tile(g, (H, W), geom, wins, nodata=nd, gapfiller=3.0, fill_nan=True)[0], _zmax(g))
        assert not np.isnan(got).any() and (got[-1] == 3.0).any()


def _counts(dbm, raster, wins, gapfiller, fill_nan, padding=0, interpolate=True):
    plan = dbm.tiling._plan(raster, wins, padding, None, gapfiller, interpolate)
    out = dbm.DeviceArray((len(wins), 1, plan[3], plan[4]))
    return dbm.tiling._cut(raster, plan, gapfiller, fill_nan, out.ptr, plan[3] * plan[4], want_counts=True)


@pytest.mark.parametrize("case", [(120, 150, 36, 3), (100, 131, 36, 5), (77, 90, 8, 3), (64, 64, 64, 1), (301, 1000, 36, 3), (50, 9000, 10, 4)])
def test_filled_window_flags(dbm, case):
    H, W, size, step = case
    r = np.random.default_rng(H + W)
    base = r.normal(0, 1, (H, W)).astype(np.float32)
    variants = []
    g = base.copy()
    g[H - 1, W - 1] = np.nan                 # one NaN in the very last row and column
    variants.append(g)
    g = base.copy()
    for _ in range(6):                       # blobs
        r0, c0 = r.integers(0, H), r.integers(0, W)
        g[r0:r0 + r.integers(1, 9), c0:c0 + r.integers(1, 30)] = np.nan
    g[0, 0] = np.nan
    variants.append(g)
    variants.append(base)                    # no NaN at all
    for g in variants:
        for dy in (-250.0, 250.0):           # both row orders
            for dx in (250.0, -250.0):
                geom = dbm.GridGeometry(1000.0, 2000.0, dx, dy)
                want = tl.filled_windows(g, (1000.0, 2000.0, dx, dy), size, step)
                got = _flags(dbm, g, geom, size, step)
                assert got.shape == want.shape and np.array_equal(got, want), (int(got.sum()), int(want.sum()))
                bounds = dbm.get_window_bounds(dbm.Raster(g, geom), height=size, width=size, step=step)
                assert bounds == dbm.tiling.bounds_from_flags(want, geom, (H, W), size, step)


def _flags(dbm, g, geom, size, step):
    from deepbedmap_amd import _lib

    H, W = g.shape
    dg = dbm.to_device(g)
    ny, nx = (H - size) // step + 1, (W - size) // step + 1
    fdev = dg.ctx.malloc(ny * nx)
    try:
        _lib.check(_lib.lib().dbm_grid_filled_windows(dg.ctx.handle, C.c_void_p(dg.ptr), H, W, size, step, int(geom.dy > 0), int(geom.dx < 0),
                                                      C.c_void_p(fdev)), dg.ctx.handle)
        out = np.empty((ny, nx), np.uint8)
        _lib.check(_lib.lib().dbm_memcpy_d2h(dg.ctx.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(fdev), out.nbytes), dg.ctx.handle)
    finally:
        dg.ctx.free(fdev)
    return out


def _tile_abi(dbm, dgrid, H, W, geom, windows, n, mode, res, out_h, out_w, out, stride, nodata=None, fill=None, fill_nan=0, counts=None):
    from deepbedmap_amd import _lib

    g = np.asarray(geom, dtype=np.float64)
    return _lib.lib().dbm_grid_tile(dgrid.ctx.handle, C.c_void_p(dgrid.ptr) if dgrid.ptr else None, H, W, g.ctypes.data_as(C.POINTER(C.c_double)),
                                    windows.ctypes.data_as(C.c_void_p) if windows is not None else None, n, mode, res, out_h, out_w,
                                    None if nodata is None else C.byref(C.c_double(nodata)), None if fill is None else C.byref(C.c_float(fill)),
                                    fill_nan, C.c_void_p(out.ptr) if out is not None else None, stride, counts)


def test_same_bits_from_call_to_call_and_edge_values_of_n(dbm):
    H, W = 150, 170
    g, geom = _raster(H, W, 100.0, seed=9, nans=200)
    wins = _windows(geom, H, W, 100.0, 11, seed=1) * 3
    host_raster = dbm.Raster(g, dbm.GridGeometry(*geom), nodata=-9999.0)
    resident = dbm.Raster(dbm.to_device(g), dbm.GridGeometry(*geom), nodata=-9999.0)
    assert resident.device() is resident._dev
    runs = [dbm.selective_tile(r, wins, gapfiller=1.0, fill_nan=fn).get() for r in (host_raster, resident, resident, host_raster) for fn in (False, True)]
    for k in (2, 4, 6):
        assert np.array_equal(runs[k].view(np.uint32), runs[0].view(np.uint32))
        assert np.array_equal(runs[k + 1].view(np.uint32), runs[1].view(np.uint32))
    assert host_raster._host is None and host_raster.device() is host_raster._dev      # uploaded once
    # n = 1 through the Python layer, n = 0 through the C entry point (a no-op that succeeds, even with NULL pointers)
    one = dbm.selective_tile(resident, wins[:1]).get()
    assert np.array_equal(one.view(np.uint32), dbm.selective_tile(resident, wins).get()[:1].view(np.uint32))
    dgrid = resident.device()
    out = dbm.to_device(np.full((2, 11, 11), 5.0, np.float32))
    assert _tile_abi(dbm, dgrid, H, W, geom, np.zeros((0, 4)), 0, 1, 100.0, 11, 11, out, 121) == 0
    assert _tile_abi(dbm, dgrid, H, W, geom, None, 0, 1, 100.0, 11, 11, None, 121) == 0
    assert (out.get() == 5.0).all()


def test_refusals_launch_nothing(dbm):
    from deepbedmap_amd import _lib

    H, W = 40, 50
    g = np.arange(H * W, dtype=np.float32).reshape(H, W)
    geom = (500.0, 39500.0, 1000.0, -1000.0)
    dgrid = dbm.to_device(g)
    out = dbm.to_device(np.full((2, 9, 9), -1.0, np.float32))
    wins = np.array([[5000.0, 5000.0, 14000.0, 14000.0], [6000.0, 6000.0, 15000.0, 15000.0]])
    idx = np.array([[3, 3, 1, 1], [0, 0, 1, 1]], dtype=np.int64)
    ok = dict(dgrid=dgrid, H=H, W=W, geom=geom, windows=wins, n=2, mode=1, res=1000.0, out_h=9, out_w=9, out=out, stride=81)
    null_grid = dbm.DeviceArray((1,), dgrid.ctx, ptr=0, owner=dgrid)
    cases = [dict(out_h=0), dict(out_w=0), dict(out_h=-3), dict(H=1), dict(W=1), dict(geom=(500.0, 39500.0, 0.0, -1000.0)),
             dict(geom=(500.0, 39500.0, 1000.0, 0.0)), dict(geom=(500.0, 39500.0, float("nan"), -1000.0)),
             dict(geom=(500.0, 39500.0, 1000.0, float("inf"))), dict(mode=2), dict(mode=-1), dict(dgrid=null_grid), dict(out=None),
             dict(windows=None), dict(stride=80), dict(stride=0), dict(n=-1), dict(res=0.0), dict(res=float("nan")),
             dict(nodata=float("inf")),
             dict(mode=0, windows=np.array([[3, 3, 1, 1], [32, 0, 1, 1]], dtype=np.int64)),       # rows 32..40: one past the raster
             dict(mode=0, windows=np.array([[3, 3, 1, 1], [0, 42, 1, 1]], dtype=np.int64)),
             dict(mode=0, windows=np.array([[3, 3, 1, 1], [7, 0, -1, 1]], dtype=np.int64)),
             dict(mode=0, windows=np.array([[3, 3, 1, 1], [0, 0, 2, 1]], dtype=np.int64)),
             dict(mode=0, windows=np.array([[-1, 3, 1, 1], [0, 0, 1, 1]], dtype=np.int64))]
    for c in cases:
        rc = _tile_abi(dbm, **{**ok, **c})
        msg = _lib.lib().dbm_last_error(dgrid.ctx.handle)
        assert rc == 1 and msg and b"dbm_grid_tile" in msg, (c, rc, msg)
    dgrid.ctx.synchronize()
    assert (out.get() == -1.0).all()      # nothing was launched
    # H = 1 is fine for slicing; the accepted forms of both modes write what the restatement says
    assert _tile_abi(dbm, **{**ok, "mode": 0, "windows": idx}) == 0
    assert np.array_equal(out.get(), np.stack([g[3:12, 3:12], g[0:9, 0:9]]))
    assert _tile_abi(dbm, **ok) == 0
    _close(out.get()[:, None], tl.tile(g, (H, W), geom, wins)[0], _zmax(g))
    fl = dgrid.ctx.malloc(64)
    for c in (dict(size=35), dict(size=0), dict(size=8194), dict(step=0), dict(H=30), dict(W=35), dict(grid=None), dict(flags=None)):
        a = {**dict(grid=dgrid.ptr, H=H, W=W, size=36, step=3, flags=fl), **c}
        rc = _lib.lib().dbm_grid_filled_windows(dgrid.ctx.handle, C.c_void_p(a["grid"]) if a["grid"] else None, a["H"], a["W"], a["size"],
                                                a["step"], 0, 0, C.c_void_p(a["flags"]) if a["flags"] else None)
        assert rc == 1 and b"dbm_grid_filled_windows" in _lib.lib().dbm_last_error(dgrid.ctx.handle), c
    dgrid.ctx.free(fl)


def test_plane_past_2_to_the_31_elements(dbm):
    """46 400 x 46 400 float32 = 2.15 x 10^9 elements, 8.6 GB (W1 has 2.48 x 10^9): windows in the last rows and columns need 64-bit
    ELEMENT offsets.  The separable field a[r] + b[c] (float32 sums) lets the restatement evaluate only the nodes it needs; the plane
    is uploaded in row blocks so the host never holds more than one."""
    from deepbedmap_amd import _lib

    H = W = 46_400
    assert H * W > 2 ** 31
    r = np.random.default_rng(21)
    a = r.normal(0, 100, H).astype(np.float32)
    b = r.normal(0, 100, W).astype(np.float32)
    dgrid = dbm.DeviceArray((H, W))
    block = 800
    for r0 in range(0, H, block):
        host = np.add.outer(a[r0:r0 + block], b)
        assert host.dtype == np.float32 and host.flags.c_contiguous
        _lib.check(_lib.lib().dbm_memcpy_h2d(dgrid.ctx.handle, C.c_void_p(dgrid.ptr + 4 * r0 * W), host.ctypes.data_as(C.c_void_p), host.nbytes),
                   dgrid.ctx.handle)
    del host
    gc.collect()
    val = lambda rr, cc: a[rr] + b[cc]   # noqa: E731  (float32 + float32: the same bits as the plane's nodes)
    d = 100.0
    geom = (-2_320_000.0 + d / 2, 2_320_000.0 - d / 2, d, -d)      # north-up, edges at +-2 320 000
    raster = dbm.Raster(dgrid, dbm.GridGeometry(*geom))
    south, east = -2_320_000.0, 2_320_000.0
    wins = [(east - 9000.0 - 1000.0, south + 1000.0, east - 1000.0, south + 10000.0),          # samples ON the nodes, the last row and column included
            (east - 9000.0 - 1000.0 - 50.0, south + 1000.0 + 50.0, east - 1000.0 - 50.0, south + 10000.0 + 50.0),   # samples in mid-cell
            (east - 9000.0 - 3000.0, south + 20000.0, east - 3000.0, south + 29000.0),
            (east - 9000.0 + 2000.0, south - 2000.0, east + 2000.0, south + 7000.0),           # over the south-east corner
            (-2_320_000.0 + 1000.0, 2_320_000.0 - 10000.0, -2_320_000.0 + 10000.0, 2_320_000.0 - 1000.0)]   # the first rows and columns
    got = dbm.selective_tile(raster, wins, padding=1000).get()
    want, _ = tl.tile(val, (H, W), geom, wins, padding=1000)
    assert got.shape == (5, 1, 110, 110) and np.isnan(want[3]).any() and not np.isnan(want[[0, 1, 2, 4]]).any()
    _close(got, want, float(np.abs(a).max() + np.abs(b).max()))
    cut = [(east - 3600.0, south, east, south + 3600.0), (east - 3600.0 - 700.0, south + 500.0, east - 700.0, south + 4100.0)]
    got = dbm.selective_tile(raster, cut, interpolate=False).get()
    assert np.array_equal(got[0, 0], np.add.outer(a[H - 36:], b[W - 36:]))
    assert np.array_equal(got[1, 0], np.add.outer(a[H - 41:H - 5], b[W - 43:W - 7]))
    del raster, dgrid
    gc.collect()


def _random_generator(dbm, seed=1):
    from oracle import model as omodel

    og = omodel.GeneratorModel(num_residual_blocks=1, seed=seed)
    g = dbm.GeneratorModel(num_residual_blocks=1, initialize=False)
    for name, p in g._tensors.items():
        p.array = og.params[name]
    return g


def test_model_inputs_of_an_area_feed_the_test_area_score(dbm):
    data = _training_rasters(dbm, seed=3)
    bed, bedgeom = data["bedmap2"]
    bed = bed.copy()
    bed[36:39, 20:24] = -9999.0                 # a gap in BEDMAP2 inside the area: filled with -5000 (deepbedmap.py:168)
    acc, accgeom = data["accumulation"]
    acc = acc.copy()
    acc[40, 15] = -9999.0
    rasters = {k: dbm.Raster(g, geom) for k, (g, geom) in data.items()}
    rasters["bedmap2"] = dbm.Raster(bed, bedgeom, nodata=-9999.0)
    rasters["accumulation"] = dbm.Raster(acc, accgeom, nodata=-9999.0)
    bound = (-1_590_000.0, -290_000.0, -1_574_000.0, -278_000.0)      # 16 km x 12 km
    tiles = dbm.get_deepbedmap_model_inputs(bound, rasters["bedmap2"], rasters["rema"], rasters["velocity_x"], rasters["velocity_y"],
                                            rasters["accumulation"])
    X, W1, W2, W3 = tiles
    assert all(isinstance(t, dbm.DeviceArray) for t in tiles)
    assert (X.shape, W1.shape, W2.shape, W3.shape) == ((1, 1, 14, 18), (1, 1, 140, 180), (1, 2, 28, 36), (1, 1, 14, 18))

    def want(g, name, **kw):
        geom = data[name][1]
        return tl.tile(g, g.shape, tuple(geom.as_array()), [bound], padding=1000, **kw)[0]

    wX = want(bed, "bedmap2", nodata=-9999.0, gapfiller=-5000.0)
    assert (wX == -5000.0).any()
    _close(X.get(), wX, 9999.0)
    _close(W1.get(), want(data["rema"][0], "rema"), 1.0)
    _close(np.ascontiguousarray(W2.get()[:, :1]), want(data["velocity_x"][0], "velocity_x", resolution=500, gapfiller=0.0), 1.0)
    _close(np.ascontiguousarray(W2.get()[:, 1:]), want(data["velocity_y"][0], "velocity_y", resolution=500, gapfiller=0.0), 1.0)
    wW3 = want(acc, "accumulation", nodata=-9999.0, gapfiller=0.0)
    _close(W3.get(), wW3, 9999.0)
    # the score of the area: the forward runs on the GPU-cut tiles in both arms, the sampling is restated
    g = _random_generator(dbm)
    Hh, Ww = 4 * (14 - 2), 4 * (18 - 2)
    x = bound[0] + 125.0 + 250.0 * np.arange(Ww)
    y = bound[3] - 125.0 - 250.0 * np.arange(Hh)
    r = np.random.RandomState(31)
    pts = np.stack([r.uniform(x[0], x[-1], 4000), r.uniform(y[-1], y[0], 4000), r.normal(0.0, 1.0, 4000)], axis=1)
    rmse, grid = dbm.get_deepbedmap_test_result(g, X, W1, W2, W3, points=pts, x=x, y=y)
    with dbm.using_config("enable_backprop", False):
        Y = g.forward(X, W1, W2, W3).array
    Y = Y.get() if isinstance(Y, dbm.DeviceArray) else np.asarray(Y)
    assert grid.shape == (Hh, Ww) and np.array_equal(grid, np.flipud(Y[0, 0]))
    ref = tr.stats(tr.sample(np.flipud(Y[0, 0]), grid.shape, (x[0], y[0], 250.0, -250.0, 0), pts[:, 0], pts[:, 1], "bicubic"), pts[:, 2])
    assert ref["count"] == len(pts) and abs(rmse - ref["rmse"]) <= 1e-12 * ref["rmse"]
    score = dbm.make_test_area_score(X, W1, W2, W3, points=pts, x=x, y=y)
    assert abs(score(g) - rmse) <= 1e-6 * rmse
