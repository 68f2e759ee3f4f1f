"""-m gpu: dbm_grid_track (grid sampling along survey tracks + the along-track error statistics) against the float64 NumPy
restatement of its semantics (tests/track_restatement.py), and the scoring layer built on it (deepbedmap_amd/evaluation.py:
get_deepbedmap_test_result, make_test_area_score; reference srgan_train.py:1422-1466)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import track_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu
INTERPS = ("nearest", "bilinear", "bicubic")


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


def _same(got, want):
    """identical NaN masks, |got - want| <= 1e-9 (1 + |want|) elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (np.isnan(got).sum(), np.isnan(want).sum())
    m = ~np.isnan(want)
    assert np.all(np.abs(got[m] - want[m]) <= 1e-9 * (1.0 + np.abs(want[m]))), np.abs(got[m] - want[m]).max()


def _grid(H, W, seed, holes=True):
    r = np.random.default_rng(seed)
    g = (r.normal(0.0, 300.0, (H, W)) + 1000.0).astype(np.float32)   # bed elevations in metres
    if holes and H * W > 16:
        g[r.random((H, W)) < 0.03] = np.nan
        g[H // 2, : W // 3] = np.nan      # a stretch of holes
    return g


def _points(H, W, reg, geom, n, seed):
    """~n points: uniform over the domain, exact nodes, domain edges, half-pixel bands, just outside, NaN coordinates."""
    r = np.random.default_rng(seed)
    half = 0.5 if reg == 1 else 0.0
    k = n // 8
    t = [r.uniform(-half, W - 1 + half, 4 * k)]
    s = [r.uniform(-half, H - 1 + half, 4 * k)]
    t.append(r.integers(0, W, k).astype(np.float64)); s.append(r.integers(0, H, k).astype(np.float64))     # nodes
    e = r.integers(0, 4, k)
    te = np.where(e == 0, -half, np.where(e == 1, W - 1 + half, r.uniform(-half, W - 1 + half, k)))
    se = np.where(e == 2, -half, np.where(e == 3, H - 1 + half, r.uniform(-half, H - 1 + half, k)))
    t.append(te); s.append(se)                                                                             # edges
    tb = np.where(r.random(k) < 0.5, r.uniform(-half, 0.5, k), r.uniform(W - 1.5, W - 1 + half, k))
    sb = np.where(r.random(k) < 0.5, r.uniform(-half, 0.5, k), r.uniform(H - 1.5, H - 1 + half, k))
    t.append(tb); s.append(sb)                                                                             # bands
    out = r.uniform(1e-9, 0.3, k)
    t.append(np.where(r.random(k) < 0.5, -half - out, W - 1 + half + out)); s.append(r.uniform(-half, H - 1 + half, k))  # outside
    t, s = np.concatenate(t), np.concatenate(s)
    nanpick = r.random(t.size) < 0.01
    t[nanpick & (r.random(t.size) < 0.5)] = np.nan
    s[nanpick & (r.random(t.size) < 0.5)] = np.nan
    x0, y0, dx, dy, _ = geom
    z = r.normal(900.0, 300.0, t.size)   # (errors of about +100 m: the mean is far from zero)
    z[r.random(t.size) < 0.01] = np.nan
    return np.ascontiguousarray(np.stack([x0 + t * dx, y0 + s * dy, z], axis=1))


def _geom(dbm, reg):
    return dbm.GridGeometry(-1000.0, 5000.0, 250.0, -125.0, "pixel" if reg else "gridline")


@pytest.mark.parametrize("shape", [(2, 2), (2, 3), (5, 2), (37, 211), (300, 170)])
@pytest.mark.parametrize("interp", INTERPS)
def test_parity_with_the_restatement(dbm, shape, interp):
    H, W = shape
    grid = _grid(H, W, seed=H * 1000 + W)
    for reg in (0, 1):
        geom = _geom(dbm, reg)
        pts = _points(H, W, reg, tuple(geom.as_array()), 100_000, seed=reg + H + W)
        for thr in (0.1, 0.5, 1.0):
            z, st = dbm.grdtrack(pts, grid, geom, interpolation=interp, threshold=thr)
            want = tr.sample(grid, (H, W), tuple(geom.as_array()), pts[:, 0], pts[:, 1], interp, thr)
            _same(z, want)
            ref = tr.stats(z, pts[:, 2])
            assert st.count == ref["count"] > 0
            for k in ("mean", "std", "min", "max", "rmse"):
                assert abs(getattr(st, k) - ref[k]) <= 1e-10 * abs(ref[k]), (k, getattr(st, k), ref[k])


def test_statistics_of_errors_in_metres(dbm):
    """Chan's pairwise merges keep std accurate for errors of metres around a large common offset."""
    H, W = 64, 96
    grid = _grid(H, W, 7, holes=False)
    geom = _geom(dbm, 1)
    pts = _points(H, W, 1, tuple(geom.as_array()), 400_000, 8)
    zi = tr.sample(grid, (H, W), tuple(geom.as_array()), pts[:, 0], pts[:, 1], "bicubic")
    r = np.random.default_rng(9)
    pts[:, 2] = zi - (5000.0 + r.normal(0.0, 2.0, len(zi)))   # e = 5000 m offset + N(0, 2 m)
    z, st = dbm.grdtrack(pts, grid, geom)
    ref = tr.stats(z, pts[:, 2])
    assert st.count == ref["count"] and st.count > 300_000
    for k in ("mean", "std", "min", "max", "rmse"):
        assert abs(getattr(st, k) - ref[k]) <= 1e-10 * abs(ref[k]), (k, getattr(st, k), ref[k])
    assert 1.9 < st.std < 2.1


def _track_dev(dbm, dgrid, H, W, geom, dpts, n, ncol, interp, zdev, sdev, thr=0.5):
    from deepbedmap_amd import _lib

    g = geom.as_array()
    _lib.check(_lib.lib().dbm_grid_track(dgrid.ctx.handle, C.c_void_p(dgrid.ptr), H, W, g.ctypes.data_as(C.POINTER(C.c_double)),
                                         C.c_void_p(dpts), n, ncol, dbm.evaluation.INTERPOLATIONS[interp], thr, C.c_void_p(zdev),
                                         C.c_void_p(sdev), _lib.DEVICE_PTRS), dgrid.ctx.handle)


def test_determinism_and_host_device_forms_agree_bitwise(dbm):
    H, W = 211, 157
    grid = _grid(H, W, 3)
    geom = _geom(dbm, 0)
    pts = _points(H, W, 0, tuple(geom.as_array()), 300_000, 4)
    dgrid = dbm.to_device(grid)
    for interp in INTERPS:
        runs = [dbm.grdtrack(pts, dgrid, geom, interpolation=interp) for _ in range(3)]
        for z, st in runs[1:]:
            assert np.array_equal(z.view(np.uint64), runs[0][0].view(np.uint64))
            assert np.array_equal(np.array(dataclass_values(st)).view(np.uint64), np.array(dataclass_values(runs[0][1])).view(np.uint64))
        dp = dbm.DevicePoints(pts)
        for _ in range(2):
            z, st = dbm.grdtrack(dp, dgrid, geom, interpolation=interp)
            assert np.array_equal(z.view(np.uint64), runs[0][0].view(np.uint64))
            assert np.array_equal(np.array(dataclass_values(st)).view(np.uint64), np.array(dataclass_values(runs[0][1])).view(np.uint64))
        # the C entry point itself with device pointers into the same buffers
        zdev, sdev = dp.outputs()
        _track_dev(dbm, dgrid, H, W, geom, dp.ptr, dp.n, 3, interp, zdev, sdev)
        s = np.empty(6)
        dbm._lib.check(dbm._lib.lib().dbm_memcpy_d2h(dgrid.ctx.handle, s.ctypes.data_as(C.c_void_p), C.c_void_p(sdev), 48),
                       dgrid.ctx.handle)
        assert np.array_equal(s.view(np.uint64), np.array(dataclass_values(runs[0][1])).view(np.uint64))
        # without values, without a z column
        z2, st2 = dbm.grdtrack(pts, dgrid, geom, interpolation=interp, return_values=False)
        assert z2 is None and dataclass_values(st2) == dataclass_values(runs[0][1])
        z3, st3 = dbm.grdtrack(pts[:, :2], dgrid, geom, interpolation=interp)
        assert np.array_equal(z3.view(np.uint64), runs[0][0].view(np.uint64)) and st3.count == 0 and np.isnan(st3.rmse)


def dataclass_values(st):
    return [float(st.count), st.mean, st.std, st.min, st.max, st.rmse]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, (1 << 20) + 7])
def test_edge_values_of_n(dbm, n):
    H, W = 50, 70
    grid = _grid(H, W, 11)
    geom = _geom(dbm, 1)
    pts = _points(H, W, 1, tuple(geom.as_array()), n + 8, 12)[:n]   # (_points makes a multiple of 8)
    z, st = dbm.grdtrack(pts, grid, geom, interpolation="bicubic")
    assert z.shape == (n,)
    _same(z, tr.sample(grid, (H, W), tuple(geom.as_array()), pts[:, 0], pts[:, 1], "bicubic"))
    ref = tr.stats(z, pts[:, 2])
    assert st.count == ref["count"]
    for k in ("mean", "std", "min", "max", "rmse"):
        a, b = getattr(st, k), ref[k]
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-10 * abs(b), (k, a, b)
    if n == 0:
        assert st.count == 0 and all(np.isnan(v) for v in dataclass_values(st)[1:])


def test_plane_past_2_to_the_31_bytes(dbm):
    """24 000 x 24 000 float32 = 2.3 GB: points in the last rows and columns (64-bit offsets); the separable field
    a[r] + b[c] (float32 sums) lets the restatement evaluate only the stencil nodes."""
    from deepbedmap_amd import _lib

    H = W = 24_000
    assert 4 * H * W > 2 ** 31
    r = np.random.default_rng(21)
    a = r.normal(0, 100, H).astype(np.float32)
    b = r.normal(0, 100, W).astype(np.float32)
    host = np.add.outer(a, b)
    assert host.dtype == np.float32
    dgrid = dbm.to_device(host)
    del host
    gc.collect()
    val = lambda rr, cc: a[rr] + b[cc]   # noqa: E731  (float32 + float32: the same bits as the plane's nodes)
    n = 200_000
    t = np.concatenate([r.uniform(W - 40, W - 1, n // 2), r.uniform(0, W - 1, n // 2)])
    s = np.concatenate([r.uniform(H - 40, H - 1, n // 4), r.uniform(0, H - 1, n // 4), r.uniform(H - 3, H - 1, n // 2)])
    t[:8] = W - 1
    s[:8] = H - 1
    geom = dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    pts = np.ascontiguousarray(np.stack([t, s, r.normal(0, 100, n)], axis=1))
    for interp in INTERPS:
        z, st = dbm.grdtrack(pts, dgrid, geom, interpolation=interp)
        _same(z, tr.sample(val, (H, W), (0.0, 0.0, 1.0, 1.0, 0), t, s, interp))
        assert st.count == n
    # refusals (nothing launched): H = 1 for bilinear / bicubic, in Python and in the C entry point
    one = dbm.DeviceArray((1, W), dgrid.ctx, ptr=dgrid.ptr, owner=dgrid)
    with pytest.raises(ValueError, match="2 x 2"):
        dbm.grdtrack(pts, one, geom, interpolation="bilinear")
    g = geom.as_array()
    for interp in (1, 2):
        rc = _lib.lib().dbm_grid_track(dgrid.ctx.handle, C.c_void_p(dgrid.ptr), 1, W, g.ctypes.data_as(C.POINTER(C.c_double)),
                                       pts.ctypes.data_as(C.c_void_p), n, 3, interp, 0.5, None, None, 0)
        assert rc == 1 and b"2 x 2" in _lib.lib().dbm_last_error(dgrid.ctx.handle)
    assert _lib.lib().dbm_grid_track(dgrid.ctx.handle, C.c_void_p(dgrid.ptr), H, W, g.ctypes.data_as(C.POINTER(C.c_double)),
                                     pts.ctypes.data_as(C.c_void_p), n, 3, 3, 0.5, None, None, 0) == 1
    assert _lib.lib().dbm_grid_track(dgrid.ctx.handle, C.c_void_p(dgrid.ptr), H, W, g.ctypes.data_as(C.POINTER(C.c_double)),
                                     pts.ctypes.data_as(C.c_void_p), n, 3, 2, 0.0, None, None, 0) == 1
    z, _ = dbm.grdtrack(pts[:100], one, geom, interpolation="nearest")   # nearest takes a single row
    _same(z, tr.sample(val, (1, W), (0.0, 0.0, 1.0, 1.0, 0), t[:100], s[:100], "nearest"))
    del one, dgrid
    gc.collect()


def test_reduced_continent_canvas_in_place(dbm):
    """The 3 x 3-tile area of test_gpu_fullsize.py (3000 x 3000 output pixels, NaN frame of 76 pixels) from
    predict_tiled_resident(download=False): sampling the DeviceArray equals sampling its download bit for bit; points in and near
    the NaN frame follow the threshold rule."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dem_model import dem_generator

    g = dem_generator(dbm, seed=909, num_residual_blocks=1)
    H = W = 750
    r = np.random.RandomState(11)
    X = r.uniform(-2000, 2000, (1, 1, H, W)).astype(np.float32)
    W1 = r.uniform(-100, 4000, (1, 1, 10 * H, 10 * W)).astype(np.float32)
    W2 = r.uniform(-10, 1000, (1, 2, 2 * H, 2 * W)).astype(np.float32)
    W3 = r.uniform(0, 500, (1, 1, H, W)).astype(np.float32)
    S = dbm.Shape
    final = S(y=4 * H, x=4 * W)
    canvas = dbm.predict_tiled_resident(g, X, W1, W2, W3, final_shape=final, ary_shape=S(y=1000, x=1000), stride=S(y=1000, x=1000),
                                        xtrapad=S(y=18, x=18), download=False, dtype="bfloat16", clip=True)
    assert isinstance(canvas, dbm.DeviceArray)
    host = canvas.get()
    frame = (18 + 1) * 4
    assert np.isnan(host[0, :frame]).all() and not np.isnan(host[0, frame:-frame, frame:-frame]).any()
    bound = (-1_000_000.0, -500_000.0, -1_000_000.0 + 250.0 * final.x, -500_000.0 + 250.0 * final.y)
    geom = dbm.GridGeometry.from_bounds(bound, final.y, final.x)
    rng = np.random.default_rng(13)
    n = 200_000
    t = np.concatenate([rng.uniform(-0.5, final.x - 0.5, n // 2), rng.uniform(frame - 3, frame + 3, n // 2)])
    s = np.concatenate([rng.uniform(-0.5, final.y - 0.5, n // 2), rng.uniform(frame, final.y - frame, n // 2)])
    pts = np.ascontiguousarray(np.stack([geom.x0 + t * geom.dx, geom.y0 + s * geom.dy, rng.normal(1000, 500, n)], axis=1))
    for interp in INTERPS:
        for thr in (0.1, 0.5, 1.0):
            z_dev, st_dev = dbm.grdtrack(pts, canvas, geom, interpolation=interp, threshold=thr)
            z_host, st_host = dbm.grdtrack(pts, host, geom, interpolation=interp, threshold=thr)
            assert np.array_equal(z_dev.view(np.uint64), z_host.view(np.uint64)) and st_dev == st_host
            _same(z_dev, tr.sample(host[0], (final.y, final.x), tuple(geom.as_array()), pts[:, 0], pts[:, 1], interp, thr))
        # the frame's edge: a band of points half in the frame is kept at a low threshold, lost at threshold 1
        band = (t > frame - 1) & (t < frame) & (s > frame + 2) & (s < final.y - frame - 3)
        if interp != "nearest":
            lo = dbm.grdtrack(pts[band], canvas, geom, interpolation=interp, threshold=0.1)[0]
            hi = dbm.grdtrack(pts[band], canvas, geom, interpolation=interp, threshold=1.0)[0]
            assert np.isnan(hi).all() and (~np.isnan(lo)).sum() > 0


def _small_area(seed=31):
    r = np.random.RandomState(seed)
    h, w = 14, 18
    X = r.uniform(-1, 1, (1, 1, h, w)).astype(np.float32)
    W1 = r.uniform(0, 1, (1, 1, 10 * h, 10 * w)).astype(np.float32)
    W2 = r.uniform(0, 1, (1, 2, 2 * h, 2 * w)).astype(np.float32)
    W3 = r.uniform(0, 1, (1, 1, h, w)).astype(np.float32)
    H, W = 4 * (h - 2), 4 * (w - 2)
    x = -1_500_000.0 + 250.0 * np.arange(W)          # ground truth coordinates: x ascending, y descending (north-up raster)
    y = -300_000.0 - 250.0 * np.arange(H)
    n = 5000
    pts = np.stack([r.uniform(x[0], x[-1], n), r.uniform(y[-1], y[0], n), r.normal(0.0, 1.0, n)], axis=1)
    return (X, W1, W2, W3), pts, x, y


def _random_generator(dbm, seed=1):
    from oracle import model as omodel

    og = omodel.GeneratorModel(num_residual_blocks=1, seed=seed)
    g = dbm.GeneratorModel(num_residual_blocks=1, initialize=False)
    for name, p in g._tensors.items():
        p.array = og.params[name]
    return g, og


def test_get_deepbedmap_test_result(dbm):
    ins, pts, x, y = _small_area()
    g, og = _random_generator(dbm)
    rmse, grid = dbm.get_deepbedmap_test_result(g, *ins, points=pts, x=x, y=y)
    with dbm.using_config("enable_backprop", False):
        Y = g.forward(*ins).array
    assert grid.shape == Y.shape[2:] and np.array_equal(grid, np.flipud(Y[0, 0]))
    # the reference's grid: np.flipud(Y_hat[0, 0]) on coords (y, x), sampled by grdtrack (-nc), RMSE of the finite errors
    geom = (x[0], y[0], x[1] - x[0], y[1] - y[0], 0)
    want = tr.stats(tr.sample(np.flipud(Y[0, 0]), grid.shape, geom, pts[:, 0], pts[:, 1], "bicubic"), pts[:, 2])
    assert want["count"] == len(pts)
    assert abs(rmse - want["rmse"]) <= 1e-12 * want["rmse"]
    # ... and the oracle's forward (float32 NumPy) through the same restatement: within the forward's own tolerance
    ref = og.forward(*ins)
    err = float(np.abs(Y - ref).max() / np.abs(ref).max())
    assert err < 1e-4
    want_o = tr.stats(tr.sample(np.flipud(ref[0, 0]), grid.shape, geom, pts[:, 0], pts[:, 1], "bicubic"), pts[:, 2])
    assert abs(rmse - want_o["rmse"]) <= 2e-4 * float(np.abs(ref).max())
    # the other interpolants and bf16 inference pass through
    for interp in ("nearest", "bilinear"):
        r2, _ = dbm.get_deepbedmap_test_result(g, *ins, points=pts, x=x, y=y, interpolation=interp)
        w2 = tr.stats(tr.sample(np.flipud(Y[0, 0]), grid.shape, geom, pts[:, 0], pts[:, 1], interp), pts[:, 2])
        assert abs(r2 - w2["rmse"]) <= 1e-12 * w2["rmse"]
    r3, _ = dbm.get_deepbedmap_test_result(g, *ins, points=pts, x=x, y=y, dtype="bfloat16")
    assert np.isfinite(r3) and abs(r3 - rmse) <= 0.05 * float(np.abs(ref).max())   # bf16 bound 3e-2 x sum |w|
    with pytest.raises(ValueError, match="z column"):
        dbm.get_deepbedmap_test_result(g, *ins, points=pts[:, :2], x=x, y=y)
    with pytest.raises(ValueError, match="do not match"):
        dbm.get_deepbedmap_test_result(g, *ins, points=pts, x=x[:-1], y=y)


def test_train_epochs_keeps_the_best_test_area_score(dbm, tmp_path):
    np.random.seed(5)
    r = np.random.RandomState(1)
    n = 12
    ds = {"X": r.rand(n, 1, 11, 11), "W1": r.rand(n, 1, 110, 110), "W2": r.rand(n, 2, 22, 22), "W3": r.rand(n, 1, 11, 11),
          "Y": r.rand(n, 1, 36, 36)}
    ds = dbm.dataset_to_device({k: v.astype(np.float32) for k, v in ds.items()})
    train_iter, _, dev_iter, _ = dbm.get_train_dev_iterators(ds, first_size=8, batch_size=4, seed=42)
    g, g_opt, d, d_opt = dbm.compile_srgan_model(num_residual_blocks=1, residual_scaling=0.3, learning_rate=5e-4)
    ins, pts, x, y = _small_area()
    score = dbm.make_test_area_score(*ins, points=pts, x=x, y=y)
    before = score(g)
    assert abs(before - dbm.get_deepbedmap_test_result(g, *ins, points=pts, x=x, y=y)[0]) <= 1e-6 * before   # resident inputs
    seen = []

    def recording(model):
        v = score(model)
        seen.append(v)
        return v

    table, best, saved = dbm.train_epochs(2, train_iter, dev_iter, g, g_opt, d, d_opt, score_fn=recording,
                                          save_path=str(tmp_path / "w"), best_score=1e30)
    assert len(seen) == 2 and all(np.isfinite(seen)) and best == min(seen)
    assert saved is not None and all(os.path.exists(p) for p in saved)
    assert abs(seen[1] - dbm.get_deepbedmap_test_result(g, *ins, points=pts, x=x, y=y)[0]) <= 1e-6 * seen[1]   # final weights
