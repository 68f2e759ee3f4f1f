"""CPU checks of the track sampling semantics (tests/track_restatement.py: what dbm_grid_track computes) against known answers,
of the geometry the GeoTIFF writer records, of the argument refusals, and of the loud failure without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_restatement as tr  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402


def _domain_points(H, W, reg, n, seed):
    """Points spread over the whole domain in node units, the half-pixel bands and the exact edges included."""
    r = np.random.default_rng(seed)
    half = 0.5 if reg == 1 else 0.0
    t = r.uniform(-half, W - 1 + half, n)
    s = r.uniform(-half, H - 1 + half, n)
    edges_t = np.array([-half, W - 1 + half, -half, W - 1 + half, 0.0, W - 1, 0.5 * (W - 1)])
    edges_s = np.array([-half, -half, H - 1 + half, H - 1 + half, H - 1, 0.0, 0.5 * (H - 1)])
    return np.concatenate([t, edges_t]), np.concatenate([s, edges_s])


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("reg", [0, 1])
def test_a_plane_is_reproduced_over_the_whole_domain(interp, reg):
    H, W = 7, 9
    geom = (1000.0, 5000.0, 250.0, -250.0, reg)   # north-up
    rr, cc = np.mgrid[0:H, 0:W]
    X, Y = geom[0] + cc * geom[2], geom[1] + rr * geom[3]
    a, b, c = 12.0, 0.25, -0.5
    grid = (a + b * X + c * Y).astype(np.float32)
    assert np.array_equal(grid.astype(np.float64), a + b * X + c * Y)   # the nodes are exact in float32
    t, s = _domain_points(H, W, reg, 4000, 1)
    xs, ys = geom[0] + t * geom[2], geom[1] + s * geom[3]
    got = tr.sample(grid, (H, W), geom, xs, ys, interp)
    want = a + b * xs + c * ys
    assert not np.isnan(got).any()
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_bicubic_reproduces_a_quadratic_away_from_the_ghost_nodes():
    H, W = 8, 11
    geom = (0.0, 0.0, 1.0, 1.0, 0)
    rr, cc = np.mgrid[0:H, 0:W]
    f = lambda x, y: 3.0 + 0.5 * x - 0.25 * y + 0.125 * x * x - 0.0625 * x * y + 0.25 * y * y   # noqa: E731
    grid = f(cc, rr).astype(np.float32)
    assert np.array_equal(grid.astype(np.float64), f(cc, rr))
    r = np.random.default_rng(2)
    xs, ys = r.uniform(1, W - 2, 3000), r.uniform(1, H - 2, 3000)   # stencil c-1 .. c+2 inside the grid
    got = tr.sample(grid, (H, W), geom, xs, ys, "bicubic")
    assert np.abs(got - f(xs, ys)).max() <= 1e-10 * np.abs(f(xs, ys)).max()
    # ... and not with a ghost node in the stencil (linear extrapolation is not quadratic)
    edge = tr.sample(grid, (H, W), geom, np.array([0.5]), np.array([0.5]), "bicubic")
    assert abs(edge[0] - f(0.5, 0.5)) > 1e-3


def test_bilinear_agrees_with_scipy():
    scipy_interp = pytest.importorskip("scipy.interpolate")
    H, W = 13, 17
    r = np.random.default_rng(3)
    grid = r.uniform(-500, 2000, (H, W)).astype(np.float32)
    geom = (-2.0, 40.0, 0.5, -2.0, 0)
    xs_nodes, ys_nodes = geom[0] + np.arange(W) * geom[2], geom[1] + np.arange(H) * geom[3]
    f = scipy_interp.RegularGridInterpolator((ys_nodes[::-1], xs_nodes), grid[::-1].astype(np.float64), method="linear")
    t, s = _domain_points(H, W, 0, 5000, 4)
    xs, ys = geom[0] + t * geom[2], geom[1] + s * geom[3]
    ys = np.clip(ys, ys_nodes.min(), ys_nodes.max())   # (scipy refuses points a rounding outside its domain)
    xs = np.clip(xs, xs_nodes.min(), xs_nodes.max())
    got = tr.sample(grid, (H, W), geom, xs, ys, "bilinear")
    want = f(np.stack([ys, xs], axis=1))
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_nan_threshold_hand_computed():
    # 4 x 4 gridline grid, node (1, 1) is NaN; a bilinear point at t = 1.25, s = 1.5 (cell (1..2, 1..2))
    grid = np.arange(16, dtype=np.float32).reshape(4, 4)
    grid[1, 1] = np.nan
    geom = (0.0, 0.0, 1.0, 1.0, 0)
    x, y = np.array([1.25]), np.array([1.5])
    # weights: (1,1) .75*.5 = .375 (NaN), (1,2) .25*.5 = .125, (2,1) .75*.5 = .375, (2,2) .25*.5 = .125; wsum valid = .625
    valid = 0.125 * 6.0 + 0.375 * 9.0 + 0.125 * 10.0
    for thr, want in ((0.1, valid / 0.625), (0.5, valid / 0.625), (1.0, np.nan)):
        got = tr.sample(grid, (4, 4), geom, x, y, "bilinear", thr)[0]
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) < 1e-12, (thr, got, want)
    # the cell's centre with its left column NaN: valid weight 0.25 + 0.25 = 0.5 -- accepted at 0.5 and 0.1, refused at 1.0
    grid2 = np.arange(16, dtype=np.float32).reshape(4, 4)
    grid2[1, 1] = grid2[2, 1] = np.nan      # the left column of the cell
    got = tr.sample(grid2, (4, 4), geom, np.array([1.5]), np.array([1.5]), "bilinear", 0.5)[0]
    assert got == 0.5 * (6.0 + 10.0)
    assert np.isnan(tr.sample(grid2, (4, 4), geom, np.array([1.5]), np.array([1.5]), "bilinear", 1.0)[0])
    assert not np.isnan(tr.sample(grid2, (4, 4), geom, np.array([1.5]), np.array([1.5]), "bilinear", 0.1)[0])
    # every node valid: the weighted sum (no division)
    assert tr.sample(grid2, (4, 4), geom, np.array([2.0]), np.array([0.0]), "bilinear", 1.0)[0] == 2.0
    # a NaN node of weight 0 (the exact node (0, 1) of cell (0..1, 1..2)): the valid weight is 1, kept even at threshold 1
    assert tr.sample(grid2, (4, 4), geom, np.array([1.0]), np.array([0.0]), "bilinear", 1.0)[0] == 1.0
    # nearest: the node itself, NaN stays NaN
    assert np.isnan(tr.sample(grid2, (4, 4), geom, np.array([1.2]), np.array([0.9]), "nearest")[0])


def test_outside_and_nan_coordinates_are_nan_and_ghosts_extrapolate():
    grid = np.array([[0, 1, 3], [10, 11, 13]], dtype=np.float32)
    gl, px = (0.0, 0.0, 1.0, 1.0, 0), (0.0, 0.0, 1.0, 1.0, 1)
    xs = np.array([-0.01, 2.01, np.nan, 1.0, -0.5, 2.5])
    ys = np.array([0.5, 0.5, 0.5, np.nan, 0.0, 1.0])
    got = tr.sample(grid, (2, 3), gl, xs, ys, "bilinear")
    assert np.isnan(got).all()
    got = tr.sample(grid, (2, 3), px, xs, ys, "bilinear")
    assert np.isnan(got[2:4]).all()
    assert got[4] == 0 + 0.5 * (0 - 1)           # ghost column -1 of row 0: z0 + (z0 - z1), half of it
    assert got[5] == 13 + 0.5 * (13 - 11)        # ghost column 3 of row 1
    assert abs(got[0] - 4.99) < 1e-12             # t = -0.01: rows 0 and 1 with their ghost column -1 (-1, 9)
    # a corner ghost: rows of ghosts (tensor product): (-1, -1) = g(0,-1) + (g(0,-1) - g(1,-1)) = -1 + (-1 - 9) = -11
    v = tr.node(lambda r, c: grid[r, c], 2, 3, np.array([-1]), np.array([-1]))
    assert v[0] == -11.0


def test_stats_of_the_restatement():
    zi = np.array([1.0, 2.0, np.nan, 4.0, np.inf])
    z = np.array([0.5, 2.5, 1.0, 1.0, 0.0])
    s = tr.stats(zi, z)
    e = np.array([0.5, -0.5, 3.0])
    assert s["count"] == 3 and s["mean"] == e.mean() and s["std"] == e.std(ddof=1)
    assert s["min"] == -0.5 and s["max"] == 3.0 and s["rmse"] == np.sqrt((e * e).mean())
    s1 = tr.stats(zi[:1], z[:1])
    assert s1["count"] == 1 and np.isnan(s1["std"]) and s1["rmse"] == 0.5
    s0 = tr.stats(zi[2:3], z[2:3])
    assert s0["count"] == 0 and all(np.isnan(s0[k]) for k in ("mean", "std", "min", "max", "rmse"))


def test_geometry_from_bounds_matches_the_geotiff_writer(tmp_path):
    H, W = 6, 10
    bound = (-1593250.0, -1090250.0, -1593250.0 + W * 250.0, -1090250.0 + H * 250.0)
    arr = np.arange(H * W, dtype=np.float32).reshape(1, H, W)
    path = dbm.save_array_to_grid(str(tmp_path / "g"), window_bound=bound, array=arr)
    _, info = dbm.read_geotiff(path)
    g = dbm.GridGeometry.from_bounds(bound, H, W)
    px, py, _ = info["pixel_scale"]
    tie = info["tiepoint"]
    assert g.registration == "pixel" and g.dx == px and g.dy == -py
    assert g.x0 - g.dx / 2 == tie[3] and g.y0 - g.dy / 2 == tie[4]   # pixel (0, 0)'s outer corner: (minx, maxy)
    # the canvas of the continent: 18000 x 22000 at 250 m
    big = dbm.GridGeometry.from_bounds((-2700000.0, -2200000.0, 2800000.0, 2300000.0), 18000, 22000)
    assert big.dx == 250.0 and big.dy == -250.0


def test_geometry_from_coords_and_flipped_rows():
    x = 100.0 + 250.0 * np.arange(5)
    y = 900.0 - 250.0 * np.arange(4)
    g = dbm.GridGeometry.from_coords(x, y)
    assert (g.x0, g.y0, g.dx, g.dy, g.registration) == (100.0, 900.0, 250.0, -250.0, "gridline")
    f = g.flipped_rows(4)
    assert f.y0 == y[-1] and f.dy == 250.0
    # sampling flipud(grid) on (x, y) is sampling grid through the flipped geometry
    r = np.random.default_rng(5)
    grid = r.normal(size=(4, 5)).astype(np.float32)
    xs, ys = r.uniform(x[0], x[-1], 500), r.uniform(y[-1], y[0], 500)
    a = tr.sample(np.flipud(grid), (4, 5), tuple(g.as_array()), xs, ys, "bicubic")
    b = tr.sample(grid, (4, 5), tuple(f.as_array()), xs, ys, "bicubic")
    assert np.abs(a - b).max() < 1e-12
    with pytest.raises(ValueError, match="evenly spaced"):
        dbm.GridGeometry.from_coords(np.array([0.0, 1.0, 3.0]), y)
    with pytest.raises(ValueError, match="at least two"):
        dbm.GridGeometry.from_coords(np.array([0.0]), y)


def test_argument_refusals_come_before_any_launch():
    pts = np.zeros((4, 3))
    g = dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="interpolation"):
        dbm.grdtrack(pts, np.zeros((4, 4), np.float32), g, interpolation="spline")
    for thr in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            dbm.grdtrack(pts, np.zeros((4, 4), np.float32), g, threshold=thr)
    for shape in ((1, 5), (5, 1), (1, 1, 1, 7)):
        for interp in ("bilinear", "bicubic"):
            with pytest.raises(ValueError, match="2 x 2"):
                dbm.grdtrack(pts, np.zeros(shape, np.float32), g, interpolation=interp)
    with pytest.raises(ValueError, match="empty"):
        dbm.grdtrack(pts, np.zeros((0, 4), np.float32), g, interpolation="nearest")
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        dbm.grdtrack(pts, np.zeros((2, 4, 4), np.float32), g)
    with pytest.raises(ValueError, match="points"):
        dbm.grdtrack(np.zeros((4, 4)), np.zeros((4, 4), np.float32), g)
    with pytest.raises(ValueError, match="non-zero"):
        dbm.GridGeometry(0.0, 0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="registration"):
        dbm.GridGeometry(0.0, 0.0, 1.0, 1.0, "cell")
    with pytest.raises(TypeError):
        dbm.grdtrack(pts, np.zeros((4, 4), np.float32), (0.0, 0.0, 1.0, 1.0, 0))


def test_product_functions_are_not_collected_as_tests():
    import deepbedmap_amd.evaluation as ev

    assert not [n for n in dir(ev) if n.startswith("test")]


def test_no_gpu_means_loud_failure():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from deepbedmap_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    pts = np.zeros((4, 3))
    g = dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    with pytest.raises(dbm.DbmError):
        dbm.grdtrack(pts, np.zeros((4, 4), np.float32), g)
    with pytest.raises(dbm.DbmError):
        dbm.DevicePoints(pts)
    x, y = np.arange(4.0), np.arange(4.0)
    with pytest.raises(dbm.DbmError):
        dbm.make_test_area_score(np.zeros((1, 1, 3, 3), np.float32), None, None, None, pts, x, y)
