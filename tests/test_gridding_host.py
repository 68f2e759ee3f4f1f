"""CPU checks of the gridding semantics (tests/gridding_restatement.py: what dbm_points_polar_stereographic, dbm_points_region and
dbm_points_blockmedian compute) against answers that do not come from it -- the worked example of EPSG Guidance Note 7-2, closed
forms, the reference's own doctest clouds grouped by hand, pandas -- and of the host-side refusals of deepbedmap_amd/gridding.py,
which need no GPU."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gridding_restatement as gr  # noqa: E402

# EPSG Guidance Note 7-2, Polar Stereographic (variant B) example: WGS 84, phi_F = 71 S, lambda_0 = 70 E, FE = FN = 6 000 000
GN72 = (6378137.0, 298.257223563, -71.0, 70.0, 6000000.0, 6000000.0)


def test_projection_worked_example_of_guidance_note_7_2():
    out, k = gr.polar_stereographic([[120.0, -75.0]], GN72, intermediates=True)
    # published: E = 7 255 380.79, N = 7 053 389.56 (two decimals: 0.005 m)
    assert abs(out[0, 0] - 7255380.79) <= 0.005, out
    assert abs(out[0, 1] - 7053389.56) <= 0.005, out
    # intermediates to half a unit of their last printed digit
    assert abs(k["t_F"] - 0.168407325) <= 0.5e-9
    assert abs(k["m_F"] - 0.326546781) <= 0.5e-9
    assert abs(k["k0"] - 0.97276901) <= 0.5e-8
    assert abs(k["t"][0] - 0.132508348) <= 0.5e-9
    assert abs(k["rho"][0] - 1638783.238) <= 0.5e-3


def test_projection_epsg3031_pole_parallel_symmetry_quadrant():
    pole = gr.polar_stereographic([[0.0, -90.0], [33.0, -90.0], [-179.0, -90.0]])
    assert np.array_equal(pole, np.zeros((3, 2)))   # exactly (0, 0)
    a, f = 6378137.0, 1.0 / 298.257223563
    e2 = 2 * f - f * f
    s71 = np.sin(np.deg2rad(71.0))
    closed = a * np.cos(np.deg2rad(71.0)) / np.sqrt(1.0 - e2 * s71 * s71)   # scale 1 on the standard parallel: rho = a m_F
    assert abs(closed - 2082760.1085) < 1e-3
    par = gr.polar_stereographic([[0.0, -71.0]])
    assert par[0, 0] == 0.0 and abs(par[0, 1] - closed) <= 1e-8   # metres: a few ulp of 2e6 m are 1e-9 m
    lons = np.array([-180.0, -135.0, -90.0, -45.0, 0.0, 45.0, 90.0, 135.0])
    ring = gr.polar_stereographic(np.stack([lons, np.full(8, -77.25)], axis=1))
    rho = np.hypot(ring[:, 0], ring[:, 1])
    assert np.all(np.abs(rho - rho[0]) <= 1e-8)   # metres
    sw = gr.polar_stereographic([[-110.25, -75.5]])
    assert sw[0, 0] < 0 and sw[0, 1] < 0
    # non-finite in, NaN out; further columns untouched
    bad = gr.polar_stereographic([[np.nan, -80.0, 7.0], [10.0, np.inf, 8.0], [10.0, -80.0, 9.0]])
    assert np.isnan(bad[:2, :2]).all() and np.isfinite(bad[2]).all() and np.array_equal(bad[:, 2], [7.0, 8.0, 9.0])


def test_projection_true_scale_at_the_pole():
    """phi_F = -90 degenerates variant B (m_F = t_F = 0): k0 = 1, rho = 2 a t / C, written out here"""
    a, f = 6378137.0, 1.0 / 298.257223563
    e = np.sqrt(2 * f - f * f)
    lat = np.array([-90.0, -85.0, -71.0, -60.0])
    phi = np.deg2rad(lat)
    t = np.tan(np.pi / 4 + phi / 2) / ((1 + e * np.sin(phi)) / (1 - e * np.sin(phi))) ** (e / 2)
    rho = 2 * a * t / np.sqrt((1 + e) ** (1 + e) * (1 - e) ** (1 - e))
    out = gr.polar_stereographic(np.stack([np.full(4, 90.0), lat], axis=1), (a, 298.257223563, -90.0, 0.0, 0.0, 0.0))
    assert out[0].tolist() == [0.0, 0.0]
    assert np.all(np.abs(out[:, 0] - rho) <= 1e-8) and np.all(np.abs(out[:, 1]) <= 1e-8)   # on the 90 E meridian: E = rho, N = 0


def test_region_of_the_references_cloud():
    cloud = 10000 * np.random.RandomState(seed=42).rand(30).reshape(10, 3)   # data_prep.py:365-368
    region, count = gr.region(cloud, 250)
    assert count == 10 and region.tolist() == [500.0, 8500.0, 0.0, 9750.0]
    # the reference prints '-250/9500/0/9750' (gmt info -Is250): the s mode only ever widens the box
    ref = [-250.0, 9500.0, 0.0, 9750.0]
    assert ref[0] <= region[0] and region[1] <= ref[1] and region[2] == ref[2] and region[3] == ref[3]
    # negative coordinates (floor and ceil are not truncation), exact multiples stay, non-finite rows do not count
    pts = np.array([[-1.0, -251.0, 0.0], [250.0, 500.0, 0.0], [np.nan, 9e9, 0.0], [9e9, 1.0, np.inf]])
    region, count = gr.region(pts, 250)
    assert count == 2 and region.tolist() == [-250.0, 250.0, -500.0, 500.0]
    region, count = gr.region(np.full((3, 3), np.nan), 250)
    assert count == 0 and np.isnan(region).all()


def test_blockmedian_of_the_references_cloud():
    cloud = 600 * np.random.RandomState(seed=42).rand(60).reshape(20, 3)   # data_prep.py:393-396
    region, _ = gr.region(cloud, 250)
    assert region.tolist() == [0.0, 750.0, 0.0, 750.0]
    assert gr.block_shape(region, 250) == (4, 4)
    table, grid, counts = gr.blockmedian(cloud, region, 250)
    filled = np.flatnonzero(counts.ravel())
    assert filled.tolist() == [4, 5, 6, 8, 9, 10, 12, 13, 14]          # the north row is empty
    assert counts.ravel()[filled].tolist() == [2, 3, 2, 2, 2, 2, 1, 5, 1]
    assert table.shape == (9, 3)
    assert np.all(np.abs(table[0] - [27.742, 532.649, 257.968]) <= 5e-4)
    assert np.all(np.abs(table[-1] - [424.844, 12.351, 581.946]) <= 5e-4)
    single = cloud[gr.assign(cloud, region, 250) == 14]
    assert single.shape == (1, 3) and np.array_equal(table[-1], single[0])   # one point: that point
    assert np.isnan(grid[0]).all() and np.array_equal(np.isnan(grid), counts == 0)
    assert np.array_equal(grid.ravel()[filled], table[:, 2].astype(np.float32))


def test_blockmedian_edges_and_ties():
    region = (0.0, 500.0, 0.0, 250.0)   # (2, 3) blocks, north row first
    pts = np.array([
        [125.0, 250.0, 1.0],     # exactly on the boundary between columns 0 and 1: east
        [0.0, 125.0, 2.0],       # exactly on the boundary between rows 0 and 1: south
        [-125.0, 0.0, 3.0],      # half a block west of xmin: used
        [625.0, 0.0, 4.0],       # half a block east of xmax: not used
        [0.0, 375.0, 5.0],       # half a block north of ymax: row = floor(-0.5 + 0.5) = 0, used (a tie goes south)
        [0.0, -125.0, 6.0],      # half a block south of ymin: row = floor(1.5 + 0.5) = 2 = H, not used
    ])
    blk = gr.assign(pts, region, 250)
    assert blk.tolist() == [1, 3, 3, -1, 0, -1]
    # an even count halves the sum of the two middle values; zeros of both signs have an order
    z = np.array([3.0, 1.0, 2.0, 4.0])
    t, _, _ = gr.blockmedian(np.stack([np.zeros(4), np.zeros(4), z], axis=1), (0, 0, 0, 0), 250)
    assert t.tolist() == [[0.0, 0.0, 2.5]]
    t, _, _ = gr.blockmedian(np.array([[0.0, 0.0, -0.0], [0.0, 0.0, 0.0], [0.0, 0.0, -0.0]]), (0, 0, 0, 0), 250)
    assert np.signbit(t[0, 2]) and not np.signbit(t[0, 0])


def test_blockmedian_against_pandas_groupby():
    pd = pytest.importorskip("pandas")
    for seed, n, region, inc in ((1, 5000, (0.0, 5000.0, -2500.0, 2500.0), 250.0), (2, 20000, (-2000000.0, -1990000.0, 100000.0, 103000.0), 250.0),
                                 (3, 777, (0.0, 30.0, 0.0, 70.0), 10.0)):
        r = np.random.default_rng(seed)
        xmin, xmax, ymin, ymax = region
        pts = np.stack([r.uniform(xmin - inc, xmax + inc, n).round(2), r.uniform(ymin - inc, ymax + inc, n).round(2),
                        r.normal(0, 3000, n)], axis=1)
        table, _, counts = gr.blockmedian(pts, region, inc)
        blk = gr.assign(pts, region, inc)
        df = pd.DataFrame({"block": blk, "x": pts[:, 0], "y": pts[:, 1], "z": pts[:, 2]})
        want = df[df.block >= 0].groupby("block").median()
        assert np.array_equal(want.index.to_numpy(), np.flatnonzero(counts.ravel()))
        assert np.array_equal(want[["x", "y", "z"]].to_numpy().view(np.uint64), table.view(np.uint64))   # bit for bit


def test_size_classes_of_the_header_and_the_bindings_agree():
    from deepbedmap_amd import gridding

    text = open(os.path.join(os.path.dirname(HERE), "include", "dbm.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"\b(DBM_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    for name in ("POINTS_THREADS", "BLOCKMEDIAN_SUB8", "BLOCKMEDIAN_SUB32", "BLOCKMEDIAN_WAVE", "BLOCKMEDIAN_LDS"):
        assert consts["DBM_" + name] == getattr(gridding, name), name
    b = gridding.BLOCKMEDIAN_CLASS_BOUNDARIES
    assert list(b) == sorted(set(b)) and len(b) + 1 == consts["DBM_BLOCKMEDIAN_CLASSES"]


def test_host_side_refusals_need_no_gpu():
    import deepbedmap_amd as dbm

    lonlat = np.array([[10.0, -80.0, 1.0]])
    for pair in (("EPSG:4326", "EPSG:3413"), ("EPSG:3031", "EPSG:4326"), ("EPSG:4326", "EPSG:4326")):
        with pytest.raises(ValueError, match="supported"):
            dbm.reproject(lonlat, *pair)
    with pytest.raises(ValueError, match="latitude"):
        dbm.reproject(np.array([[10.0, 0.5, 1.0]]))
    with pytest.raises(ValueError, match="latitude"):
        dbm.reproject(np.array([[10.0, -90.5, 1.0]]))
    with pytest.raises(ValueError):
        dbm.reproject(np.zeros((3,)))
    xyz = np.zeros((4, 3))
    for bad in ("0/750/0", "0/750/0/abc", "0/750/0/750/1", "750/0/0/750", "0/750/750/0", "0/inf/0/750", (0, 1, 2), None):
        with pytest.raises(ValueError, match="region"):
            dbm.blockmedian(xyz, bad)
    for bad in (0, -250, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="spacing"):
            dbm.blockmedian(xyz, "0/750/0/750", spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            dbm.get_region(xyz, round_increment=bad)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        dbm.blockmedian(np.zeros((4, 4)), "0/750/0/750")
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        dbm.blockmedian_grid(np.zeros((4, 2)), "0/750/0/750")
    with pytest.raises(ValueError, match="2\\^31"):
        dbm.block_shape("0/1e9/0/1e9", 1)
    assert dbm.parse_region(" 0/750/-250/9750 ") == (0.0, 750.0, -250.0, 9750.0)
    assert dbm.block_shape("0/750/0/750", 250) == (4, 4) and dbm.block_shape((0, 600, 0, 0), 250) == (1, 3)
    g = dbm.block_geometry((0.0, 1325.0, -850.0, 0.0), 250)   # 5.3 and 3.4 spacings: (4, 6) blocks, the north edge fitted (+e)
    assert dbm.block_shape((0.0, 1325.0, -850.0, 0.0), 250) == (4, 6) and (g.x0, g.y0) == (0.0, -100.0)
    assert gr.north_edge((0.0, 1325.0, -850.0, 0.0), 250) == -100.0
    g = dbm.block_geometry("0/750/0/500", 250)
    assert (g.x0, g.y0, g.dx, g.dy, g.registration) == (0.0, 500.0, 250.0, -250.0, "gridline")
