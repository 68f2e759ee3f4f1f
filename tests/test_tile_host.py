"""CPU checks of the tiling semantics (tests/tile_restatement.py: what dbm_grid_tile and dbm_grid_filled_windows compute) against
scipy.interpolate.interpn -- the engine under the reference's `DataArray.interp(method="linear")` --, numpy.ma.masked_values and the
reference's two doctest answers (tests/golden/data_prep_doctests.json), and of the host side of deepbedmap_amd/tiling.py: the tile size
rule, the alignment check of interpolate=False, the bounds arithmetic, the argument refusals and the loud failure without a GPU."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tile_restatement as tl  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402
from deepbedmap_amd import tiling  # noqa: E402

# (raster spacing, tile resolution) of X / W3, a 500 m raster, W2, W1 and Y (data_prep.py:757-771, 880-911)
PAIRINGS = [(1000.0, 1000.0), (500.0, 500.0), (450.0, 500.0), (100.0, 100.0), (250.0, 250.0)]


def _raster(H, W, d, seed, north_up=True, nans=30):
    """Node coordinates at multiples of half a pixel (exact in float64), `nans` scattered NaN nodes."""
    r = np.random.default_rng(seed)
    g = (r.normal(0.0, 300.0, (H, W)) + 1000.0).astype(np.float32)
    g.ravel()[r.choice(H * W, nans, replace=False)] = np.nan
    x0 = -1_000_000.0 + 0.5 * d * 7
    ytop = 500_000.0 + 0.5 * d * 3
    geom = (x0, ytop, d, -d) if north_up else (x0, ytop - (H - 1) * d, d, d)
    return g, geom


def _windows(geom, H, W, res, npix, seed):
    """Windows of npix x npix output pixels whose pixel centres sit at multiples of half a raster pixel: inside the raster, with
    centres ON nodes, on the first and the last node, and hanging over each of the four edges."""
    x0, y0, dx, dy = geom
    d = abs(dx)
    xs = np.sort([x0, x0 + (W - 1) * dx])
    ys = np.sort([y0, y0 + (H - 1) * dy])
    size = npix * res
    r = np.random.default_rng(seed)
    out = []

    def add(cx_first, cy_top):   # centre of the first (west, north) pixel
        left, top = cx_first - res / 2, cy_top + res / 2
        out.append((left, top - size, left + size, top))

    for _ in range(12):   # anywhere inside, centres at multiples of d / 2 (half of them on nodes when the parity agrees)
        add(xs[0] + 0.5 * d * r.integers(0, 2 * (W - 1) - int(2 * size / d)), ys[1] - 0.5 * d * r.integers(0, 2 * (H - 1) - int(2 * size / d)))
    add(xs[0], ys[1])                                             # the first pixel centre on the north-west node
    add(xs[1] - (npix - 1) * res, ys[0] + (npix - 1) * res)       # the last pixel centre on the south-east node
    add(xs[0] - 2.5 * d, ys[1] - 3 * d)                           # over the west edge
    add(xs[1] - 2 * d, ys[1] - 3 * d)                             # over the east edge
    add(xs[0] + 3 * d, ys[1] + 1.5 * d)                           # over the north edge
    add(xs[0] + 3 * d, ys[0] + 2 * d)                             # over the south edge
    add(xs[1] + 5 * d, ys[0] - 5 * d - size)                      # entirely outside
    return out


def _interpn(g, geom, ys, xs):
    scipy_interp = pytest.importorskip("scipy.interpolate")
    H, W = g.shape
    x0, y0, dx, dy = geom
    gy, gx = y0 + np.arange(H) * dy, x0 + np.arange(W) * dx
    vals = g
    if dy < 0:
        gy, vals = gy[::-1], vals[::-1]
    if dx < 0:
        gx, vals = gx[::-1], vals[:, ::-1]
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return scipy_interp.interpn((gy, gx), vals, np.stack([yy, xx], axis=-1), method="linear", bounds_error=False, fill_value=np.nan)


def _bit_equal_f32(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (np.isnan(got).sum(), np.isnan(want).sum())
    a, b = got.astype(np.float32), want.astype(np.float32)
    m = ~np.isnan(want)
    assert np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32)), np.abs(a[m] - b[m]).max()


@pytest.mark.parametrize("north_up", [True, False])
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_restatement_is_scipys_interpn_bit_for_bit(pairing, north_up):
    d, res = pairing
    H, W = 40, 50
    g, geom = _raster(H, W, d, seed=int(d) + north_up, north_up=north_up)
    wins = _windows(geom, H, W, res, 7, seed=int(res))
    nan_seen = on_node = 0
    for wb in wins:
        ys, xs = tl.window_coords(wb, res, 7, 7)
        got = tl.bilinear(g, (H, W), geom, ys, xs)
        want = _interpn(g, geom, ys, xs)
        _bit_equal_f32(got, want)
        nan_seen += int(np.isnan(want).sum())
        on_node += int(np.isin(xs, geom[0] + np.arange(W) * geom[2]).sum())
    assert nan_seen > 0 and on_node > 0
    # the whole call: shape from the first window, float32 once at the end
    tiles, _ = tl.tile(g, (H, W), geom, wins, resolution=res)
    assert tiles.shape == (len(wins), 1, 7, 7) and tiles.dtype == np.float32
    assert np.isnan(tiles[-1]).all()     # the window outside the raster


def test_a_nan_node_spoils_its_closed_cell_as_in_scipy_1_15():
    """Zero weights are not skipped (0 * NaN = NaN): with a NaN at [10, 10] of a north-up grid, samples ON the nodes come out NaN at
    rows 10-11, columns 9-10 (scipy 1.15.3; older versions pick the other cell for on-node samples)."""
    H, W = 20, 20
    g = np.arange(H * W, dtype=np.float32).reshape(H, W)
    g[10, 10] = np.nan
    geom = (0.0, 19000.0, 1000.0, -1000.0)
    ys, xs = 19000.0 - 1000.0 * np.arange(H), 1000.0 * np.arange(W)
    got = tl.bilinear(g, (H, W), geom, ys, xs)
    assert sorted(map(tuple, np.argwhere(np.isnan(got)))) == [(10, 9), (10, 10), (11, 9), (11, 10)]
    _bit_equal_f32(got, _interpn(g, geom, ys, xs))
    m = ~np.isnan(got)
    assert np.array_equal(got[m], g.astype(np.float64)[m])


def test_last_node_outside_and_nan_coordinates():
    g = np.array([[1, 2, 4], [8, 16, 32]], dtype=np.float32)
    geom = (10.0, 5.0, 2.0, -2.0)   # x nodes 10, 12, 14; y nodes 5, 3
    v = tl.bilinear(g, (2, 3), geom, np.array([5.0, 3.0, 4.0, 5.0000001, np.nan]), np.array([10.0, 14.0, 13.0, 9.9999999, 14.0000001]))
    assert v[0, 0] == 1 and v[0, 1] == 4 and v[1, 0] == 8 and v[1, 1] == 32 and v[2, 2] == 0.25 * (2 + 4 + 16 + 32)
    assert np.isnan(v[3]).all() and np.isnan(v[4]).all() and np.isnan(v[:, 3]).all() and np.isnan(v[:, 4]).all()
    i, t, bad = tl.cells(np.array([14.0]), np.array([10.0, 12.0, 14.0]))
    assert i[0] == 1 and t[0] == 1.0 and not bad[0]


def test_output_coordinates_are_numpys_linspace():
    wb = (-1593250.0 - 1000.0, -1090250.0 - 1000.0, -1593250.0 + 9000.0 + 1000.0, -1090250.0 + 9000.0 + 1000.0)
    ys, xs = tl.window_coords(wb, 100.0, 110, 110)
    assert ys[0] == wb[3] - 50.0 and ys[-1] == wb[1] + 50.0 and xs[0] == wb[0] + 50.0 and xs[-1] == wb[2] - 50.0
    rows = tiling._linspace_rows(np.array([wb[3] - 50.0, 0.1]), np.array([wb[1] + 50.0, 0.7]), 110)   # the host layer's vector form
    assert np.array_equal(rows[0], ys) and np.array_equal(rows[1], np.linspace(0.1, 0.7, 110))
    assert np.array_equal(tiling._linspace_rows(np.array([3.0]), np.array([9.0]), 1), [[3.0]])


@pytest.mark.parametrize("nodata", [-9999.0, 0.0, 32767.0, -3.4028234663852886e38, float("nan")])
def test_mask_rule_is_numpys_masked_values(nodata):
    r = np.random.default_rng(5)
    base = 0.0 if np.isnan(nodata) else nodata
    v = np.concatenate([r.normal(0, 1000, 200), base * (1 + r.uniform(-3e-5, 3e-5, 400)), base + r.uniform(-3e-8, 3e-8, 200),
                        [base, base * (1 + 2e-5), base * (1 - 2e-5), np.nan, np.inf, -np.inf, -9999.0, np.finfo(np.float64).min]])
    value = np.nan_to_num(nodata, nan=np.nan_to_num(-np.inf))     # data_prep.py:702
    want = np.ma.getmaskarray(np.ma.masked_values(v, value))
    got = tl.mask_rule(v, nodata)
    if np.isnan(nodata):
        want = want & (v != np.finfo(np.float64).min)             # (the sentinel itself: no raster holds it)
        assert not got.any()
    assert np.array_equal(got, want)
    if nodata == -9999.0:
        assert got[800] and not got[801] and not got[802] and not got[803]     # inside the band, just outside on both sides, NaN
    assert not tl.mask_rule(v, None).any()


def _doctests():
    with open(os.path.join(HERE, "golden", "data_prep_doctests.json")) as fh:
        return json.load(fh)


def test_selective_tile_doctest_answer():
    d = _doctests()["selective_tile"]
    g = np.array(d["raster"], dtype=np.float32)
    geom = dbm.GridGeometry.from_coords(d["x"], d["y"])
    tiles, counts = tl.tile(g, g.shape, tuple(geom.as_array()), d["window_bounds"])
    assert tiles.dtype == np.float32 and np.array_equal(tiles, np.array(d["expected"], dtype=np.float32)) and not counts.any()
    assert tiling.tile_shape(d["window_bounds"], 0, 1.0) == (2, 2)
    mode, windows, res, h, w = tiling._plan(dbm.Raster(g, geom), d["window_bounds"], 0, None, None, True)
    assert (mode, res, h, w) == (1, 1.0, 2, 2) and np.array_equal(windows, [[0.5, 0.5, 2.5, 2.5], [2.5, 1.5, 4.5, 3.5]])


def test_get_window_bounds_doctest_answer():
    d = _doctests()["get_window_bounds"]
    g = np.full(d["shape"], d["fill"], dtype=np.float32)
    geom = dbm.GridGeometry.from_coords(d["x"], d["y"])        # y ascending: row 0 is the south edge
    flags = tl.filled_windows(g, tuple(geom.as_array()), d["height"], d["step"])
    assert flags.shape == (2, 1) and flags.all()
    got = tiling.bounds_from_flags(flags, geom, g.shape, d["height"], d["step"])
    assert got == [tuple(b) for b in d["expected"]]


def test_bounds_arithmetic_from_a_flag_array():
    H, W, size, step = 50, 61, 36, 3
    flags = np.zeros(((H - size) // step + 1, (W - size) // step + 1), np.uint8)
    flags[0, 0] = flags[1, 2] = flags[4, 8] = flags[3, 1] = 1
    north_up = dbm.GridGeometry(-1_000_125.0 + 125.0, 2000.0 - 125.0, 250.0, -250.0)     # edges: west -1 000 125, north 2000
    want = [(-1_000_125.0, 2000.0 - 9000.0, -1_000_125.0 + 9000.0, 2000.0),
            (-1_000_125.0 + 2 * 750.0, 2000.0 - 750.0 - 9000.0, -1_000_125.0 + 2 * 750.0 + 9000.0, 2000.0 - 750.0),
            (-1_000_125.0 + 750.0, 2000.0 - 3 * 750.0 - 9000.0, -1_000_125.0 + 750.0 + 9000.0, 2000.0 - 3 * 750.0),
            (-1_000_125.0 + 8 * 750.0, 2000.0 - 4 * 750.0 - 9000.0, -1_000_125.0 + 8 * 750.0 + 9000.0, 2000.0 - 4 * 750.0)]
    assert tiling.bounds_from_flags(flags, north_up, (H, W), size, step) == want       # row-major (uly, ulx)
    south_up = north_up.flipped_rows(H)
    assert tiling.bounds_from_flags(flags, south_up, (H, W), size, step) == want       # the same nodes, the other row order
    east_first = dbm.GridGeometry(north_up.x0 + (W - 1) * 250.0, north_up.y0, -250.0, -250.0)
    assert tiling.bounds_from_flags(flags, east_first, (H, W), size, step) == want
    # every bound is a window the slicing path accepts: 36 x 36 nodes
    g = np.zeros((H, W), np.float32)
    for geom in (north_up, south_up, east_first):
        mode, windows, _, h, w = tiling._plan(dbm.Raster(g, geom), want, 0, None, None, False)
        assert (mode, h, w) == (0, 36, 36)
        rstep, cstep = (1 if geom.dy < 0 else -1), (1 if geom.dx > 0 else -1)
        assert np.array_equal(windows[:, 2], [rstep] * 4) and np.array_equal(windows[:, 3], [cstep] * 4)
        assert np.array_equal(windows[:, 0], [0, 3, 9, 12] if rstep == 1 else [H - 1, H - 4, H - 10, H - 13])
        assert np.array_equal(windows[:, 1], [0, 6, 3, 24] if cstep == 1 else [W - 1, W - 7, W - 4, W - 25])


def test_filled_windows_restatement_by_hand():
    g = np.zeros((10, 10), np.float32)
    g[9, 9] = np.nan                      # the very last row and column (north-up: the south-east corner)
    geom = (0.0, 0.0, 1.0, -1.0)
    f = tl.filled_windows(g, geom, 4, 2)  # ny = nx = 4: windows at 0, 2, 4, 6
    assert f.tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]]
    f = tl.filled_windows(g, (0.0, 0.0, 1.0, 1.0), 4, 2)    # row 9 is now the NORTH edge: window row 0 holds it
    assert f.tolist() == [[1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    f = tl.filled_windows(g, (0.0, 0.0, -1.0, -1.0), 4, 2)  # ... and column 9 the WEST edge
    assert f.tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 1, 1]]
    f = tl.filled_windows(g[:9, :9], geom, 4, 3)  # 9 - 4 = 5: ny = nx = 2, windows at 0 and 3; rows and columns 7-8 are never covered
    assert f.tolist() == [[1, 1], [1, 1]]
    g[6, 2] = np.nan
    assert tl.filled_windows(g[:9, :9], geom, 4, 3).tolist() == [[1, 1], [0, 1]]


def test_tile_size_comes_from_the_first_window():
    g = np.zeros((40, 40), np.float32)
    r = dbm.Raster(g, dbm.GridGeometry(500.0, 39500.0, 1000.0, -1000.0))
    wins = [(5000.0, 5000.0, 14000.0, 14000.0), (5000.0, 5000.0, 9000.0, 30000.0)]
    assert tiling._plan(r, wins, 1000, None, None, True)[3:] == (11, 11)
    assert tiling._plan(r, wins[::-1], 1000, None, None, True)[3:] == (27, 6)
    assert tiling._plan(r, wins, 1000, 500, None, True)[3:] == (22, 22)
    assert tiling._plan(r, wins, 1000, 100, None, True)[3:] == (110, 110)
    assert tiling._plan(r, wins, 0, 250, None, True)[3:] == (36, 36)
    assert tiling._plan(r, [(0.0, 0.0, 9999.0, 9000.5)], 0, None, None, True)[3:] == (9, 9)    # int() truncates
    # the restatement follows the same rule
    assert tl.tile(g, (40, 40), (500.0, 39500.0, 1000.0, -1000.0), wins, padding=1000)[0].shape == (2, 1, 11, 11)


def test_slicing_demands_windows_that_cut_the_grid_at_its_nodes():
    H, W = 60, 70
    g = np.arange(H * W, dtype=np.float32).reshape(H, W)
    geom = dbm.GridGeometry(-1_000_000.0 + 125.0, 200_000.0 - 125.0, 250.0, -250.0)
    r = dbm.Raster(g, geom)
    good = [(-1_000_000.0 + 750.0, 200_000.0 - 750.0 - 9000.0, -1_000_000.0 + 750.0 + 9000.0, 200_000.0 - 750.0),
            (-1_000_000.0, 200_000.0 - 9000.0, -1_000_000.0 + 9000.0, 200_000.0)]
    mode, windows, res, h, w = tiling._plan(r, good, 0, None, None, False)
    assert (mode, res, h, w) == (0, 250.0, 36, 36) and windows.tolist() == [[3, 3, 1, 1], [0, 0, 1, 1]]
    # the restatement slices the same nodes
    tiles, _ = tl.tile(g, (H, W), tuple(geom.as_array()), good, interpolate=False)
    assert np.array_equal(tiles[0, 0], g[3:39, 3:39]) and np.array_equal(tiles[1, 0], g[0:36, 0:36])
    for k, shift in ((1, (1.0, 0.0)), (0, (0.0, 1.0)), (1, (-1.0, -1.0))):
        bad = [list(b) for b in good]
        bad[k] = [bad[k][0] + shift[0], bad[k][1] + shift[1], bad[k][2] + shift[0], bad[k][3] + shift[1]]
        with pytest.raises(ValueError, match=f"window {k} "):
            tiling._plan(r, bad, 0, None, None, False)
        with pytest.raises(ValueError, match=f"window {k} "):
            dbm.selective_tile(r, bad, interpolate=False)
        with pytest.raises(KeyError):
            tl.tile(g, (H, W), tuple(geom.as_array()), bad, interpolate=False)
    outside = [(good[1][0] - 250.0, good[1][1], good[1][2] - 250.0, good[1][3])]      # aligned, but one column west of the raster
    with pytest.raises(ValueError, match="window 0 "):
        dbm.selective_tile(r, outside, interpolate=False)
    with pytest.raises(ValueError, match="cannot resample"):
        dbm.selective_tile(r, good, resolution=500, interpolate=False)
    with pytest.raises(ValueError, match="window 0 "):
        dbm.selective_tile(r, good, padding=100, interpolate=False)    # half a pixel off after the padding


def test_argument_refusals_come_before_the_library_is_touched():
    g = np.zeros((40, 40), np.float32)
    geom = dbm.GridGeometry(500.0, 39500.0, 1000.0, -1000.0)
    r = dbm.Raster(g, geom)
    wins = [(5000.0, 5000.0, 14000.0, 14000.0)]
    with pytest.raises(TypeError, match="Raster"):
        dbm.selective_tile(g, wins)
    with pytest.raises(TypeError, match="GridGeometry"):
        dbm.Raster(g, (500.0, 39500.0, 1000.0, -1000.0))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        dbm.Raster(np.zeros((2, 4, 4), np.float32), geom)
    with pytest.raises(ValueError, match="empty raster"):
        dbm.Raster(np.zeros((0, 4), np.float32), geom)
    with pytest.raises(ValueError, match="nodata"):
        dbm.Raster(g, geom, nodata=float("inf"))
    for bad in ([], [(0.0, 0.0, 1.0)], (0.0, 0.0, 1.0, 1.0), [(0.0, 0.0, float("nan"), 1.0)]):
        with pytest.raises(ValueError, match="window_bounds"):
            dbm.selective_tile(r, bad)
    with pytest.raises(ValueError, match="square pixels"):
        dbm.selective_tile(dbm.Raster(g, dbm.GridGeometry(0.0, 0.0, 1000.0, -500.0)), wins)
    for res in (0, -500, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution"):
            dbm.selective_tile(r, wins, resolution=res)
    with pytest.raises(ValueError, match="padding"):
        dbm.selective_tile(r, wins, padding=float("nan"))
    with pytest.raises(ValueError, match="gapfiller"):
        dbm.selective_tile(r, wins, gapfiller=float("nan"))
    with pytest.raises(ValueError, match="empty tiles"):
        dbm.selective_tile(r, [(0.0, 0.0, 900.0, 5000.0)])
    with pytest.raises(ValueError, match="empty tiles"):
        dbm.selective_tile(r, wins, padding=-4600)
    with pytest.raises(ValueError, match="2 x 2"):
        dbm.selective_tile(dbm.Raster(np.zeros((1, 40), np.float32), geom), wins)
    with pytest.raises(ValueError, match="channel"):
        dbm.selective_tile(r, wins, channel=1)
    with pytest.raises(TypeError, match="DeviceArray"):
        dbm.selective_tile(r, wins, out=np.zeros((1, 1, 9, 9), np.float32))
    for kw in (dict(height=36, width=30), dict(height=35, width=35), dict(height=0, width=0), dict(step=0)):
        with pytest.raises(ValueError, match="square|even|step"):
            dbm.get_window_bounds(r, **kw)
    with pytest.raises(ValueError, match="smaller than one window"):
        dbm.get_window_bounds(r, height=42, width=42)
    with pytest.raises(TypeError, match="Raster"):
        dbm.get_window_bounds(g)
    with pytest.raises(TypeError, match="rema must be a Raster"):
        dbm.get_deepbedmap_model_inputs((5000.0, 5000.0, 14000.0, 14000.0), r, g, r, r, r)
    with pytest.raises(ValueError, match="window_bound"):
        dbm.get_deepbedmap_model_inputs((5000.0, 5000.0, 14000.0), r, r, r, r, r)
    with pytest.raises(ValueError, match="at least one"):
        dbm.tile_training_set([], r, r, r, r, r)
    hi = dbm.Raster(np.zeros((80, 80), np.float32), dbm.GridGeometry(5125.0, 24875.0, 250.0, -250.0))
    w9, w6 = [(5000.0, 5000.0, 14000.0, 14000.0)], [(5000.0, 5000.0, 11000.0, 11000.0)]
    with pytest.raises(ValueError, match="different shapes"):
        dbm.tile_training_set([(hi, w9), (hi, w6)], r, r, r, r, r)
    with pytest.raises(TypeError, match="accumulation must be a Raster"):
        dbm.tile_training_set([(hi, w9)], r, r, r, r, None)
    with pytest.raises(ValueError, match="window 0 "):
        dbm.tile_training_set([(hi, [(5001.0, 5000.0, 14001.0, 14000.0)])], r, r, r, r, r)


def test_raster_from_a_geotiff_written_by_this_package(tmp_path):
    H, W = 6, 10
    bound = (-1593250.0, -1090250.0, -1593250.0 + W * 250.0, -1090250.0 + H * 250.0)
    arr = np.arange(H * W, dtype=np.float32).reshape(1, H, W)
    path = dbm.save_array_to_grid(str(tmp_path / "g"), window_bound=bound, array=arr)
    r = dbm.Raster.from_geotiff(path)
    g = r.geometry
    assert r.shape == (H, W) and r.nodata == -2000.0
    assert (g.x0, g.y0, g.dx, g.dy) == (bound[0] + 125.0, bound[3] - 125.0, 250.0, -250.0)
    assert g == dbm.GridGeometry.from_bounds(bound, H, W)
    assert np.array_equal(r._host, arr[0])
    # the whole file as one window slices back to itself
    assert tiling._plan(r, [bound], 0, None, None, False)[1].tolist() == [[0, 0, 1, 1]]


def test_product_functions_are_not_collected_as_tests():
    assert not [n for n in dir(tiling) if n.startswith("test")]


def test_no_gpu_means_loud_failure():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from deepbedmap_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    g = np.zeros((80, 80), np.float32)
    r = dbm.Raster(g, dbm.GridGeometry(500.0, 79500.0, 1000.0, -1000.0))
    hi = dbm.Raster(g, dbm.GridGeometry(5125.0, 24875.0, 250.0, -250.0))
    wins = [(5000.0, 5000.0, 14000.0, 14000.0)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(dbm.DbmError):
            dbm.selective_tile(r, wins, padding=1000)
        with pytest.raises(dbm.DbmError):
            dbm.selective_tile(hi, wins, interpolate=False)
        with pytest.raises(dbm.DbmError):
            dbm.get_window_bounds(hi)
        with pytest.raises(dbm.DbmError):
            dbm.get_deepbedmap_model_inputs(wins[0], r, r, r, r, r)
        with pytest.raises(dbm.DbmError):
            dbm.tile_training_set([(hi, wins)], r, r, r, r, r)
