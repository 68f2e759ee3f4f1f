"""CPU checks of the comparison grids' yardstick (tests/comparison_restatement.py, NumPy only) against scipy.ndimage and numpy.nanstd, and
of the argument validation of deepbedmap_amd/comparison.py (which raises before the library is touched).

Tolerance of the restatement against scipy on DEM-range inputs (U(-2000, 2000)): the worst absolute difference over every case below
was measured as 9.1e-13 (scipy 1.15.3; the orders, scales, shapes, casts and clips of `cases()`); asserted at 16 x that, 1.5e-11 -- the
margin is for summation order: scipy's recursion start values are closed forms, the restatement's are sums, and the B-spline weights
are applied in another order.  Inputs in [0, 1) are held to the same bound scaled by 1 / 2000."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import comparison_restatement as cr  # noqa: E402

MEASURED_WORST = 9.1e-13
TOL_DEM = 16 * MEASURED_WORST

SCALES = [4, 2, 1 / 2.5, (3, 0.5)]
ORDERS = [1, 3]
# odd sizes, axes of length 2, 3 and 5 (shorter than any warm-up), one a few hundred nodes long
SHAPES = [(37, 53), (2, 3), (3, 5), (5, 2), (2, 2), (101, 64), (5, 301)]


def dem(shape, seed):
    return np.random.default_rng(seed).uniform(-2000.0, 2000.0, shape)


def scipy_rescale(x, scale, order, anti_aliasing=True, clip=True, as_int=False):
    """the scipy call chain of current scikit-image's rescale / resize (mode="reflect" there is ndimage's "mirror")"""
    from scipy import ndimage

    x = np.asarray(x)
    x = (x.astype(np.int32) if as_int else x).astype(np.float64)
    out_h, out_w = cr.output_shape(x.shape, scale)
    lo, hi = x.min(), x.max()
    if anti_aliasing:
        sigma = [max(0.0, (x.shape[0] / out_h - 1) / 2), max(0.0, (x.shape[1] / out_w - 1) / 2)]
        x = ndimage.gaussian_filter(x, sigma, mode="mirror")
    y = ndimage.zoom(x, (out_h / x.shape[0], out_w / x.shape[1]), order=order, mode="mirror", grid_mode=True)
    assert y.shape == (out_h, out_w)
    return np.clip(y, lo, hi) if clip else y


def cases():
    for shape in SHAPES:
        for scale in SCALES:
            if min(cr.output_shape(shape, scale)) < 1:
                continue
            for order in ORDERS:
                yield shape, scale, order


@pytest.mark.parametrize("shape,scale,order", list(cases()))
def test_rescale_restatement_matches_scipy(shape, scale, order):
    x = dem(shape, seed=shape[0] * 1000 + shape[1])
    worst = 0.0
    for clip in (True, False):
        for as_int in (False, True):
            got = cr.rescale64(x, scale, order, True, clip, as_int)
            want = scipy_rescale(x, scale, order, True, clip, as_int)
            assert got.shape == want.shape
            worst = max(worst, float(np.abs(got - want).max()))
    got = cr.rescale64(x, scale, order, anti_aliasing=False, clip=False)
    worst = max(worst, float(np.abs(got - scipy_rescale(x, scale, order, anti_aliasing=False, clip=False)).max()))
    print("worst |restatement - scipy|", worst)
    assert worst <= TOL_DEM, worst


def test_rescale_restatement_matches_scipy_on_unit_range():
    x = np.random.default_rng(5).random((41, 29))
    for scale in SCALES:
        for order in ORDERS:
            d = np.abs(cr.rescale64(x, scale, order) - scipy_rescale(x, scale, order)).max()
            assert d <= TOL_DEM / 2000.0, (scale, order, d)


def test_pieces_match_scipy():
    from scipy import ndimage

    x = dem((23, 7), 3)
    for sigma in (0.5, 0.75, 3.2):
        assert np.abs(cr.gaussian_axis0(x, sigma) - ndimage.gaussian_filter1d(x, sigma, axis=0, mode="mirror")).max() <= TOL_DEM
    for n in (2, 3, 5, 23):
        y = dem((n, 4), n)
        assert np.abs(cr.prefilter_axis0(y) - ndimage.spline_filter1d(y, order=3, axis=0, mode="mirror")).max() <= TOL_DEM
    assert cr.output_shape((45000, 55000), 1 / 2.5) == (18000, 22000)
    assert cr.output_shape((5, 5), 0.5) == (2, 2)   # NumPy rounds 2.5 to the even neighbour


def test_clip_matters_and_is_applied():
    x = dem((40, 40), 11)
    free = cr.rescale64(x, 4, order=3, clip=False)
    assert free.min() < x.min() and free.max() > x.max()   # the cubic spline overshoots a rough grid
    held = cr.rescale64(x, 4, order=3, clip=True)
    assert held.min() >= x.min() and held.max() <= x.max()
    xi = x.astype(np.int32).astype(np.float64)
    cast = cr.rescale64(x, 4, order=3, clip=True, as_int=True)
    assert cast.min() >= xi.min() and cast.max() <= xi.max()
    assert np.array_equal(cast, cr.rescale64(xi, 4, order=3, clip=True))
    assert cr.rescale(x, 2, order=1).dtype == np.float32
    assert cr.cubic_bedmap(x[None, None]).shape == (1, 1, 4 * 38, 4 * 38)


def brute_force_std(g, window):
    import warnings

    h = window // 2
    H, W = g.shape
    out = np.full((H, W), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for r in range(H):
            for c in range(W):
                out[r, c] = np.nanstd(g[max(0, r - h):r + h + 1, max(0, c - h):c + h + 1])
    return out


def test_roughness_reproduces_the_reference_doctest():
    doc = json.load(open(os.path.join(HERE, "golden", "paper_figures_doctests.json")))["standard_deviation_2d"]
    grid = np.arange(doc["grid"]["arange"][0], doc["grid"]["arange"][1], doc["grid"]["arange"][2]).reshape(doc["grid"]["shape"])
    got = cr.standard_deviation_2d64(grid, doc["window_length"])
    want = np.array(doc["result"])
    assert got.shape == want.shape == (3, 5)
    # the doctest prints six significant digits
    for g, w in zip(got.ravel(), want.ravel()):
        assert ("%.6f" % g).rstrip("0") == ("%.6f" % w).rstrip("0"), (g, w)


@pytest.mark.parametrize("window", [1, 3, 5, 9])
def test_roughness_matches_nanstd_brute_force(window):
    r = np.random.default_rng(window)
    g = r.uniform(-2000.0, 2000.0, (33, 41))
    g[r.random(g.shape) < 0.1] = np.nan           # holes
    g[:7] = g[-7:] = np.nan                        # a NaN frame wider than the window's half-width
    g[:, :7] = g[:, -7:] = np.nan
    g[12:24, 10:22] = np.nan                       # a block that leaves whole windows empty
    g[26:31, 30:36] = 1234.5                       # a constant plateau
    got = cr.standard_deviation_2d64(g, window)
    want = brute_force_std(g, window)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got).sum() > 100 and np.isfinite(got).sum() > 300
    m = np.isfinite(want)
    # both are float64: n <= 81 terms, the shifted form loses at most a factor n + 1 to cancellation (the shift is a node of the window),
    # so the variance is good to about n (n + 1) 2^-53 = 7e-13 relative, the root to half that, on values up to 4000: 2e-9 absolute
    print("worst |restatement - nanstd|", np.abs(got[m] - want[m]).max())
    assert np.abs(got[m] - want[m]).max() <= 2e-9, np.abs(got[m] - want[m]).max()
    if window <= 5:
        assert np.all(got[28, 32:34] == 0.0)       # a constant window gives exactly 0
    assert cr.standard_deviation_2d(g, window).dtype == np.float32


def test_roughness_window_rules():
    g = np.zeros((4, 4))
    for bad in (0, 2, 4, 64, 65, -1):
        with pytest.raises(ValueError):
            cr.standard_deviation_2d64(g, bad)
    assert np.all(cr.standard_deviation_2d64(g + 3.3, 63) == 0.0)


def test_python_layer_validates_before_the_library_is_touched(monkeypatch):
    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib, comparison

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "default_context", boom)
    x = np.zeros((6, 7), dtype=np.float32)
    for order in (0, 2, 4, 5, "cubic"):
        with pytest.raises(ValueError, match="order"):
            dbm.rescale(x, 2, order=order)
    with pytest.raises(ValueError, match="2 x 2"):
        dbm.rescale(np.zeros((1, 9), dtype=np.float32), 2)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        dbm.rescale(np.zeros((2, 3, 4, 5), dtype=np.float32), 2)
    for scale in (0, -1.0, float("nan"), float("inf"), (1, 2, 3)):
        with pytest.raises(ValueError, match="scale"):
            dbm.rescale(x, scale)
    with pytest.raises(TypeError, match="scale"):
        dbm.rescale(x, "big")
    with pytest.raises(ValueError, match="no output node"):
        dbm.rescale(x, 0.01)
    for window in (0, 2, 4, 64, 65, -3):
        with pytest.raises(ValueError, match="window_length"):
            dbm.standard_deviation_2d(x, window)
    with pytest.raises(TypeError, match="window_length"):
        dbm.standard_deviation_2d(x, 3.0)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        dbm.standard_deviation_2d(np.zeros((2, 2, 2), dtype=np.float32), 3)
    with pytest.raises(ValueError, match=r"\(1, 1, h, w\)"):
        dbm.cubic_bedmap(x)
    with pytest.raises(ValueError, match="interior"):
        dbm.cubic_bedmap(np.zeros((1, 1, 3, 9), dtype=np.float32))
    geom = dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    pts = np.zeros((4, 3))
    with pytest.raises(TypeError, match="grids"):
        dbm.compare_on_tracks(pts, [(x, geom)])
    with pytest.raises(TypeError, match="GridGeometry"):
        dbm.compare_on_tracks(pts, {"a": (x, (0, 0, 1, 1))})
    with pytest.raises(ValueError, match="z column"):
        dbm.compare_on_tracks(pts[:, :2], {"a": (x, geom)})
    assert comparison.rescale_output_shape((45000, 55000), 1 / 2.5) == (18000, 22000)
    assert comparison.rescale_output_shape((10, 10), (3, 0.5)) == (30, 5)
