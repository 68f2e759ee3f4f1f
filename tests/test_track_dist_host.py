"""CPU checks of the error distribution (DESIGN.md "Error distribution"): tests/track_dist_restatement.py -- what
dbm_track_error_quantiles and dbm_track_error_histogram compute -- against np.quantile, pandas' describe() and np.histogram on seeded
data (values are compared, not the sign of a zero), the argument refusals of the Python layer, the header, and the loud failure without
a GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_dist_restatement as td  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    """equal values (0.0 == -0.0), NaN in the same places"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (got, want)


def _samples(seed):
    """errors of every kind the rule has to get right: continuous, heavily tied, tiny, all equal, one, two"""
    r = np.random.default_rng(seed)
    yield r.normal(-30.0, 80.0, r.integers(3, 400))
    yield r.integers(-5, 6, r.integers(3, 400)).astype(np.float64)            # ties, zeros
    yield r.choice([-1.5, 0.0, 2.25], r.integers(3, 200))                     # three values repeated
    yield r.normal(0.0, 1.0, r.integers(3, 50)) * 5e-324 * 2.0 ** r.integers(0, 40)   # denormals
    yield np.full(r.integers(1, 9), r.normal())                               # all equal
    yield r.normal(size=1)
    yield r.normal(size=2) * 1e150                                            # (squares stay finite for std)


def test_errors_that_take_part():
    pts = np.zeros((7, 3))
    pts[:, 2] = [1.0, np.nan, 2.0, 3.0, 0.0, np.inf, 4.0]
    zi = np.array([1.5, 1.0, np.nan, 3.0, -0.0, 1.0, np.inf])
    e = td.errors(pts, zi)
    assert np.array_equal(e, [0.5, 0.0, 0.0]) and not np.signbit(e).any()    # (3 - 3 = +0, -0 - 0 = -0 -> +0)
    k = td.keys(np.array([-np.inf, -1.0, -5e-324, 0.0, 5e-324, 1.0, np.inf]))
    assert np.all(np.diff(k.astype(object)) > 0)                              # the keys keep the order


@pytest.mark.parametrize("seed", range(40))
def test_quantile_rule_is_numpys(seed):
    r = np.random.default_rng(1000 + seed)
    for e in _samples(seed):
        q = np.concatenate([[0.0, 1.0, 0.25, 0.5, 0.75], r.random(11)])
        r.shuffle(q)
        _same(td.quantiles(e, q), np.quantile(e, q, method="linear"))


@pytest.mark.parametrize("seed", range(10))
def test_describe_is_pandas(seed):
    pd = pytest.importorskip("pandas")
    for e in _samples(100 + seed):
        want = pd.Series(e).describe()
        got = td.describe(e)
        assert list(got) == list(want.index) == ["count", "mean", "std", "min", "25%", "50%", "75%", "max"]
        for k in ("count", "min", "25%", "50%", "75%", "max"):
            _same(got[k], want[k])
        for k in ("mean", "std"):   # (pandas sums in another order)
            assert (np.isnan(got[k]) and np.isnan(want[k])) or abs(got[k] - want[k]) <= 1e-12 * max(abs(want[k]), np.abs(e).max()), k
    other = pd.Series(np.arange(11.0)).describe(percentiles=[0.125, 0.9])
    assert list(td.describe(np.arange(11.0), (0.125, 0.5, 0.9))) == list(other.index)


def test_empty_and_single_inputs():
    pd = pytest.importorskip("pandas")
    assert np.isnan(td.quantiles(np.array([]), [0.0, 0.5, 1.0])).all()
    want = pd.Series(np.array([], dtype=np.float64)).describe()
    got = td.describe(np.array([]))
    assert got["count"] == want["count"] == 0 and all(np.isnan(got[k]) and np.isnan(want[k]) for k in list(got)[1:])
    _same(td.quantiles(np.array([7.5]), [0.0, 0.3, 1.0]), [7.5, 7.5, 7.5])
    _same(td.histogram(np.array([]), np.linspace(0.0, 1.0, 26)), np.histogram(np.array([]), bins=25)[0])
    c, edges = np.histogram(np.array([7.5]), bins=25)
    assert (edges[0], edges[-1]) == (7.0, 8.0)
    _same(td.histogram(np.array([7.5]), edges), c)


@pytest.mark.parametrize("seed", range(40))
def test_histogram_rule_is_numpys(seed):
    r = np.random.default_rng(2000 + seed)
    for e in _samples(200 + seed):
        for bins in (1, 2, 25, int(r.integers(3, 300)), 4096):
            st = dbm.TrackStats(e.size, 0.0, 0.0, e.min(), e.max(), 0.0)
            try:
                want, edges = np.histogram(e, bins=bins)
            except ValueError:   # more bins than a range of denormals has values: NumPy refuses, and so does the layer built on it
                with pytest.raises(ValueError, match="Too many bins"):
                    dbm.evaluation.histogram_edges(st, bins)
                continue
            _same(td.histogram(e, edges), want)
            _same(dbm.evaluation.histogram_edges(st, bins), edges)
            lo, hi = np.sort(r.uniform(e.min() - 1.0, e.max() + 1.0, 2))     # often narrower than the data
            if lo < hi:
                want, edges = np.histogram(e, bins=bins, range=(lo, hi))
                _same(td.histogram(e, edges), want)


def test_histogram_values_on_edges_and_beside_them():
    e = np.arange(-200.0, 151.0)                                              # integer errors, range (-150, 100), 25 bins of 10
    want, edges = np.histogram(e, bins=25, range=(-150, 100))
    assert np.array_equal(edges, np.arange(-150.0, 101.0, 10.0))
    got = td.histogram(e, edges)
    _same(got, want)
    assert got.sum() == 251 and got[-1] == 11 and np.all(got[:-1] == 10)      # the right edge belongs to the last bin
    edges = np.linspace(-0.7, 0.9, 26)
    beside = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
    _same(td.histogram(beside, edges), np.histogram(beside, bins=25, range=(-0.7, 0.9))[0])
    _same(dbm.evaluation.histogram_edges(dbm.evaluation._NO_STATS, 25), np.histogram(np.array([]), bins=25)[1])      # (0, 1)
    _same(dbm.evaluation.histogram_edges(dbm.TrackStats(3, 2.0, 0.0, 2.0, 2.0, 2.0), 4), np.histogram(np.full(3, 2.0), bins=4)[1])   # -+ 0.5


def test_description_rows_and_labels():
    st = dbm.TrackStats(5, 1.0, 2.0, -3.0, 4.0, 2.5)
    d = dbm.TrackDescription(st, (0.75, 0.25, 0.5), (3.0, 1.0, 2.0))
    assert list(d.as_dict().items()) == [("count", 5), ("mean", 1.0), ("std", 2.0), ("min", -3.0), ("25%", 1.0), ("50%", 2.0), ("75%", 3.0),
                                         ("max", 4.0)]
    assert d.histogram is None and d.stats.rmse == 2.5
    assert list(dbm.TrackDescription(st, (0.125, 0.9), (0.0, 0.0)).as_dict())[4:6] == ["12.5%", "90%"]
    with pytest.raises(Exception):
        d.stats = st   # frozen
    assert [f.name for f in __import__("dataclasses").fields(dbm.TrackStats)] == ["count", "mean", "std", "min", "max", "rmse"]


def test_argument_refusals_come_before_any_work():
    pts, grid, g = np.zeros((4, 3)), np.zeros((4, 4), np.float32), dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    for bad in ((), tuple(np.linspace(0, 1, 17)), (0.5, 1.5), (-0.1,), (float("nan"),), ((0.5, 0.5),)):
        with pytest.raises(ValueError, match="percentiles"):
            dbm.describe_errors(pts, grid, g, percentiles=bad)
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="bins"):
            dbm.error_histogram(pts, grid, g, bins=bad)
        with pytest.raises(ValueError, match="bins"):
            dbm.describe_errors(pts, grid, g, bins=bad)
    for bad in (2.5, True, "auto", [0.0, 1.0]):
        with pytest.raises(TypeError, match="bins"):
            dbm.error_histogram(pts, grid, g, bins=bad)
    for bad in ((1.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            dbm.error_histogram(pts, grid, g, range=bad)
    with pytest.raises(TypeError, match="map a name"):
        dbm.describe_on_tracks(pts, [(grid, g)])
    with pytest.raises(TypeError, match="GridGeometry"):
        dbm.describe_on_tracks(pts, {"a": (grid, (0.0, 0.0, 1.0, 1.0))})
    with pytest.raises(ValueError, match="z column"):
        dbm.describe_on_tracks(pts[:, :2], {"a": (grid, g)})
    with pytest.raises(ValueError, match="percentiles"):
        dbm.describe_on_tracks(pts, {"a": (grid, g)}, percentiles=(2.0,))
    with pytest.raises(ValueError, match="bins"):
        dbm.describe_on_tracks(pts, {"a": (grid, g)}, bins=0)


def test_header_states_the_rules_and_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    i = text.index("int dbm_track_error_quantiles(")
    doc = text[max(0, i - 4000):i]
    assert re.search(r"deepbedmap\.py:550-563", doc) and re.search(r"deepbedmap\.py:575-608", doc)
    for phrase in ("h = (m - 1) q", "b - d (1 - g)", "g >= 0.5", "-0.0 counts as +0.0", "no float atomics", "radix select", "m = 0: NaN",
                   "e < edges[i]", "i != bins - 1", "Refused (status 1"):
        assert phrase in doc, phrase
    flags = {k: int(v) for k, v in re.findall(r"\b(DBM_TRACK_[A-Z_]+)\s*=\s*(\d+)", text)}
    ev = dbm.evaluation
    assert (flags["DBM_TRACK_MAX_QUANTILES"], flags["DBM_TRACK_MAX_BINS"], flags["DBM_TRACK_DIST_WORKSPACE"]) == (ev.MAX_QUANTILES, ev.MAX_BINS,
                                                                                                                 ev.DIST_WORKSPACE)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Error distribution" in design
    for name in ("TrackDescription", "describe_errors", "error_histogram", "describe_on_tracks"):
        assert hasattr(dbm, name), name


def test_no_gpu_means_loud_failure():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from deepbedmap_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    pts, grid, g = np.zeros((4, 3)), np.zeros((4, 4), np.float32), dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    with pytest.raises(dbm.DbmError):
        dbm.describe_errors(pts, grid, g)
    with pytest.raises(dbm.DbmError):
        dbm.error_histogram(pts, grid, g)
    with pytest.raises(dbm.DbmError):
        dbm.describe_on_tracks(pts, {"a": (grid, g)}, bins=25)
