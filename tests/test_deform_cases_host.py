"""No GPU: the cases and the comparison of tests/test_gpu_deform_backward.py can tell a wrong deformable backward from a right one.

The offset regimes, the reference and check() are the GPU module's own.  Here the all-float32 oracle must pass them in every regime,
and two mutated restatements -- built from the oracle's source text -- must be rejected:
  (a) sampling coordinates computed in float64: near-zero offsets put every sample next to an integer coordinate, and the float32
      rounding of the normalise / denormalise round trip decides on which side.  goff is off by O(1) of its largest value under `zero`
      and `tiny` on the 36 x 36 plane, and by a few 1e-6 under normal(0, 1) -- which is why the latter regime alone proves nothing;
  (b) border corners replicated instead of zero: rejected under `border`.

NOT expected to fail: a mask mutant.  With pad = 1 a clipped coordinate has both of its corners in the zero padding (the sampler's own
ring and the convolution's padding), so the coordinate-gradient masks multiply values that are zero already: a non-strict mask gives
the identical goff in every regime.  Asserted below, so that nobody hunts for a case that tells the masks apart.
"""
import inspect
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import ops  # noqa: E402
from test_gpu_deform_backward import (BOUNDS, OUTPUTS, REGIMES, check, deviations, is_exact_plane, make_case, oracle32,  # noqa: E402
                                      reference)

SHAPES = [(2, 36, 36), (3, 7, 15)]
CASES = [(s, r) for s in SHAPES for r in REGIMES if r != "window_edge" and (r != "lattice" or is_exact_plane(*s[1:]))]
CASES += [(s, "window_edge") for s in SHAPES]   # (appended: the cases above keep their ids)


def _mutant(edits):
    """deform_conv2d_backward restated with `edits` = [(function name, old text, new text)] applied to the oracle's source."""
    ns = dict(vars(ops))
    for fn in ("_deform_geometry", "deform_conv2d_backward"):
        src = inspect.getsource(getattr(ops, fn))
        for name, old, new in edits:
            if name == fn:
                assert src.count(old) == 1, (fn, old)
                src = src.replace(old, new)
        exec(compile(src, f"<mutant of {fn}>", "exec"), ns)

    def run(*a):
        with np.errstate(over="ignore"):   # (`far`, as in reference())
            return dict(zip(OUTPUTS, ns["deform_conv2d_backward"](*a)))
    return run


FLOAT64_COORDS = _mutant([("_deform_geometry", "f = offset.dtype.type", "f = np.float64; offset = offset.astype(np.float64)")])
REPLICATED_BORDER = _mutant([("deform_conv2d_backward", "xpp = np.pad(x, ((0, 0), (0, 0), (pad + 1, pad + 1), (pad + 1, pad + 1)))",
                              "xpp = np.pad(x, ((0, 0), (0, 0), (pad + 1, pad + 1), (pad + 1, pad + 1)), mode='edge')")])
NON_STRICT_MASKS = _mutant([("deform_conv2d_backward", "gu = gu * ((u > 0) & (u < Wp + 1))", "gu = gu * ((u >= 0) & (u <= Wp + 1))"),
                            ("deform_conv2d_backward", "gv = gv * ((v > 0) & (v < Hp + 1))", "gv = gv * ((v >= 0) & (v <= Hp + 1))")])


@pytest.fixture(scope="module")
def evaluated():
    """case and reference per (shape, regime): computed once, shared, not modified."""
    out = {}
    for shape, regime in CASES:
        case = make_case(64, 64, shape, regime)
        ref = reference(*case)
        for a in case + tuple(ref.values()):
            a.setflags(write=False)
        out[shape, regime] = case, ref
    return out


@pytest.mark.parametrize("shape,regime", CASES)
def test_float32_oracle_passes_every_regime(evaluated, shape, regime):
    case, ref = evaluated[shape, regime]
    check(oracle32(*case), ref, regime=regime)


@pytest.mark.parametrize("shape,regime", CASES)
def test_mask_mutant_is_not_expected_to_fail(evaluated, shape, regime):
    case, ref = evaluated[shape, regime]
    x, off, w, gy = case
    got = NON_STRICT_MASKS(x.astype(np.float64), off, w.astype(np.float64), gy.astype(np.float64))
    assert np.array_equal(got["goff"], ref["goff"])


@pytest.mark.parametrize("regime", ["zero", "tiny"])
def test_float64_coordinates_are_rejected_near_zero_offsets(evaluated, regime):
    case, ref = evaluated[(2, 36, 36), regime]
    x, off, w, gy = case
    got = FLOAT64_COORDS(x.astype(np.float64), off, w.astype(np.float64), gy.astype(np.float64))
    errs = deviations(got, ref)
    assert errs["goff"] > 0.1, errs   # O(1) of goff's largest value: a tenth of the samples take the other side's one-sided difference
    with pytest.raises(AssertionError, match="goff"):
        check(got, ref, regime=regime)


def test_float64_coordinates_pass_under_normal1(evaluated):
    """(the regime the suite used before: it cannot see the coordinate arithmetic)"""
    case, ref = evaluated[(2, 36, 36), "normal1"]
    x, off, w, gy = case
    check(FLOAT64_COORDS(x.astype(np.float64), off, w.astype(np.float64), gy.astype(np.float64)), ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_replicated_border_is_rejected(evaluated, shape):
    case, ref = evaluated[shape, "border"]
    x, off, w, gy = case
    got = REPLICATED_BORDER(x.astype(np.float64), off, w.astype(np.float64), gy.astype(np.float64))
    errs = deviations(got, ref)
    assert errs["goff"] >= BOUNDS["goff"] and errs["gw"] >= BOUNDS["gw"], errs
    with pytest.raises(AssertionError):
        check(got, ref, regime="border")


def _corners_inside(off, H, W):
    """How many of its four corners each sample has inside the image: (N, 9, H * W)."""
    with np.errstate(over="ignore"):
        u0, v0 = ops._deform_geometry(off, H, W, 3, 3, 1, 1)[4:6]
    inside = 0
    for dv in (0, 1):
        for du in (0, 1):
            yy, xx = v0 + dv - 2, u0 + du - 2
            inside = inside + ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W))
    return inside


@pytest.mark.parametrize("shape", SHAPES)
def test_regimes_put_the_samples_where_they_say(evaluated, shape):
    N, H, W = shape
    inside = _corners_inside(evaluated[shape, "border"][0][1], H, W)
    assert set(np.unique(inside)) == {1, 2}   # every cell straddles an edge (two corners in the padding) or both (three: a corner cell)
    assert _corners_inside(evaluated[shape, "all_out"][0][1], H, W).max() == 0
    u0, v0 = ops._deform_geometry(evaluated[shape, "converge"][0][1], H, W, 3, 3, 1, 1)[4:6]
    assert set(np.unique(u0 - 2)) <= {W // 2 - 1, W // 2} and set(np.unique(v0 - 2)) <= {H // 2 - 1, H // 2}
    far = _corners_inside(evaluated[shape, "far"][0][1], H, W)
    assert (far == 0).mean() > 0.1 and (far == 4).any()
    # near-zero offsets: a good part of the float32 coordinates is NOT the integer it would be in exact arithmetic
    if (H, W) == (36, 36):
        u = ops._deform_geometry(evaluated[shape, "zero"][0][1], H, W, 3, 3, 1, 1)[0]
        assert 0.05 < (u != np.round(u)).mean() < 0.5 and (u < np.round(u)).mean() > 0.03


# ---- the forward table (tests/test_gpu_deform_forward.py): its cases and tolerances, without a GPU ----
import re  # noqa: E402

import test_gpu_deform_forward as fwd  # noqa: E402

ROOT = os.path.dirname(HERE)
FWD_PLANES = sorted(set(k[1] for k in fwd.ALL_CASES))


def test_window_edge_straddles_both_window_limits_on_every_plane():
    """offsets in [-2, 3) stay inside the LDS windows: each plane of the forward table has offsets at -2 and just below it, just below 3
    and at it -- on both axes wherever an axis has room for the six values (N * H * W >= 2)"""
    lo, hi = np.float32(-2.0), np.float32(3.0)
    for plane in FWD_PLANES:
        off = REGIMES["window_edge"](np.random.RandomState(zlib.crc32(repr(plane).encode()) % 2**31), *plane)
        assert off.dtype == np.float32 and off.shape == (plane[0], 18, plane[1], plane[2])
        axes = [off] if plane[0] * plane[1] * plane[2] < 2 else [off[:, :9], off[:, 9:]]
        for o in axes:
            assert (o == lo).any() and (o == np.nextafter(lo, np.float32(-np.inf))).any() and (o < lo - 0.25).any(), plane
            assert (o == hi).any() and (o == np.nextafter(hi, np.float32(-np.inf))).any() and (o > hi + 0.25).any(), plane
            assert ((o > lo) & (o < hi)).mean() > 0.6, plane
    for key in fwd.ALL_CASES:   # ... and so do the offsets the table's cases really use
        if key[2] == "window_edge":
            o = fwd.make_inputs(*key[1:])[1]
            assert (o < lo).any() and (o == lo).any() and (o >= hi).any() and (o == np.nextafter(hi, np.float32(-np.inf))).any(), key


def test_only_all_out_has_no_mass_and_the_float32_oracle_sets_the_forward_tolerances():
    """`all_out`: every sample of every case has zero mass; every other regime leaves mass in every case's output (but `far` on one pixel).  16 x the float32
    oracle's worst per-element deviation over the forward table lies above the floor and under the 1e-4 cap for every fp32 quantity:
    the cap is never what lets a case pass."""
    for key in fwd.ALL_CASES:
        m = fwd.figures(*key[1:])["sample_mass_max"]
        # (the one exception, asserted: the nine normal(0, 6) taps of `far` around the ONE pixel of (1, 1, 1) all miss it -- the GPU
        #  module then holds y to the bias exactly, as under all_out: its exact check is keyed on the mass, not on the regime's name)
        assert (m == 0) == (key[2] == "all_out" or key[1:] == ((1, 1, 1), "far")), (key, m)
    worst, tol = fwd.oracle32_worst(), fwd.tolerances()
    for q in fwd.QUANTITIES:
        print(f"forward table, {q}: float32 oracle's worst |d| / mass {worst[q]:.3e}, x 16 = {16 * worst[q]:.3e}, tolerance {tol[q]:.3e}")
        assert fwd.TOL_FLOOR < 16 * worst[q] < fwd.TOL_CAP, (q, worst[q])
        assert tol[q] == 16 * worst[q]
    assert tol["x3"] == 2.0 ** -15 + tol["y"]


def _window_form_constants():
    src = open(os.path.join(ROOT, "deepbedmap_amd", "csrc", "deform_window.h")).read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("DWF_R", "DWF_POS", "DWF_MAXPIX")}


def fp32_window_ok(H, W, R, POS, MAXPIX):
    """launch_deform_conv_fused: (span_rows + 2 R + 3) * (W + 2 R + 3) <= DWF_MAXPIX, span_rows = min(H, (POS - 1 + W - 1) / W + 1)"""
    span_rows = min(H, (POS - 1 + W - 1) // W + 1)
    return (span_rows + 2 * R + 3) * (W + 2 * R + 3) <= MAXPIX


def test_forward_table_sits_on_both_sides_of_the_window_threshold():
    k = _window_form_constants()
    assert k == {"DWF_R": 2, "DWF_POS": 128, "DWF_MAXPIX": 528}, k
    ok = lambda H, W: fp32_window_ok(H, W, k["DWF_R"], k["DWF_POS"], k["DWF_MAXPIX"])   # noqa: E731
    for H, last in ((6, 37), (36, 37), (5, 37), (1, 59), (2, 51)):
        assert ok(H, last) and not ok(H, last + 1), (H, last)
        assert all(ok(H, w) for w in range(1, last + 1)) and not any(ok(H, w) for w in range(last + 1, 200)), H
    planes = dict([(p, kern) for p, kern, _ in fwd.FP32_PLANES] + fwd.LATTICE_PLANES)
    for (N, H, W), kern in planes.items():
        assert kern == ("w" if ok(H, W) else "g"), (N, H, W)
    for edge in ((1, 6, 37), (1, 6, 38), (1, 1, 59), (1, 1, 60), (1, 2, 51), (1, 2, 52)):
        assert edge in planes, edge
