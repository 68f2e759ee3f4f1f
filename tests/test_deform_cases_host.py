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

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import ops  # noqa: E402
from test_gpu_deform_backward import (BOUNDS, OUTPUTS, REGIMES, check, deviations, is_exact_plane, make_case, oracle32,  # noqa: E402
                                      reference)

SHAPES = [(2, 36, 36), (3, 7, 15)]
CASES = [(s, r) for s in SHAPES for r in REGIMES if r != "lattice" or is_exact_plane(*s[1:])]


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
