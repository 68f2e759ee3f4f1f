"""-m gpu: dbm_op_deform_conv2d_backward -- every form of the deformable layers' backward pass at its edges, through the C ABI.

Reference: ops.deform_conv2d_backward(x64, off32, w64, gy64) -- the offsets stay float32, so the oracle forms the sampling coordinates,
their floor and the bilinear weights in float32 (as the reference's elementwise float32 operations do) and every sum in float64.  The
device gets the float32 casts of the same arrays.  Bounds (max-norm relative, the project's own, test_gpu_ops.py): 1e-4 for gx, gw, gb
and 5e-4 for goff.  Without a tolerance: every output finite; goff == 0 wherever the reference's is exactly 0; nothing reaches gx or
gw when every sample lies outside (`all_out`); a repeated call gives the same bits in deterministic mode.

Contracts (include/dbm.h, kernels.h, model.h): gw / gb are ACCUMULATED -- they are prefilled with random values of the gradient's
scale and `result - prefill` is compared; gx / goff are OVERWRITTEN -- they are prefilled with NaN and compared directly.

Offset regimes: see REGIMES.  Near-zero offsets matter most: a freshly initialised offset convolution puts every sample next to an
integer coordinate, where the offset gradient is a one-sided difference whose side the float32 rounding of _offset2grid's normalise /
denormalise round trip decides -- a kernel whose coordinate arithmetic is not the reference's sequence of single float32 operations
passes under normal(0, 1) (3.4e-6) and is off by O(1) there (tests/test_deform_cases_host.py shows it on the CPU).

The kernels under test beside the fused ones live in csrc/deform_sampler.hip.  Its deterministic forms take sixteen channels per
workgroup (launch_deform_backward checks C % 16 == 0; the entry point demands C % 32 == 0): the eight-channel deterministic
instantiations, which no call could reach, are gone.

A mask mutant is NOT among the things these cases can catch: with pad = 1 a clipped coordinate has both of its corners in the zero
padding, so the coordinate-gradient masks never change a value (tests/test_deform_cases_host.py asserts that a non-strict mask gives
the identical goff).  Nobody needs to hunt for a case that tells the masks apart.

Measured on an MI355X (largest over the 154 calls of this module; `device` = HIP against the reference, `float32 oracle` = the
all-float32 NumPy oracle against the same reference):
    output   device     (case)                                    float32 oracle
    gx       3.25e-06   C 64, O 64, (2, 27, 79), converge         4.31e-06
    goff     7.34e-07   C 64, O 64, (1, 1, 1), normal1            4.21e-07
    gw       1.07e-06   C 64, O 1, (2, 27, 79), converge          1.51e-06
    gb       1.29e-06   C 64, O 1, (1, 22, 97), normal1           3.84e-06
The module takes 20 s there (154 device calls, twice as many evaluations of the NumPy oracle).  The `window_edge` regime (added with
tests/test_gpu_deform_forward.py: offsets at the forward's LDS-window limit) brought four more fused rows, none above 4.8e-07.

Found by the bitwise-repeat assertion: past plane 1476 (2133 with C = 64) launch_deform_backward scattered gx with fp32 atomics in
deterministic mode too, so two identical calls differed in gx on (1, 22, 97) and (1, 7, 211).  It now sorts the sampling lists in
global memory there (deform_csr_build_global_kernel) and gathers; the atomic scatter remains for dbm_set_deterministic(0).
"""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUTPUTS = ("gx", "goff", "gw", "gb")
BOUNDS = {"gx": 1e-4, "goff": 5e-4, "gw": 1e-4, "gb": 1e-4}
FUSED_PLANE = 2133   # the last plane the fused backward (CSR input-gradient lists in LDS) takes


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- offset regimes: f(rs, N, H, W) -> float32 (N, 18, H, W); channels 0..8 are x offsets, 9..17 y offsets ----
def _tap_coords(H, W):
    """Image coordinates (x, y) of the undeformed taps: (9, H, W) each (3x3 kernel, pad 1)."""
    t = np.arange(9)
    bx = np.arange(W)[None, None, :] + (t % 3)[:, None, None] - 1 + np.zeros((9, H, W))
    by = np.arange(H)[None, :, None] + (t // 3)[:, None, None] - 1 + np.zeros((9, H, W))
    return bx, by


def _offsets_to(tx, ty, H, W):
    """The offsets that put every sample at image coordinates (tx, ty), each (N, 9, H, W)."""
    bx, by = _tap_coords(H, W)
    return np.concatenate([tx - bx[None], ty - by[None]], axis=1).astype(np.float32)


def regime_zero(rs, N, H, W):
    return np.zeros((N, 18, H, W), np.float32)


def regime_tiny(rs, N, H, W):
    return rs.normal(0, 1e-3, size=(N, 18, H, W)).astype(np.float32)


def regime_lattice(rs, N, H, W):
    """Integers and half-integers from -2 .. 2 (exact on planes with H + 1 and W + 1 powers of two)."""
    return rs.choice(np.arange(-2.0, 2.5, 0.5), size=(N, 18, H, W)).astype(np.float32)


def regime_normal1(rs, N, H, W):
    return rs.normal(0, 1.0, size=(N, 18, H, W)).astype(np.float32)


def regime_border(rs, N, H, W):
    """Every sample in a cell that straddles the image's edge: x in (-1, 0) or (W - 1, W), or y likewise, or both (the cells at the
    image's corners); the other coordinate anywhere inside."""
    def axis(n_pix, on_edge):
        edge = np.where(rs.rand(N, 9, H, W) < 0.5, -1.0, n_pix - 1.0) + rs.uniform(0.05, 0.95, size=(N, 9, H, W))
        inside = rs.uniform(0, n_pix - 1.0, size=(N, 9, H, W))
        return np.where(on_edge, edge, inside)
    ex, ey = rs.rand(N, 9, H, W) < 0.5, rs.rand(N, 9, H, W) < 0.5
    ex = ex | ~ey   # at least one of the two on an edge
    return _offsets_to(axis(W, ex), axis(H, ey), H, W)


def regime_far(rs, N, H, W):
    """normal(0, 6) with a tenth of the taps at +-1e9 and +-3e38: finite, but far outside every plane."""
    off = rs.normal(0, 6.0, size=(N, 18, H, W))
    far = rs.choice([1e9, -1e9, 3e38, -3e38], size=off.shape)
    return np.where(rs.rand(*off.shape) < 0.1, far, off).astype(np.float32)


def regime_all_out(rs, N, H, W):
    return np.full((N, 18, H, W), 1e6, np.float32)


def regime_converge(rs, N, H, W):
    """Every tap of every position within one pixel of ONE input pixel (the centre): that pixel's sampling list holds `plane` entries
    per tap -- the counting sort's largest bin, the longest insertion sort, the longest fixed-order sum."""
    tx = W // 2 + rs.uniform(-0.95, 0.95, size=(N, 9, H, W))
    ty = H // 2 + rs.uniform(-0.95, 0.95, size=(N, 9, H, W))
    return _offsets_to(tx, ty, H, W)


WINDOW_EDGE_VALUES = np.array([-2.0, np.nextafter(np.float32(-2.0), np.float32(-np.inf)), np.nextafter(np.float32(3.0), np.float32(-np.inf)),
                               3.0, -2.5, 3.5], np.float32)


def regime_window_edge(rs, N, H, W):
    """normal(0, 0.5) with a third of the offsets at the limit of the forward's LDS windows: both window kernels keep offsets in
    [-2, 3) and serve the others from memory.  The six values are dealt in turn to randomly chosen entries, the x offsets starting
    with the first and the y offsets with the fourth, so that even a one-pixel plane holds every one of them."""
    off = rs.normal(0, 0.5, size=(N, 18, H, W)).astype(np.float32)
    for axis in (0, 1):
        part = off[:, 9 * axis:9 * axis + 9].reshape(-1)   # (a copy: the slice is not contiguous)
        idx = rs.permutation(part.size)[:(part.size + 2) // 3]
        part[idx] = WINDOW_EDGE_VALUES[(np.arange(idx.size) + 3 * axis) % 6]
        off[:, 9 * axis:9 * axis + 9] = part.reshape(N, 9, H, W)
    return off


REGIMES = {"zero": regime_zero, "tiny": regime_tiny, "lattice": regime_lattice, "normal1": regime_normal1, "border": regime_border,
           "far": regime_far, "all_out": regime_all_out, "converge": regime_converge, "window_edge": regime_window_edge}


def is_exact_plane(H, W):
    """H + 1 and W + 1 powers of two: the division of _offset2grid's normalisation is exact."""
    return ((H + 1) & H) == 0 and ((W + 1) & W) == 0


# ---- cases, references, the comparison (importable without the library: tests/test_deform_cases_host.py) ----
def make_case(C_in, O, shape, regime):
    """x, off, w, gy in float32, seeded by the case itself."""
    N, H, W = shape
    rs = np.random.RandomState(zlib.crc32(repr((C_in, O, shape, regime)).encode()) % 2**31)
    x = rs.normal(size=(N, C_in, H, W)).astype(np.float32)
    off = REGIMES[regime](rs, N, H, W)
    w = (rs.normal(size=(O, C_in, 3, 3)) / np.sqrt(C_in * 9)).astype(np.float32)
    gy = rs.normal(size=(N, O, H, W)).astype(np.float32)
    return x, off, w, gy


def reference(x, off, w, gy):
    """The float64 reference on float32 coordinates."""
    assert off.dtype == np.float32
    with np.errstate(over="ignore"):   # (`far`: a coordinate of 3e38 pixels overflows to inf on its way back from [-1, 1], then clips)
        return dict(zip(OUTPUTS, ops.deform_conv2d_backward(x.astype(np.float64), off, w.astype(np.float64), gy.astype(np.float64))))


def oracle32(x, off, w, gy):
    """The all-float32 oracle: what its own rounding costs against reference()."""
    with np.errstate(over="ignore"):
        return dict(zip(OUTPUTS, ops.deform_conv2d_backward(x, off, w, gy)))


def prefills(ref, seed):
    """Random gw / gb of the reference gradient's scale (what an accumulating kernel must add to)."""
    rs = np.random.RandomState(seed)
    out = []
    for k in ("gw", "gb"):
        scale = float(np.abs(ref[k]).max()) or 1.0
        out.append((rs.normal(size=ref[k].shape) * scale).astype(np.float32))
    return out


def deviations(got, ref, gw0=None, gb0=None):
    """Max-norm relative error per output; gw / gb net of their prefill."""
    pre = {"gw": gw0, "gb": gb0}
    return {k: rel(np.asarray(got[k], np.float64) - (0 if pre.get(k) is None else pre[k].astype(np.float64)), ref[k]) for k in OUTPUTS}


def check(got, ref, gw0=None, gb0=None, regime=None):
    """Asserts every bound and every tolerance-free property; returns the errors per output."""
    errs = deviations(got, ref, gw0, gb0)
    failures = []
    for k in OUTPUTS:
        if not np.isfinite(got[k]).all():
            failures.append(f"{k}: not finite")
        if not errs[k] < BOUNDS[k]:
            failures.append(f"{k}: {errs[k]:.3e} >= {BOUNDS[k]:.0e}")
    stray = np.asarray(got["goff"])[ref["goff"] == 0]
    if not np.all(stray == 0):
        failures.append(f"goff: {np.count_nonzero(stray != 0)} nonzero where the reference is exactly 0")
    if regime == "all_out":
        if not np.all(np.asarray(got["gx"]) == 0):
            failures.append("gx: nonzero although every sample is outside")
        if gw0 is not None and not np.array_equal(np.asarray(got["gw"]), gw0):
            failures.append("gw: changed although every sample is outside")
    assert not failures, (failures, errs)
    return errs


def assert_lattice_is_exact(off, H, W):
    """On an exact plane the reference's float32 coordinates ARE the intended ones (padded frame: image coordinate + 2)."""
    assert is_exact_plane(H, W)
    u, v = ops._deform_geometry(off, H, W, 3, 3, 1, 1)[:2]
    assert u.dtype == np.float32
    bx, by = _tap_coords(H, W)
    N = off.shape[0]
    assert np.array_equal(u.astype(np.float64), (off[:, :9].astype(np.float64) + bx[None] + 2).reshape(N, 9, H * W))
    assert np.array_equal(v.astype(np.float64), (off[:, 9:].astype(np.float64) + by[None] + 2).reshape(N, 9, H * W))


# ---- the device side ----
def load():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


@pytest.fixture(scope="module")
def dbm():
    return load()


def run_device(dbm, case, gw0, gb0, profile=False):
    """One call of the entry point on prefilled outputs: ({gx, goff, gw, gb}, tags of the bracketed deformable launches)."""
    d, _lib, ctx = dbm
    x, off, w, gy = case
    N, C_in, H, W = x.shape
    O = w.shape[0]
    lib = _lib.lib()
    dev = lambda a: d.to_device(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    dx, doff, dw, dgy = dev(x), dev(off), dev(w), dev(gy)
    gx, goff = dev(np.full(x.shape, np.nan, np.float32)), dev(np.full(off.shape, np.nan, np.float32))
    gw, gb = dev(gw0), dev(gb0)
    if profile:
        _lib.check(lib.dbm_profile_begin(ctx.handle), ctx.handle)
    rc = lib.dbm_op_deform_conv2d_backward(ctx.handle, dx.ptr, doff.ptr, dw.ptr, dgy.ptr, gx.ptr, goff.ptr, gw.ptr, gb.ptr, N, C_in, H, W, O)
    tags = [r["tag"] for r in ctx.profile_records() if r["tag"].startswith("deform")] if profile else []
    _lib.check(rc, ctx.handle)
    ctx.synchronize()
    return {"gx": gx.get(), "goff": goff.get(), "gw": gw.get(), "gb": gb.get()}, tags


@functools.lru_cache(maxsize=2)
def prepared(C_in, O, shape, regime):
    """The case, its reference, its prefills and the float32 oracle's own deviation (computed once, shared, not modified)."""
    case = make_case(C_in, O, shape, regime)
    if regime == "lattice":
        assert_lattice_is_exact(case[1], shape[1], shape[2])
    ref = reference(*case)
    gw0, gb0 = prefills(ref, 1 + shape[0])
    dev32 = deviations(oracle32(*case), ref)
    for a in case + (gw0, gb0) + tuple(ref.values()):
        a.setflags(write=False)
    return case, ref, gw0, gb0, dev32


def run_and_check(dbm, C_in, O, shape, regime, repeat, profile=False, label=""):
    case, ref, gw0, gb0, dev32 = prepared(C_in, O, shape, regime)
    got, tags = run_device(dbm, case, gw0, gb0, profile)
    errs = deviations(got, ref, gw0, gb0)
    print("DEFORM_BWD", label, C_in, O, shape, regime, " ".join(f"{k}={errs[k]:.3e}/{dev32[k]:.3e}" for k in OUTPUTS), flush=True)
    check(got, ref, gw0, gb0, regime)
    if repeat:
        again, _ = run_device(dbm, case, gw0, gb0)
        diff = [k for k in OUTPUTS if not np.array_equal(got[k], again[k], equal_nan=True)]
        assert not diff, f"a second identical call differs in {diff}"
    return tags


# N, H, W
FUSED_SHAPES = [
    (1, 1, 1), (1, 1, 7), (2, 7, 1), (1, 3, 5),   # fewer positions than one 64-position tile; planes one pixel wide
    (3, 7, 15),      # exact plane; 315 positions = 4.92 tiles, tiles straddle images
    (1, 31, 63),     # exact plane, 1953 positions, wide rows
    (5, 36, 36),     # the model's plane; 101.25 tiles
    (2, 27, 79),     # plane 2133: the last one the CSR input-gradient kernel takes
    (1, 22, 97),     # plane 2134: the first one on launch_deform_backward
    (13, 36, 36),    # 263.25 tiles > 256 workgroups: eight workgroups of deform_wgrad64_fused_kernel take a second tile, the last tile
                     # holds 16 positions, its fold reads 256 partials; the 64 -> 1 layer's fold reads 264
]


def _fused_cases():
    out = [(s, r) for s in FUSED_SHAPES for r in ("normal1", "tiny")]
    for s in ((3, 7, 15), (5, 36, 36)):
        out += [(s, r) for r in REGIMES if r not in ("normal1", "tiny", "window_edge") and (r != "lattice" or is_exact_plane(*s[1:]))]
    out += [((1, 31, 63), "lattice"), ((1, 1, 7), "lattice"), ((2, 27, 79), "converge"), ((2, 27, 79), "all_out")]
    out += [((3, 7, 15), "window_edge"), ((5, 36, 36), "window_edge")]   # (appended: the rows above keep their ids)
    return [(s, O, r) for s, r in out for O in (64, 1)]


@pytest.mark.parametrize("shape,O,regime", _fused_cases())
def test_fused_forms(dbm, shape, O, regime):
    """C = 64, O in {1, 64}, deterministic mode (the default): the fused kernels of deform_bwd.hip up to plane 2133, the sample-matrix
    forms beyond; which side ran is pinned by the profiler tags of the 64 -> 64 layer's launches."""
    tags = run_and_check(dbm, 64, O, shape, regime, repeat=True, profile=O == 64)
    if O == 64:
        fused = shape[1] * shape[2] <= FUSED_PLANE
        assert any(t.startswith("deform_bwd64_") for t in tags) == fused, tags
        assert any(t.startswith("deform_wgrad64_") for t in tags) == fused, tags


UNFUSED_SHAPES = [(2, 12, 10), (1, 36, 41), (1, 7, 211)]   # 1476: the last plane of the LDS kernels; 1477: the first past them


@pytest.mark.parametrize("C_in,O,shape,regime,det", [(c, o, s, r, det) for c, o in ((32, 1), (32, 32), (64, 32), (96, 64))
                                                     for s in UNFUSED_SHAPES for r in ("normal1", "tiny", "far") for det in (1, 0)])
def test_unfused_forms(dbm, C_in, O, shape, regime, det):
    """C != 64 or O not in {1, 64}: the sample matrix, deform_backward_csr_kernel (<16, 1024, true> with determinism on, <8, 1024, false>
    without); past plane 1476 the lists sorted in global memory (determinism on) or the atomic scatter (off); the GEMV's / the 1x1
    form's weight gradient."""
    d, _lib, ctx = dbm
    from deepbedmap_amd import srgan

    try:
        _lib.check(_lib.lib().dbm_set_deterministic(ctx.handle, det), ctx.handle)
        run_and_check(dbm, C_in, O, shape, regime, repeat=bool(det), label=f"det{det}")
    finally:   # what srgan.apply_config sets, so that later modules see the default
        srgan._applied_deterministic[0] = None
        srgan.apply_config(ctx)


SWITCHED_ENV = {"DBM_DEFORM1_PREMUL_BWD": "0", "DBM_DEFORM_WGRAD_FUSED": "0"}


def switched_forms_main():
    """The child process of test_switched_forms (the switches are read once per process)."""
    dbm = load()
    for shape in ((3, 7, 15), (5, 36, 36)):
        for regime in ("tiny", "border", "normal1"):
            for O in (1, 64):
                tags = run_and_check(dbm, 64, O, shape, regime, repeat=True, profile=O == 64, label="switched")
                if O == 64:   # the input / offset gradients stay fused, the weight gradient comes from the sample matrix
                    assert any(t.startswith("deform_bwd64_") for t in tags) and not any(t.startswith("deform_wgrad64_") for t in tags), tags


def test_switched_forms(dbm):
    """launch_deform_bwd1_fused (DBM_DEFORM1_PREMUL_BWD=0) and the 64 -> 64 layer's weight gradient from the sample matrix
    (DBM_DEFORM_WGRAD_FUSED=0), against the same reference and bounds, in one child process."""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_gpu_deform_backward as t; t.switched_forms_main()"
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **SWITCHED_ENV), capture_output=True, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
