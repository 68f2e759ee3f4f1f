"""-m gpu: dbm_op_deform_forward_launch -- the deformable layers' forward kernels launched as Generator::forward launches them, in every
offset regime of tests/test_gpu_deform_backward.py (plus `window_edge`), every element compared against its own L1 mass.

What the op-level forward tests of test_gpu_ops.py do not reach: offsets on a pixel, between two, across the image's edge, at +-1e9 and
+-3e38, all outside, all on one pixel, at the LDS windows' limit; the offsets' 32-channel buffer (offsn = 32 * plane, channels 18..31
belong to the offset convolution's padding: they hold NaN here); act = 1 on the fp32 64 -> 64 kernels; the channels-last twin yt (beside
y and alone), the retained sample matrix colout (the only way to deform_conv64_fused_kernel on a narrow plane) and the retained
premultiplied planes z; both sides of the fp32 window form's width threshold.

Reference: ops.deform_conv2d(x64, off32, w64, b64) -- coordinates, floor and one-dimensional weights in float32 (as the reference's
elementwise float32 operations form them: reference() of the backward module), every sum in float64; with act, LeakyReLU 0.2 on the
float64 value.  The sample matrix is the oracle's own (return_cache); z is the float64 contraction sum_c w[o, c, t] x[c], laid out
(n, o * 9 + t, p) as deform1_sample_kernel reads it (its header comment; deform1_premul_kernel's: z[(n * nz + k) * plane + p]).

Comparison: EVERY element of every output.  y / yt against deform_conv2d(|x|, off, |w|, |b|) (the bilinear weights are >= 0: the sum
of the absolute terms), colout against the sample of |x|, z against sum |w||x|.  An element without mass must equal the reference
exactly (`rel_mass`); where no sample of a case has mass (`all_out`, and `far` on the one-pixel plane) y is exactly bias, resp. the
float32 lrelu(bias), in every form, split-bf16 included.  Every
output finite in every regime.

Tolerances, none taken from the kernels:
  fp32 forms (y, yt, colout, z): the rule of test_gpu_conv_launches.py -- 16 x the worst deviation of the all-float32 oracle from the
    float64 reference over the whole table in the same normalisation, floor 8 * 2^-24, cap 1e-4, computed at run time (`tolerances`;
    tests/test_deform_cases_host.py asserts that 16 x the oracle's figure stays under the cap, so the cap never lets a case pass).
  split-bf16 forms 2 / 3 / 4: deform_conv64_x3_kernel blends in fp32, splits the blended SAMPLE and (pack_deform_x3_kernel) the WEIGHT
    as hi = bf16(v), lo = bf16(v - hi) and accumulates hi*lo + lo*hi + hi*hi in fp32 (three v_mfma_f32_32x32x16_bf16 per k step, small
    terms first): confirmed in the kernel.  Each operand keeps 16 significand bits: the dropped lo*lo is <= 2^-16 of the term, the two
    representation errors add <= 2 * 2^-17; together 2^-15 of the element's mass, plus the fp32 tolerance of y for the blend and the
    accumulation.

Bitwise: yt is y transposed; yt from a call with y == nullptr is yt from a call with both; form 3 == form 4; the fp32 window kernel
(no colout) == the fp32 gathering kernel (colout), as launch_deform_conv_fused's comment promises; offsn = 32 * plane with NaN in
channels 18..31 == offsn = 18 * plane; a second identical call == the first.  Every output buffer has 64 floats of NaN behind it and
is prefilled with NaN: the guard keeps its bits, the buffer is overwritten everywhere.  Outputs that are not requested are not
allocated (a row with colout and without yt: the kernel copes with the null).

Which kernel ran is asserted on every launch: the entry point's report names the path (fused 64 -> 64 launcher, premultiplied,
gather-then-multiply, split-bf16 launcher, sampler + GEMV, sampler + implicit GEMM), the profiler's tag the launcher's choice
(deform64w_ / deform64_..._keep / deform64x3w_ / deform64x3_); the table states the expectation per plane (FP32_PLANES' second column),
tests/test_deform_cases_host.py restates it from launch_deform_conv_fused's formula and DWF_MAXPIX.

Out of scope: deform1_premul_mfma_kernel starts at 2^18 positions (launch_premul) and keeps test_deform1_premultiplication_on_the_
matrix_pipes (test_gpu_ops.py).

No case failed on the kernels as they were: this module found no bug, and the two "same bits" promises (fp32 window == gathering,
form 3 == form 4) hold in every regime, `far` and `window_edge` included.

Nothing of the table is thinned: the 64 -> O rows run every O in {1, 2, 3, 16} and form 6 runs O in {1, 64} under every regime on
every one of their planes, the three lattice planes included (the references of a (plane, regime) pair are shared, a row costs its
launches only).

Figures of the run on an MI355X (gfx950) that accompanied this file, worst |d| / mass over the table's 320 rows (1 813 launches; 322
tests with test_refused_combinations and the figures' printer); the tolerances are computed at run time, these are theirs:
  output            float32 oracle's worst   tolerance    kernels' worst   (case)
  y, yt  fp32            1.91e-07            3.06e-06       3.31e-07       64 -> 64, (1, 22, 97), zero, launch (c): gathering + colout
  y, yt  split-bf16      1.91e-07            3.36e-05       2.98e-06       (1, 5, 3), far, form 3, act 0   (2^-15 = 3.05e-05 + y's fp32 tolerance)
  colout                 2.48e-07            3.96e-06       2.34e-07       64 -> 64, (3, 36, 36), tiny, launch (b)
  z                      3.95e-07            6.31e-06       1.07e-07       64 -> 3, (3, 36, 36), normal1, form 1
yt has no figure of its own: it is y's bits, asserted.  The worst fp32 figure is 1.7 x the float32 oracle's own; the split-bf16 forms
use a tenth of their derived bound.  The module takes 9 s there (2.9 s of them the first row's: it loads the library and evaluates the
float32 oracle over the whole table for the tolerances); no row takes more than 0.1 s.

Mutations tried on a scratch copy -- on an earlier state of the table: 238 rows, 91 of them fp32 64 -> 64, before (1, 30, 9) joined it
and with the 64 -> O rows at O = 1 plus one of {2, 3, 16} per pair --, the rows of this module that failed, and test_gpu_ops.py's
deformable tests (`-k deform`, 26):
  1. deform_conv64_fusedw_kernel stages one window row too few (the last row stays zero; the `near` test unchanged -- the mismatch a
     `<=` in the test would make, without reading past the LDS allocation): fp32 (3, 36, 36) under border, converge, far, normal1 and
     window_edge (0.05 .. 0.19 of the mass).  test_gpu_ops.py: 3 of 26 failed too.  (3, 36, 36) was then the table's only window
     plane with more rows than a tile's window -- on the others the window's last row lies below the image anyway -- so (1, 30, 9)
     was added: it fails the mutant under border, far and window_edge.
  2. `act` ignored in deform_conv64_fused_kernel: 90 of the 91 fp32 rows (every one but (1, 5, 3) all_out, whose exact answer is 0) --
     launch (b)'s bits against launch (a)'s on window planes, launch (a)'s tolerance on gathering planes.  test_gpu_ops.py: all passed.
  3. the offsets' image stride hard-wired to 18 * plane in launch_deform_conv_fused: every fp32 and few-channel row on a plane with
     N >= 2 but the all_out ones (45 rows; 0.2 .. 0.33 of the mass, 242 x the mass under far).  test_gpu_ops.py: all passed.
  4. yt written from the pre-activation value in deform_conv64_fused_kernel: the same 90 rows ("yt is not y transposed" on gathering
     planes, launch (b)'s yt against launch (a)'s on window planes).  test_gpu_ops.py: all passed.
  5. deform_conv64_x3_kernel drops the lo * hi product: 37 of the 43 split-bf16 rows (form 3 == form 4, the first assertion to meet
     it; the six others have no mass: all_out, and far on one pixel).  test_gpu_ops.py: 14 of 26 failed too.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import ops
from test_gpu_conv_launches import TOL_CAP, TOL_FLOOR, bits, rel_mass, tolerance   # noqa: F401  (TOL_*: the host module's)
from test_gpu_deform_backward import REGIMES, _offsets_to, assert_lattice_is_exact, is_exact_plane   # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats of NaN behind every output buffer
SLOPE32 = np.float32(0.2)
X3_SPLIT = 2.0 ** -15            # module docstring: lo*lo dropped (2^-16) + two representation errors (2 * 2^-17)
QUANTITIES = ("y", "colout", "z")

# ---- the table ----
# 64 -> 64 fp32: (N, H, W), the kernel a launch WITHOUT colout reaches ("w": deform_conv64_fusedw_kernel, "g": deform_conv64_fused_kernel;
# with colout it is always the latter), why
FP32_PLANES = [
    ((1, 1, 1), "w", "one pixel"),
    ((1, 5, 3), "w", "fewer positions than one 64-position tile; no bias"),
    ((2, 7, 9), "w", "126 positions: two images, each less than one 128-position window tile"),
    ((1, 6, 37), "w", "H >= 5: the last window width, 12 x 44 = 528 window pixels"),
    ((1, 6, 38), "g", "H >= 5: the first gathering width"),
    ((1, 1, 59), "w", "H = 1: the last window width, 8 x 66 = 528"),
    ((1, 1, 60), "g", "H = 1: the first gathering width"),
    ((1, 2, 51), "w", "H = 2: the last window width, 9 x 58 = 522"),
    ((1, 2, 52), "g", "H = 2: the first gathering width, 9 x 59 = 531"),
    ((3, 36, 36), "w", "the model's plane: 60.75 gathering tiles, 11 window tiles per image, the last one ragged"),
    ((1, 22, 97), "g", "a wide ragged gathering plane"),
    ((1, 30, 9), "w", "beyond the issue's table: a second window plane whose tiles' last window rows lie inside the image (mutation 1)"),
]
LATTICE_PLANES = [((1, 7, 15), "w"), ((2, 31, 31), "w"), ((1, 3, 63), "g")]   # H + 1 and W + 1 powers of two (`lattice` only)
X3_PLANES = [
    ((1, 1, 1), "one pixel"),
    ((1, 5, 3), "less than a tile; no bias"),
    ((1, 16, 16), "exactly one 16 x 16 window tile"),
    ((1, 17, 33), "one row and one column past a tile edge"),
    ((2, 37, 21), "ragged over two images"),
]
FEW_PLANES = [(1, 1, 1), (2, 7, 9), (3, 36, 36), (1, 22, 97)]   # 256-position blocks of deform1_sample_kernel ragged and across images
FEW_O = (1, 2, 3, 16)            # blockIdx.y = co; 16: the dynamic-LDS limit of deform1_premul_kernel
UNFUSED_PLANES = [(2, 7, 9), (1, 22, 97)]
NON_LATTICE = [r for r in REGIMES if r != "lattice"]


def _pairs(planes):
    return [(p, r) for p in planes for r in NON_LATTICE]


FP32_CASES = _pairs([p for p, _, _ in FP32_PLANES]) + [(p, "lattice") for p, _ in LATTICE_PLANES]
X3_CASES = _pairs([p for p, _ in X3_PLANES]) + [(p, "lattice") for p, _ in LATTICE_PLANES]


# every O under every (plane, regime): nothing is thinned (the references of a pair are shared, a row costs its launches only)
FEW_CASES = [(o, p, r) for p, r in _pairs(FEW_PLANES) + [(p, "lattice") for p, _ in LATTICE_PLANES] for o in FEW_O]
UNFUSED_CASES = [(o, p, r) for p, r in _pairs(UNFUSED_PLANES) + [(p, "lattice") for p, _ in LATTICE_PLANES] for o in (1, 64)]
ALL_CASES = sorted(set([(64, p, r) for p, r in FP32_CASES + X3_CASES] + FEW_CASES + UNFUSED_CASES), key=repr)


def fp32_kernel_without_colout(plane):
    return dict([(p, k) for p, k, _ in FP32_PLANES] + LATTICE_PLANES)[plane]


# ---- cases and references (importable without the library: tests/test_deform_cases_host.py) ----
# The oracle's sample matrix is 576 float64 rows per position and does not depend on the weights: a (plane, regime) pair has ONE x and
# ONE set of offsets, and the weights of all its layers (O = 64, 1, 2, 3, 16) are stacked into one 86-channel tensor, so that one call of
# ops.deform_conv2d serves every row on that pair.  Output channels are independent: a layer's reference is its slice.
O_SLICES = {64: slice(0, 64), 1: slice(64, 65), 2: slice(65, 67), 3: slice(67, 70), 16: slice(70, 86)}
O_ALL = 86


def make_inputs(plane, regime):
    """x, off (N, 18, H, W), the stacked w (86, 64, 3, 3) and bias (None on the (1, 5, 3) plane) in float32, seeded by the pair itself"""
    N, H, W = plane
    rs = np.random.RandomState(zlib.crc32(repr(("fwd", plane, regime)).encode()) % 2**31)
    x = rs.normal(size=(N, 64, H, W)).astype(np.float32)
    off = REGIMES[regime](rs, N, H, W)
    w = (rs.normal(size=(O_ALL, 64, 3, 3)) / 24.0).astype(np.float32)
    b = None if plane == (1, 5, 3) else rs.normal(size=O_ALL).astype(np.float32)
    return x, off, w, b


def lrelu(v):
    return np.where(v >= 0, v, v.dtype.type(0.2) * v)


def _cols(colm, N, P):
    """the oracle's sample matrix (N * P, 576) in the kernels' layout (N, 576, P), row c * 9 + t"""
    return np.ascontiguousarray(colm.reshape(N, P, 576).transpose(0, 2, 1))


def _premul(x, w):
    """z (N, O, 9, P) = sum_c w[o, c, t] x[n, c, p] in the operands' type"""
    N, _, H, W = x.shape
    wt = np.ascontiguousarray(w.reshape(w.shape[0], 64, 9).transpose(0, 2, 1)).reshape(-1, 64)   # row o * 9 + t
    return np.matmul(wt[None], x.reshape(N, 64, H * W)).reshape(N, w.shape[0], 9, H * W)


def evaluate(plane, regime, with32):
    """Inputs of a (plane, regime) pair, the float64 references and L1 masses of every output, and (with32) the all-float32 oracle's
    deviations in the same normalisation, per layer"""
    x, off, w, b = make_inputs(plane, regime)
    N, H, W = plane
    if regime == "lattice":
        assert_lattice_is_exact(off, H, W)
    d = np.float64
    few = slice(64, O_ALL)
    absb = None if b is None else np.abs(b).astype(d)
    with np.errstate(over="ignore"):   # (`far`: a coordinate of 3e38 pixels overflows to inf on its way back from [-1, 1], then clips)
        y, (colm,) = ops.deform_conv2d(x.astype(d), off, w.astype(d), None if b is None else b.astype(d), return_cache=True)
        ym, (colmm,) = ops.deform_conv2d(np.abs(x).astype(d), off, np.abs(w).astype(d), absb, return_cache=True)
    out = dict(x=x, off=off, w=w, b=b, y=y, y_mass=ym, col=_cols(colm, N, H * W), col_mass=_cols(colmm, N, H * W),
               z=_premul(x.astype(d), w[few].astype(d)), z_mass=_premul(np.abs(x).astype(d), np.abs(w[few]).astype(d)))
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    out["sample_mass_max"] = float(out["col_mass"].max())
    if with32:
        with np.errstate(over="ignore"):
            y32, (colm32,) = ops.deform_conv2d(x, off, w, b, return_cache=True)
        assert y32.dtype == np.float32 and colm32.dtype == np.float32
        z32 = _premul(x, w[few]).astype(d)
        dev = {"colout": rel_mass(_cols(colm32, N, H * W).astype(d) - out["col"], out["col_mass"])}
        for O, sl in O_SLICES.items():
            dev["y", O] = max(rel_mass(y32[:, sl].astype(d) - y[:, sl], ym[:, sl]), rel_mass(lrelu(y32[:, sl]).astype(d) - lrelu(y[:, sl]), ym[:, sl]))
            if O <= 16:
                zs = slice(sl.start - 64, sl.stop - 64)
                dev["z", O] = rel_mass(z32[:, zs] - out["z"][:, zs], out["z_mass"][:, zs])
        out["dev32"] = dev
    return out


@functools.lru_cache(maxsize=None)
def figures(plane, regime):
    """the scalars of a pair: the float32 oracle's deviations per layer and the largest sample mass"""
    e = evaluate(plane, regime, True)
    return dict(e["dev32"], sample_mass_max=e["sample_mass_max"])


@functools.lru_cache(maxsize=2)
def _pair(plane, regime):
    """(computed once for the run of consecutive rows on the pair, shared, not modified; the 576-row matrices are not kept for the
    whole module: ROWS is ordered by pair)"""
    return evaluate(plane, regime, False)


def case(O, plane, regime):
    """one layer of a pair: its inputs, references and masses ({y, colout, z}), the float32 oracle's figures"""
    e, sl, N, P = _pair(plane, regime), O_SLICES[O], plane[0], plane[1] * plane[2]
    f = figures(plane, regime)
    ref, mass = {"y": e["y"][:, sl], "colout": e["col"]}, {"y": e["y_mass"][:, sl], "colout": e["col_mass"]}
    dev32 = {"y": f["y", O], "colout": f["colout"]}
    if O <= 16:
        zs = slice(sl.start - 64, sl.stop - 64)
        ref["z"], mass["z"], dev32["z"] = e["z"][:, zs].reshape(N, O * 9, P), e["z_mass"][:, zs].reshape(N, O * 9, P), f["z", O]
    return dict(x=e["x"], off=e["off"], w=np.ascontiguousarray(e["w"][sl]), b=None if e["b"] is None else np.ascontiguousarray(e["b"][sl]),
                ref=ref, mass=mass, dev32=dev32, O=O, plane=plane, regime=regime, no_sample_mass=f["sample_mass_max"] == 0)


@functools.lru_cache(maxsize=None)
def oracle32_worst():
    """{y, colout, z}: the all-float32 oracle's worst |d| / mass over the whole table (y with and without LeakyReLU)"""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for O, plane, regime in ALL_CASES:
        f = figures(plane, regime)
        worst["y"] = max(worst["y"], f["y", O])
        worst["colout"] = max(worst["colout"], f["colout"])
        if O <= 16:
            worst["z"] = max(worst["z"], f["z", O])
    return worst


@functools.lru_cache(maxsize=None)
def tolerances():
    t = {q: tolerance(v) for q, v in oracle32_worst().items()}
    t["x3"] = X3_SPLIT + t["y"]
    return t


# ---- the device side ----
@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


WORST = {}   # quantity -> (figure, what produced it): printed by the module's last test


def _note(q, err, what):
    if err > WORST.get(q, (-1.0, None))[0]:
        WORST[q] = (err, what)


def launch(dbm, c, form, act=0, want=("y",), wide=False):
    """One call on fresh buffers.  want: the outputs requested (the others are NULL); wide: the offsets in a 32-channel buffer whose
    channels 18..31 hold NaN.  Checks the guards and that every requested output was overwritten everywhere; returns
    ({name: array}, the path by its name in _lib.DEFORM_PATHS, deformable profiler tags)."""
    d, _lib, ctx = dbm
    N, H, W = c["plane"]
    O, P = c["O"], c["plane"][1] * c["plane"][2]
    off = c["off"]
    if wide:
        off = np.concatenate([off, np.full((N, 14, H, W), np.nan, np.float32)], axis=1)
    shapes = {"y": (N, O, H, W), "yt": (N * P, 64), "colout": (N, 576, P), "z": (N, O * 9, P)}
    a = _lib.DeformLaunch()
    a.form, a.N, a.H, a.W, a.O, a.act = form, N, H, W, O, act
    keep = [d.to_device(v) for v in (c["x"], off, c["w"])]
    a.x, a.off, a.w = (k.ptr for k in keep)
    a.offsn = off.shape[1] * P
    if c["b"] is not None:
        keep.append(d.to_device(c["b"]))
        a.bias = keep[-1].ptr
    out = {}
    for name in want:
        n = int(np.prod(shapes[name]))
        out[name] = d.to_device(np.full(n + GUARD, np.nan, np.float32))
        setattr(a, name, out[name].ptr)
    report = (C.c_int * 1)(-1)
    lib = _lib.lib()
    _lib.check(lib.dbm_profile_begin(ctx.handle), ctx.handle)
    rc = lib.dbm_op_deform_forward_launch(ctx.handle, C.byref(a), report)
    tags = [r["tag"] for r in ctx.profile_records() if r["tag"].startswith("deform")]
    _lib.check(rc, ctx.handle)
    ctx.synchronize()
    got = {}
    for name in want:
        flat = out[name].get().reshape(-1)
        n = flat.size - GUARD
        assert np.array_equal(bits(flat[n:]), bits(np.full(GUARD, np.nan, np.float32))), f"form {form}: wrote behind {name}"
        assert np.isfinite(flat[:n]).all(), f"form {form}: {name} holds {np.count_nonzero(~np.isfinite(flat[:n]))} non-finite values (NaN prefill?)"
        got[name] = flat[:n].reshape(shapes[name])
    return got, _lib.DEFORM_PATHS.get(report[0], report[0]), tags


def nhwc(y):
    return np.ascontiguousarray(y.transpose(0, 2, 3, 1)).reshape(-1, y.shape[1])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def check_y(c, y, act, tol, what, q="y"):
    """every element of y (N, O, H, W) against the float64 reference and its own mass; where no sample has mass: exactly the bias"""
    ref = lrelu(c["ref"]["y"]) if act else c["ref"]["y"]
    err = rel_mass(y.astype(np.float64) - ref, c["mass"]["y"])
    _note(q, err, what)
    print(f"DEFORM_FWD {what}: {q} {err:.3e} (float32 oracle {c['dev32']['y']:.3e}, tolerance {tol:.3e})", flush=True)
    assert err <= tol, (what, err, tol)
    if c["no_sample_mass"]:   # (`all_out`; `far` on the one-pixel plane, whose nine taps all miss it)
        b = np.zeros(c["O"], np.float32) if c["b"] is None else c["b"]
        want = (np.where(b >= 0, b, SLOPE32 * b) if act else b).astype(np.float32)
        assert same(y, np.broadcast_to(want[None, :, None, None], y.shape)), f"{what}: y is not exactly the bias although every sample is outside"


def check_q(c, q, got, tol, what):
    err = rel_mass(got.astype(np.float64) - c["ref"][q], c["mass"][q])
    _note(q, err, what)
    print(f"DEFORM_FWD {what}: {q} {err:.3e} (float32 oracle {c['dev32'][q]:.3e}, tolerance {tol:.3e})", flush=True)
    assert err <= tol, (what, q, err, tol)


def kernel_of(tags):
    """the one deformable launch of a call, by its tag: "w" / "g" (fp32 window / gathering), "g+keep", "x3w", "x3g", or the tag itself"""
    assert len(tags) == 1, tags
    t = tags[0]
    for prefix, name in (("deform64x3w_", "x3w"), ("deform64x3_", "x3g"), ("deform64w_", "w"), ("deform64_", "g")):
        if t.startswith(prefix):
            return name + ("+keep" if t.endswith("_keep") else "")
    return t


def row_fp32_64_to_64(dbm, O, plane, regime):
    """form 0, O = 64: deform_conv64_fusedw_kernel / deform_conv64_fused_kernel, with and without colout, act 0 / 1, yt beside y, alone, absent"""
    c, tol = case(O, plane, regime), tolerances()   # (O = 64 on every row of this kind)
    what = f"fp32 64->64 {plane} {regime}"
    plain = fp32_kernel_without_colout(plane)
    # (a) the generator's inference launch: 32-channel offsets, act, y and its twin
    a, path, tags = launch(dbm, c, 0, act=1, want=("y", "yt"), wide=True)
    assert (path, kernel_of(tags)) == ("fused64", plain), (path, tags)
    check_y(c, a["y"], 1, tol["y"], what + " (a)")
    assert same(a["yt"], nhwc(a["y"])), "yt is not y transposed"
    # (b) the retained pass of the unfused weight gradient: the same with the sample matrix -> the gathering kernel
    b, path, tags = launch(dbm, c, 0, act=1, want=("y", "yt", "colout"), wide=True)
    assert (path, kernel_of(tags)) == ("fused64", "g+keep"), (path, tags)
    check_q(c, "colout", b["colout"], tol["colout"], what + " (b)")
    assert not b["colout"][c["mass"]["colout"] == 0].any(), "a sample whose four corners lie in the padding is not exactly 0"
    assert same(b["y"], a["y"]) and same(b["yt"], a["yt"]), f"kernel {plain} and the gathering kernel differ in bits"
    # (c) colout without yt, act 0, 18-channel offsets
    cc, path, tags = launch(dbm, c, 0, act=0, want=("y", "colout"))
    assert (path, kernel_of(tags)) == ("fused64", "g+keep"), (path, tags)
    check_y(c, cc["y"], 0, tol["y"], what + " (c)")
    assert same(cc["colout"], b["colout"]), "colout differs between offsn = 18 * plane and 32 * plane / act 0 and 1"
    # (d) the twin alone (y == nullptr), 18-channel offsets
    dd, path, tags = launch(dbm, c, 0, act=1, want=("yt",))
    assert (path, kernel_of(tags)) == ("fused64", plain), (path, tags)
    assert same(dd["yt"], a["yt"]), "yt from a call with y == nullptr (offsn = 18 * plane) differs from yt beside y (offsn = 32 * plane, NaN in 18..31)"
    # (d') the same through the gathering kernel's sample-matrix path: colout and yt, no y
    dk, path, tags = launch(dbm, c, 0, act=1, want=("yt", "colout"))
    assert (path, kernel_of(tags)) == ("fused64", "g+keep"), (path, tags)
    assert same(dk["yt"], a["yt"]) and same(dk["colout"], b["colout"]), "the gathering kernel with colout and yt but y == nullptr gives other bits"
    # (e) y alone, act 0, 32-channel offsets: against (c), whose offsets are 18-channel and whose kernel gathers
    e, path, tags = launch(dbm, c, 0, act=0, want=("y",), wide=True)
    assert (path, kernel_of(tags)) == ("fused64", plain), (path, tags)
    assert same(e["y"], cc["y"]), f"kernel {plain} at offsn = 32 * plane (NaN in 18..31) differs from the gathering kernel at 18 * plane"
    # a second identical call
    again, _, _ = launch(dbm, c, 0, act=1, want=("y", "yt"), wide=True)
    assert same(again["y"], a["y"]) and same(again["yt"], a["yt"]), "a second identical call gives other bits"


def row_split_bf16_64_to_64(dbm, O, plane, regime):
    """forms 3 (deform_conv64_x3w_kernel) and 4 (deform_conv64_x3_kernel), y / yt / both, act 0 / 1; form 2 takes the gathering kernel here"""
    c, tol = case(O, plane, regime), tolerances()   # (O = 64 on every row of this kind)
    what = f"split-bf16 {plane} {regime}"
    w3, path, tags = launch(dbm, c, 3, act=1, want=("y", "yt"), wide=True)
    assert (path, kernel_of(tags)) == ("x3", "x3w"), (path, tags)
    check_y(c, w3["y"], 1, tol["x3"], what + " form 3", q="y x3")
    assert same(w3["yt"], nhwc(w3["y"])), "form 3: yt is not y transposed"
    g4, path, tags = launch(dbm, c, 4, act=1, want=("y", "yt"))
    assert (path, kernel_of(tags)) == ("x3", "x3g"), (path, tags)
    check_y(c, g4["y"], 1, tol["x3"], what + " form 4", q="y x3")
    assert same(g4["yt"], nhwc(g4["y"])), "form 4: yt is not y transposed"
    assert same(g4["y"], w3["y"]), "form 3 (offsn = 32 * plane, NaN in 18..31) and form 4 (18 * plane) differ in bits"
    for form, kern in ((3, "x3w"), (4, "x3g")):
        t, path, tags = launch(dbm, c, form, act=1, want=("yt",), wide=form == 4)
        assert (path, kernel_of(tags)) == ("x3", kern), (path, tags)
        assert same(t["yt"], w3["yt"]), f"form {form}: yt from a call with y == nullptr differs"
    y0 = {}
    for form, kern in ((3, "x3w"), (4, "x3g"), (2, "x3g")):
        y0[form], path, tags = launch(dbm, c, form, act=0, want=("y",))
        assert (path, kernel_of(tags)) == ("x3", kern), (path, tags)
    check_y(c, y0[3]["y"], 0, tol["x3"], what + " form 3 act 0", q="y x3")
    assert same(y0[4]["y"], y0[3]["y"]) and same(y0[2]["y"], y0[3]["y"]), "forms 2 / 3 / 4 differ in bits (act 0)"
    again, _, _ = launch(dbm, c, 3, act=1, want=("y", "yt"), wide=True)
    assert same(again["y"], w3["y"]) and same(again["yt"], w3["yt"]), "a second identical call gives other bits"


def row_few_output_channels(dbm, O, plane, regime):
    """O <= 16: form 1 (deform1_premul_kernel + deform1_sample_kernel, z returned), form 5 (deform_conv1_fused_kernel), form 0 (the layer's
    own choice: the premultiplied form, on the caller's z or on a scratch)"""
    c, tol = case(O, plane, regime), tolerances()
    what = f"64->{O} {plane} {regime}"
    p, path, tags = launch(dbm, c, 1, want=("y", "z"), wide=True)
    assert path == "premul" and tags == [f"deform{O}_{plane[1]}x{plane[2]}_n{plane[0]}"], (path, tags)
    check_y(c, p["y"], 0, tol["y"], what + " form 1")
    check_q(c, "z", p["z"], tol["z"], what + " form 1")
    g, path, tags = launch(dbm, c, 5, want=("y",))
    assert path == "gather1" and len(tags) == 1, (path, tags)
    check_y(c, g["y"], 0, tol["y"], what + " form 5")
    own, path, _ = launch(dbm, c, 0, want=("y", "z"))
    assert path == "premul", path
    assert same(own["y"], p["y"]) and same(own["z"], p["z"]), "form 0 (offsn = 18 * plane) and form 1 (32 * plane, NaN in 18..31) differ in bits"
    own2, path, _ = launch(dbm, c, 0, want=("y",), wide=True)
    assert path == "premul" and same(own2["y"], p["y"]), "form 0 on a scratch z differs"
    g2, _, _ = launch(dbm, c, 5, want=("y",), wide=True)
    assert same(g2["y"], g["y"]), "form 5: offsn = 32 * plane (NaN in 18..31) differs from 18 * plane"


def row_unfused_sampler_path(dbm, O, plane, regime):
    """form 6: deform_sample_kernel + gemv_cols_kernel (O = 1) / the implicit GEMM over the sample matrix (O = 64, with LeakyReLU)"""
    c, tol = case(O, plane, regime), tolerances()
    what = f"unfused 64->{O} {plane} {regime}"
    act = int(O == 64)
    u, path, _ = launch(dbm, c, 6, act=act, want=("y", "colout"), wide=True)
    assert path == ("sampler+igemm" if O == 64 else "sampler+gemv"), path
    check_y(c, u["y"], act, tol["y"], what)
    if O == 64:
        check_q(c, "colout", u["colout"], tol["colout"], what)
    else:   # (the case of an O <= 16 row keeps no sample-matrix tolerance of its own: the 64 -> 64 table's)
        err = rel_mass(u["colout"].astype(np.float64) - c["ref"]["colout"], c["mass"]["colout"])
        _note("colout", err, what)
        assert err <= tol["colout"], (what, err)
    v, path, _ = launch(dbm, c, 6, act=act, want=("y",))
    assert same(v["y"], u["y"]), "the sample matrix as a scratch / offsn = 18 * plane gives other bits"


# One test per row; the rows of a (plane, regime) pair follow each other, so that the pair's references are computed once.
ROW_KINDS = {"fp32": row_fp32_64_to_64, "x3": row_split_bf16_64_to_64, "few": row_few_output_channels, "unfused": row_unfused_sampler_path}
ROWS = sorted([("fp32", 64, p, r) for p, r in FP32_CASES] + [("x3", 64, p, r) for p, r in X3_CASES] + [("few",) + k for k in FEW_CASES] +
              [("unfused",) + k for k in UNFUSED_CASES], key=lambda k: (k[2], k[3], k[0], k[1]))


@pytest.mark.parametrize("kind,O,plane,regime", ROWS, ids=["%s-%d-%dx%dx%d-%s" % ((k, o) + p + (r,)) for k, o, p, r in ROWS])
def test_row(dbm, kind, O, plane, regime):
    ROW_KINDS[kind](dbm, O, plane, regime)


def test_refused_combinations(dbm):
    """what the launchers do not support is refused, by name"""
    d, _lib, ctx = dbm
    c1, c64 = case(1, (1, 1, 1), "zero"), case(64, (1, 1, 1), "zero")
    for c, form, act, want in ((c1, 1, 1, ("y",)), (c1, 5, 0, ("y", "z")), (c1, 0, 0, ("y", "yt")), (c1, 0, 0, ("y", "colout")),
                               (c64, 3, 0, ("y", "colout")), (c64, 0, 0, ("y", "z")), (c64, 0, 0, ()), (c64, 1, 0, ("y",)), (c1, 3, 0, ("y",)),
                               (c64, 6, 0, ("y", "yt")), (c1, 6, 1, ("y",)), (c64, 7, 0, ("y",))):
        with pytest.raises(_lib.DbmError, match="dbm_op_deform_forward_launch"):
            launch(dbm, c, form, act=act, want=want)


def test_zz_measured_figures():
    """(last: prints what the module measured -- the table of the docstring)"""
    t, w32 = tolerances(), oracle32_worst()
    for q in ("y", "y x3", "colout", "z"):
        if q in WORST:
            base = "y" if q.startswith("y") else q
            print(f"DEFORM_FWD_WORST {q}: float32 oracle {w32[base]:.3e}  tolerance {t['x3' if q == 'y x3' else base]:.3e}  kernels {WORST[q][0]:.3e}  ({WORST[q][1]})")
