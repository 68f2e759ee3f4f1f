"""-m gpu: the head of the generator at op level against the float64 NumPy oracle -- DeepbedmapInputBlock in its three forward forms
(input_block.hip, and layer by layer through misc.hip / igemm.hip), its weight gradients as Generator::backward runs them, the
few-channel weight-gradient kernels in both forms (misc.hip) and the backward of the nearest x2 resize (sumpool2_kernel).

dbm_op_input_block / dbm_op_input_block_backward run the generator's own launch sequences (generator.hip: input_block_form,
input_block_forward, input_block_rebuild_cols, input_block_queue_wgrads, input_block_small_wgrads); dbm_op_smallcin_wgrad is
launch_smallcin_conv_wgrad with or without the scratch buffer the discriminator hands it; dbm_op_sumpool2 is launch_sumpool2.  Every
row of the tables below names the form it is meant to reach and asserts what the op reports: a threshold that moves takes a row's
coverage away loudly.

What is compared.  EVERY element against its own float64 L1 mass (the manner of test_gpu_conv_launches.py): an output element
against conv(|x|, |w|) + |b| of its branch, a gW / gb entry against sum |dy * x| / sum |dy| plus the magnitude of the prefill it adds
onto.  The reference is oracle.ops.conv2d / conv2d_backward on float64 copies, branch by branch.  Memory a launch must not touch --
the gap between images when ysn > 128 * plane, y when yt is asked for, 256 floats before and after every output -- is prefilled with
NaN and compared bitwise.  Gradients are prefilled with random values of each entry's own scale; the net of the prefill is compared.

Tolerance, not taken from the kernels: per quantity (y, gW, gb) 16 x the worst deviation of the FLOAT32 oracle from the float64 one
over this file's own tables in the same normalisation, floor 8 * 2^-24, cap 1e-4; computed at run time (`tolerances`).

Inputs at two magnitudes: "unit" (U[0, 1) tiles, what the smoke run feeds) and "metres" (the sweep's: X in +-2000, W1 in -100..4000,
W2 in -10..1000, W3 in 0..500).  Weights are N(0, 1) / sqrt(K), biases are nonzero (0.5 .. 1.5, either sign).

The slices of smallcin_wgrad_partial_kernel: a launch is cut into 64 slices of ceil(T / 64) positions.  The partial form runs only
for T >= 16384 positions, i.e. T = 64 q + r with q >= 256: the last slice then holds q + r - 63 > 0 positions (r > 0), never none --
a slice past the end cannot occur above the threshold.  The rows "s-disc", "s-w1" and "s-ragged" have short last slices (216, 195
and 246 positions against 264, 257 and 263).

Figures of the run on an MI355X (gfx950) that accompanied this file; the tolerances are computed at run time, these are theirs:
  quantity   float32 oracle's worst   tolerance   kernels' worst
  y               2.28e-07            3.65e-06       2.3e-07
  gW              2.46e-07            3.93e-06       4.4e-07   (1.9e-07 in deterministic mode)
  gb              1.52e-07            2.43e-06       2.6e-07   (7.7e-08 in deterministic mode)
Kernels' worst |d| / mass per form, both magnitudes:
  forward   fused (form 1) 2.3e-07    rows (form 2) 2.1e-07, yt = y transposed bit for bit    layer-wise (form 0) 2.2e-07
            layer-wise against rows on (3, 66): 2.0e-07
  backward  (gW / gb; deterministic | atomics; category, K slices of both wide branches)
            b-11-n1 1.9e-07 / 3.8e-08 | the same, cat 0, S 1       b-11-n3 8.2e-08 / 3.8e-08 | 8.5e-08 / 5.3e-08, cat 0, S 3
            b-11-n64 3.3e-08 / 3.0e-08 | 4.4e-07 / 2.6e-07, cat 0, S 32 | 64
            b-3x3-n2 1.3e-07 / 7.7e-08 | the same, cat 0, S 1      b-14x19-n2 7.1e-08 / 2.7e-08 | 1.0e-07 / 8.0e-08, cat 0, S 4
            b-20x72-n1 5.9e-08 / 2.4e-08 | 1.0e-07 / 6.3e-08, cat 9, S 5        b-11-n3-wide 8.2e-08 / 3.8e-08 | 8.3e-08 / 4.7e-08, cat 0, S 3
  few-channel weight gradients   per element (form 0) 7.9e-08 / 2.6e-08    partial + fold (form 1) 2.6e-08 / 2.0e-08
  sumpool2_kernel   every plane bit for bit, with and without mask
No kernel was found wrong.  The module takes 3 s there (95 cases; the slowest, 0.6 s, is the first one, which loads the library and
computes the references of every table).
Mutations of input_block.hip tried on scratch builds, the forward table and the NaN-pixel cases run against each:
  the tenth tap's B index unclamped (`k1 = 2 * s + 1`)      no value changes (its A operand is zero): every row of the table passes;
                                                            test_a_nan_pixel_reaches_only_its_receptive_field fails for "fused" and
                                                            "rows" (64 / 96 outputs NaN outside the pixel's windows)
  the tenth tap's A operand unmasked (`av[s] = wt[k]`)      26 rows fail: every fused and rows row
  the yt channel offset `4 * g + 16 * hh`                   10 rows fail: every rows row that asks for yt
  the last of the six W1 partial tiles dropped              26 rows fail: every fused and rows row
  the rows kernel's `col < avail` zeroing removed           nothing fails, and nothing can: the columns it clears lie past the last
      column any STORED position reads (position p < OW - ox0 reads W1 columns up to 10 p + 29 < avail1, likewise W2, X, W3), and a
      position that is not stored reads position 0's window (`pv`); MFMA columns are independent, so no output depends on them.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ops

pytestmark = pytest.mark.gpu

TOL_CAP = 1e-4            # the project's criterion for every dbm_op_* contraction (tests/test_gpu_ops.py)
EPS24 = 2.0 ** -24
TOL_FLOOR = 8 * EPS24
MARGIN = 16.0
PAD = 256                 # guard floats on either side of a device tensor (a multiple of 4: the tensor stays 16-byte aligned)
LAYERWISE, FUSED, ROWS = 0, 1, 2
MAGS = ("unit", "metres")

# conv_on_X, conv_on_W1, conv_on_W2, conv_on_W3: (input channels, kernel, stride, input plane in units of the tile)
BRANCH = ((1, 3, 1, 1), (1, 30, 10, 10), (2, 6, 2, 2), (1, 3, 1, 1))
IN_NAMES = ("x", "w1", "w2", "w3")
RANGES = {"unit": ((0, 1), (0, 1), (0, 1), (0, 1)), "metres": ((-2000, 2000), (-100, 4000), (-10, 1000), (0, 500))}


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Guarded:
    """`n` float32 values on the device, `offset` floats past a 16-byte boundary, PAD floats of NaN on either side; `get` checks them."""

    def __init__(self, d, host, offset=0):
        host = np.ascontiguousarray(host, dtype=np.float32)
        self.shape, self.n, self.lead = host.shape, host.size, PAD + offset
        self.arr = d.to_device(self._padded(host))
        self.ptr = C.c_void_p(self.arr.ptr + 4 * self.lead)

    def _padded(self, host):
        buf = np.full(self.lead + self.n + PAD, np.nan, np.float32)
        buf[self.lead:self.lead + self.n] = host.ravel()
        return buf

    def set(self, host):
        self.arr.set(self._padded(np.ascontiguousarray(host, dtype=np.float32)))

    def get(self):
        full = self.arr.get()
        guard = np.concatenate([full[:self.lead], full[self.lead + self.n:]])
        assert same_bytes(guard, np.full(guard.size, np.nan, np.float32)), "floats beside the tensor were overwritten"
        return full[self.lead:self.lead + self.n].reshape(self.shape).copy()


def tolerance_of(worst):
    return min(TOL_CAP, max(TOL_FLOOR, MARGIN * worst))


def worst_rel(dev, mass, what):
    """max |dev| / mass over every element; an element without mass must not deviate at all"""
    dev, mass = np.abs(np.asarray(dev, np.float64)), np.asarray(mass, np.float64)
    assert np.all(np.isfinite(dev)), f"{what}: not finite"
    assert np.all(dev[mass == 0] == 0), f"{what}: an element without mass deviates"
    return float((dev / np.where(mass > 0, mass, 1.0)).max())


# ------------------------------------------------------------------------------------------------------------------------
# the input block: data, references
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_data(N, H, W, mag):
    """float32 inputs, weights and biases of one case with the float64 forward reference, its L1 mass and the float32 oracle's
    deviation; shared by every test that needs them (never modified)."""
    rs = np.random.RandomState([N, H, W, MAGS.index(mag)])
    out = {"case": (N, H, W, mag)}
    ys, masses, y32 = [], [], []
    for i, (cin, k, stride, scale) in enumerate(BRANCH):
        lo, hi = RANGES[mag][i]
        x = rs.uniform(lo, hi, (N, cin, scale * H, scale * W)).astype(np.float32)
        w = (rs.normal(size=(32, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
        b = (rs.uniform(0.5, 1.5, 32) * rs.choice([-1.0, 1.0], 32)).astype(np.float32)
        for a in (x, w, b):
            a.setflags(write=False)
        out[IN_NAMES[i]], out["k" + str(i)], out["b" + str(i)] = x, w, b
        x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
        ys.append(ops.conv2d(x64, w64, b64, stride=stride))
        masses.append(ops.conv2d(np.abs(x64), np.abs(w64), np.abs(b64), stride=stride))
        y32.append(ops.conv2d(x, w, b, stride=stride))
    out["y"], out["mass"] = np.concatenate(ys, axis=1), np.concatenate(masses, axis=1)
    assert out["y"].shape == (N, 128, H - 2, W - 2)
    out["oracle32"] = worst_rel(np.concatenate(y32, axis=1).astype(np.float64) - out["y"], out["mass"], "float32 oracle")
    return out


@functools.lru_cache(maxsize=None)
def grad_data(N, H, W, mag):
    """The incoming gradient g (N, 128, plane) of one case, per branch the float64 gW / gb with their L1 masses, the float32 oracle's
    deviations and the prefills (random, of each entry's own scale)."""
    dd = block_data(N, H, W, mag)
    rs = np.random.RandomState([N, H, W, MAGS.index(mag), 7])
    g = rs.normal(size=(N, 128, H - 2, W - 2)).astype(np.float32)
    g.setflags(write=False)
    out = {"g": g, "branches": [], "oracle32": {"gW": 0.0, "gb": 0.0}}
    for i, (cin, k, stride, scale) in enumerate(BRANCH):
        x, w = dd[IN_NAMES[i]], dd["k" + str(i)]
        gi = g[:, 32 * i:32 * i + 32]
        _, gW, gb = ops.conv2d_backward(x.astype(np.float64), w.astype(np.float64), gi.astype(np.float64), stride=stride, need_gx=False)
        _, mW, mb = ops.conv2d_backward(np.abs(x.astype(np.float64)), w.astype(np.float64), np.abs(gi.astype(np.float64)), stride=stride,
                                        need_gx=False)
        _, gW32, gb32 = ops.conv2d_backward(x, w, gi, stride=stride, need_gx=False)
        out["oracle32"]["gW"] = max(out["oracle32"]["gW"], worst_rel(gW32.astype(np.float64) - gW, mW, "float32 oracle gW"))
        out["oracle32"]["gb"] = max(out["oracle32"]["gb"], worst_rel(gb32.astype(np.float64) - gb, mb, "float32 oracle gb"))
        gW0 = (rs.uniform(-1, 1, gW.shape) * np.where(mW > 0, mW, 1.0)).astype(np.float32)
        gb0 = (rs.uniform(-1, 1, gb.shape) * np.where(mb > 0, mb, 1.0)).astype(np.float32)
        for a in (gW0, gb0):
            a.setflags(write=False)
        out["branches"].append({"gW": gW, "gb": gb, "mW": mW, "mb": mb, "gW0": gW0, "gb0": gb0})
    return out


# ------------------------------------------------------------------------------------------------------------------------
# forward: the table
# ------------------------------------------------------------------------------------------------------------------------
# id: (N, H, W, form asked for, form that must run, options).  Options: "ysn" extra floats between images; "off" the input that sits
# one float past a 16-byte boundary; "yt" run again for the channels-last output; "twice" the launch must repeat bit for bit.
FWD_ROWS = {
    # the fused kernel, 11 x 11
    "f-n1": (1, 11, 11, FUSED, FUSED, {"twice": 1}),
    "f-n2": (2, 11, 11, -1, FUSED, {"twice": 1}),
    "f-n5": (5, 11, 11, FUSED, FUSED, {"twice": 1}),
    "f-ysn": (2, 11, 11, -1, FUSED, {"ysn": 40, "twice": 1}),
    "f-w1off": (2, 11, 11, -1, LAYERWISE, {"off": "w1"}),      # in_al16: a 4-byte-aligned view takes the layer-wise path
    "f-w2off": (2, 11, 11, -1, LAYERWISE, {"off": "w2"}),
    # the rows kernel, with y and again with yt
    "r-3x66": (1, 3, 66, ROWS, ROWS, {"yt": 1, "twice": 1}),        # one output row, exactly two tiles
    "r-4x67": (2, 4, 67, ROWS, ROWS, {"yt": 1, "twice": 1}),        # odd width: scalar staging; last tile of one position; image strides
    "r-5x68": (1, 5, 68, ROWS, ROWS, {"yt": 1, "twice": 1}),        # 16-byte staging, last tile of two
    "r-3x97": (1, 3, 97, ROWS, ROWS, {"yt": 1, "twice": 1}),        # last tile of 31
    "r-5x68-off": (1, 5, 68, ROWS, ROWS, {"yt": 1, "twice": 1, "off": "w1"}),   # scalar staging behind an even width
    "r-4x67-ysn": (2, 4, 67, ROWS, ROWS, {"ysn": 12, "twice": 1}),
    # eligibility edges under the model's own choice
    "e-3x65": (1, 3, 65, -1, LAYERWISE, {}),
    "e-3x66": (1, 3, 66, -1, ROWS, {"twice": 1}),
    "e-11x11": (1, 11, 11, -1, FUSED, {"twice": 1}),
    "e-11x12": (1, 11, 12, -1, LAYERWISE, {}),
    # layer by layer
    "l-3x3": (2, 3, 3, LAYERWISE, LAYERWISE, {}),                  # a 1 x 1 plane
    "l-3x12": (2, 3, 12, LAYERWISE, LAYERWISE, {}),
    "l-14x19": (2, 14, 19, LAYERWISE, LAYERWISE, {"ysn": 4}),
    "l-11x11": (2, 11, 11, LAYERWISE, LAYERWISE, {}),
    "l-3x66": (1, 3, 66, LAYERWISE, LAYERWISE, {"against": ROWS}),
}
FWD_RUNS = [(rid, mag) for rid in FWD_ROWS for mag in MAGS]

# id: (N, H, W, channels of the buffer g lives in)
BWD_ROWS = {
    "b-11-n1": (1, 11, 11, 128),
    "b-11-n3": (3, 11, 11, 128),
    "b-11-n64": (64, 11, 11, 128),      # 5184 positions: the wide branches' launch splits K
    "b-3x3-n2": (2, 3, 3, 128),         # planes one pixel wide
    "b-14x19-n2": (2, 14, 19, 128),
    "b-20x72-n1": (1, 20, 72, 128),     # a 1260-position plane: the 1x1 GEMM category with 900 channels
    "b-11-n3-wide": (3, 11, 11, 160),   # g inside a wider buffer, NaN in the channels past 128
}
BWD_RUNS = [(rid, mag, det) for rid in BWD_ROWS for mag in MAGS for det in (1, 0)]


def expected_wgrad_cat(plane, gsn):
    """choose_form (wgrad_plan.h) for the wide branches' 1x1 view: the 1x1 GEMM on large contiguous planes, else the workgroup form"""
    return 9 if plane >= 256 and plane % 4 == 0 and gsn % 4 == 0 else 0


@functools.lru_cache(maxsize=None)
def tolerances():
    """16 x the float32 oracle's worst deviation over the tables of this file, per quantity; floor 8 * 2^-24, cap 1e-4"""
    worst = {"y": 0.0, "gW": 0.0, "gb": 0.0}
    for N, H, W, _, _, _ in FWD_ROWS.values():
        for mag in MAGS:
            worst["y"] = max(worst["y"], block_data(N, H, W, mag)["oracle32"])
    for N, H, W, _ in BWD_ROWS.values():
        for mag in MAGS:
            o = grad_data(N, H, W, mag)["oracle32"]
            worst["gW"], worst["gb"] = max(worst["gW"], o["gW"]), max(worst["gb"], o["gb"])
    for row in SC_ROWS:
        o = sc_data(row)["oracle32"]
        worst["gW"], worst["gb"] = max(worst["gW"], o["gW"]), max(worst["gb"], o["gb"])
    return {k: tolerance_of(v) for k, v in worst.items()}, worst


def run_forward(dbm, dd, form, want_yt=False, ysn_extra=0, off=None):
    """One dbm_op_input_block call on NaN-filled, guarded outputs -> (y (N, 128, h, w), yt (N * plane, 128) or None, form_out).
    Checks what the launch must leave alone."""
    d, _lib, ctx = dbm
    N, H, W, _ = dd["case"]
    plane = (H - 2) * (W - 2)
    ysn = 128 * plane + ysn_extra
    ins = [Guarded(d, dd[n], offset=1 if off == n else 0) for n in IN_NAMES]
    wb = [Guarded(d, dd[k + str(i)]) for i in range(4) for k in ("k", "b")]
    y = Guarded(d, np.full((N, ysn), np.nan, np.float32))
    yt = Guarded(d, np.full((N * plane, 128), np.nan, np.float32)) if want_yt else None
    f = C.c_int(-99)
    ctx.call("dbm_op_input_block", *[t.ptr for t in ins], *[t.ptr for t in wb], y.ptr, ysn, yt.ptr if yt else None, N, H, W, form, C.byref(f))
    for t, n in zip(ins, IN_NAMES):
        assert same_bytes(t.get(), dd[n]), n
    yh = y.get()
    if want_yt:
        assert same_bytes(yh, np.full((N, ysn), np.nan, np.float32)), "y was written although yt was asked for"
        return None, yt.get(), f.value
    assert same_bytes(yh[:, 128 * plane:], np.full((N, ysn_extra), np.nan, np.float32)), "the gap between images was written"
    return yh[:, :128 * plane].reshape(N, 128, H - 2, W - 2), None, f.value


def forward_error(y, dd):
    return worst_rel(y.astype(np.float64) - dd["y"], dd["mass"], "y")


@pytest.mark.parametrize("rid,mag", FWD_RUNS, ids=[f"{r}-{m}" for r, m in FWD_RUNS])
def test_input_block_forward(dbm, rid, mag):
    N, H, W, form, want, opt = FWD_ROWS[rid]
    dd = block_data(N, H, W, mag)
    tol = tolerances()[0]["y"]
    kw = {"ysn_extra": opt.get("ysn", 0), "off": opt.get("off")}
    y, _, f = run_forward(dbm, dd, form, **kw)
    err = forward_error(y, dd)
    line = f"FWD {rid:11s} {mag:6s} N {N} {H}x{W} form {f} y {err:.3e} (tol {tol:.3e})"
    assert f == want, (rid, "form_out", f, "expected", want)
    if opt.get("twice"):
        y2, _, f2 = run_forward(dbm, dd, form, **kw)
        assert f2 == f and same_bytes(y, y2), "two launches on the same inputs differ"
    if opt.get("yt"):
        _, yt, ft = run_forward(dbm, dd, form, want_yt=True, **kw)
        assert ft == ROWS
        assert same_bytes(yt.reshape(N, (H - 2) * (W - 2), 128).transpose(0, 2, 1), y.reshape(N, 128, -1)), "yt is not y transposed, bit for bit"
        _, yt2, _ = run_forward(dbm, dd, form, want_yt=True, **kw)
        assert same_bytes(yt, yt2), "two channels-last launches on the same inputs differ"
    if "against" in opt:
        y2, _, f2 = run_forward(dbm, dd, opt["against"])
        assert f2 == opt["against"]
        gap = worst_rel(y.astype(np.float64) - y2.astype(np.float64), dd["mass"], "form against form")
        line += f" against form {f2} {gap:.3e}"
        assert gap <= 2 * tol, (gap, tol)
    print(line)
    assert err <= tol, (rid, mag, err, tol)


def test_input_block_forms_are_refused_where_they_cannot_run(dbm):
    d, _lib, ctx = dbm
    for (N, H, W), form, kw, match in [((2, 11, 11), FUSED, {"off": "w1"}, "16-byte"), ((2, 11, 11), FUSED, {"off": "w2"}, "16-byte"),
                                       ((1, 11, 12), FUSED, {}, "11 x 11"), ((1, 3, 65), ROWS, {}, "two tiles"),
                                       ((1, 11, 11), FUSED, {"want_yt": True}, "yt"), ((1, 3, 66), LAYERWISE, {"want_yt": True}, "yt"),
                                       ((1, 11, 11), -1, {"want_yt": True}, "yt")]:
        with pytest.raises(_lib.DbmError, match=match):
            run_forward(dbm, block_data(N, H, W, "unit"), form, **kw)


# One NaN pixel per input: (row, column) in x, w1, w2 (channel 1), w3
NAN_CASES = {
    "fused": (1, 11, 11, FUSED, ((4, 4), (47, 63), (9, 13), (6, 7))),
    "layerwise": (1, 11, 11, LAYERWISE, ((4, 4), (47, 63), (9, 13), (6, 7))),
    "rows": (1, 4, 67, ROWS, ((1, 40), (17, 333), (3, 70), (1, 20))),
}


@pytest.mark.parametrize("name", list(NAN_CASES))
def test_a_nan_pixel_reaches_only_its_receptive_field(dbm, name):
    """An output element is NaN exactly where the float64 reference is: the MFMA forms multiply padding taps (the tenth of the 3x3
    branches) and padding columns by zero, and 0 * NaN is NaN -- what such a term reads must lie inside the element's own window."""
    N, H, W, form, pixels = NAN_CASES[name]
    dd = dict(block_data(N, H, W, "unit"))
    ys, masses = [], []
    for i, (cin, k, stride, scale) in enumerate(BRANCH):
        x = dd[IN_NAMES[i]].copy()
        x[0, cin - 1, pixels[i][0], pixels[i][1]] = np.nan
        dd[IN_NAMES[i]] = x
        w64, b64 = dd["k" + str(i)].astype(np.float64), dd["b" + str(i)].astype(np.float64)
        ys.append(ops.conv2d(x.astype(np.float64), w64, b64, stride=stride))
        masses.append(ops.conv2d(np.abs(x.astype(np.float64)), np.abs(w64), np.abs(b64), stride=stride))
    ref, mass = np.concatenate(ys, axis=1), np.concatenate(masses, axis=1)
    y, _, f = run_forward(dbm, dd, form)
    assert f == form
    hit = np.isnan(ref)
    assert hit.any() and not hit.all() and all(np.isnan(r).any() for r in ys)
    assert np.array_equal(np.isnan(y), hit), ("NaN elements", int(np.isnan(y).sum()), "reference", int(hit.sum()),
                                              np.argwhere(np.isnan(y) != hit)[:4].tolist())
    err = worst_rel(np.where(hit, 0.0, y.astype(np.float64) - ref), np.where(hit, 1.0, mass), "y")
    assert err <= tolerances()[0]["y"], err


# ------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------
def run_backward(dbm, dd, gd, gch):
    """dbm_op_input_block_backward from the prefills -> (eight raw gradient arrays, categories, K slices)"""
    d, _lib, ctx = dbm
    N, H, W, _ = dd["case"]
    plane = (H - 2) * (W - 2)
    gbuf = np.full((N, gch, H - 2, W - 2), np.nan, np.float32)
    gbuf[:, :128] = gd["g"]
    ins = [Guarded(d, dd[n]) for n in IN_NAMES]
    g = Guarded(d, gbuf)
    grads = [Guarded(d, b[k]) for b in gd["branches"] for k in ("gW0", "gb0")]
    cat, S = (C.c_int * 2)(-99, -99), (C.c_int * 2)(-99, -99)
    ctx.call("dbm_op_input_block_backward", *[t.ptr for t in ins], g.ptr, gch * plane, *[t.ptr for t in grads], N, H, W, cat, S)
    for t, n in zip(ins, IN_NAMES):
        assert same_bytes(t.get(), dd[n]), n
    assert same_bytes(g.get(), gbuf), "g"
    return [t.get() for t in grads], list(cat), list(S)


def backward_errors(raw, gd):
    eW = eb = 0.0
    for i, b in enumerate(gd["branches"]):
        eW = max(eW, worst_rel(raw[2 * i].astype(np.float64) - b["gW0"] - b["gW"], b["mW"] + np.abs(b["gW0"]), f"gW of branch {i}"))
        eb = max(eb, worst_rel(raw[2 * i + 1].astype(np.float64) - b["gb0"] - b["gb"], b["mb"] + np.abs(b["gb0"]), f"gb of branch {i}"))
    return eW, eb


def restore_deterministic(ctx):
    from deepbedmap_amd import srgan

    srgan._applied_deterministic[0] = None   # what srgan.apply_config sets, so that later modules see the default
    srgan.apply_config(ctx)


@pytest.mark.parametrize("rid,mag,det", BWD_RUNS, ids=[f"{r}-{m}-det{t}" for r, m, t in BWD_RUNS])
def test_input_block_backward(dbm, rid, mag, det):
    d, _lib, ctx = dbm
    N, H, W, gch = BWD_ROWS[rid]
    dd, gd = block_data(N, H, W, mag), grad_data(N, H, W, mag)
    tol = tolerances()[0]
    plane = (H - 2) * (W - 2)
    try:
        _lib.check(_lib.lib().dbm_set_deterministic(ctx.handle, det), ctx.handle)
        raw, cat, S = run_backward(dbm, dd, gd, gch)
        eW, eb = backward_errors(raw, gd)
        print(f"BWD {rid:12s} {mag:6s} det={det} cat {cat} S {S} gW {eW:.3e} (tol {tol['gW']:.3e}) gb {eb:.3e} (tol {tol['gb']:.3e})")
        want = expected_wgrad_cat(plane, gch * plane)
        assert cat == [want, want], (rid, cat, want)
        assert all(s >= 1 for s in S), S
        if rid == "b-11-n64":
            assert S[0] >= 2, ("the 900-channel branch no longer splits K at 5184 positions", S)
        if rid == "b-20x72-n1":
            assert want == 9
        assert eW <= tol["gW"], (eW, tol["gW"])
        assert eb <= tol["gb"], (eb, tol["gb"])
        if det:
            raw2, cat2, S2 = run_backward(dbm, dd, gd, gch)
            assert (cat2, S2) == (cat, S)
            assert all(same_bytes(a, b) for a, b in zip(raw, raw2)), "deterministic mode: a repeated call gave other bits"
    finally:
        restore_deterministic(ctx)


# ------------------------------------------------------------------------------------------------------------------------
# the few-channel weight-gradient kernels
# ------------------------------------------------------------------------------------------------------------------------
PER_ELEMENT, PARTIAL_FOLD = 0, 1
# (id, N, C, H, W, O, k, stride, pad, with scratch, form that must run, gb)
SC_ROWS = (
    ("s-16383", 1, 1, 127, 129, 8, 3, 1, 1, 1, PER_ELEMENT, 1),        # one position below the threshold
    ("s-16384", 16, 1, 32, 32, 8, 3, 1, 1, 1, PARTIAL_FOLD, 1),        # exactly on it; power-of-two plane and width: the decode is one
                                                                       # short on every row
    ("s-disc", 13, 1, 36, 36, 64, 3, 1, 1, 1, PARTIAL_FOLD, 1),        # the discriminator's own smallest
    ("s-w1", 3, 1, 5462, 1, 8, 3, 1, 1, 1, PARTIAL_FOLD, 1),           # width 1
    ("s-ragged", 5, 1, 57, 59, 8, 3, 1, 1, 1, PARTIAL_FOLD, 0),        # 16815 positions, odd sizes, no bias gradient
    ("s-pad0", 20, 1, 32, 32, 8, 3, 1, 0, 1, PER_ELEMENT, 1),          # 18000 positions with scratch, but not conv_layer0's geometry
    ("s-2ch", 9, 2, 44, 44, 8, 2, 1, 0, 1, PER_ELEMENT, 1),            # 16641 positions, eight taps in two channels: the same
    ("s-16384-plain", 16, 1, 32, 32, 8, 3, 1, 1, 0, PER_ELEMENT, 1),   # without scratch the large shape takes the per-element kernel
    ("s-disc-plain", 13, 1, 36, 36, 64, 3, 1, 1, 0, PER_ELEMENT, 0),
    ("s-in-w2", 2, 2, 22, 22, 32, 6, 2, 0, 0, PER_ELEMENT, 1),         # the input block's own geometries on small planes
    ("s-in-w1", 1, 1, 110, 110, 32, 30, 10, 0, 0, PER_ELEMENT, 1),
)
SC_IDS = [r[0] for r in SC_ROWS]


@functools.lru_cache(maxsize=None)
def sc_data(row):
    rid, N, Cc, H, W, O, k, stride, pad, _, _, has_gb = row
    rs = np.random.RandomState([N, Cc, H, W, O, k, stride, pad])
    x = rs.normal(size=(N, Cc, H, W)).astype(np.float32)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gy = rs.normal(size=(N, O, OH, OW)).astype(np.float32)
    w = np.zeros((O, Cc, k, k))
    x64, gy64 = x.astype(np.float64), gy.astype(np.float64)
    _, gW, gb = ops.conv2d_backward(x64, w, gy64, stride=stride, pad=pad, need_gx=False)
    _, mW, mb = ops.conv2d_backward(np.abs(x64), w, np.abs(gy64), stride=stride, pad=pad, need_gx=False)
    _, gW32, gb32 = ops.conv2d_backward(x, w.astype(np.float32), gy, stride=stride, pad=pad, need_gx=False)
    gW0 = (rs.uniform(-1, 1, gW.shape) * np.where(mW > 0, mW, 1.0)).astype(np.float32)
    gb0 = (rs.uniform(-1, 1, gb.shape) * np.where(mb > 0, mb, 1.0)).astype(np.float32)
    for a in (x, gy, gW0, gb0):
        a.setflags(write=False)
    o32 = {"gW": worst_rel(gW32.astype(np.float64) - gW, mW, "float32 oracle gW"), "gb": worst_rel(gb32.astype(np.float64) - gb, mb, "float32 oracle gb")}
    return {"x": x, "gy": gy, "gW": gW, "gb": gb, "mW": mW, "mb": mb, "gW0": gW0, "gb0": gb0, "oracle32": o32}


def test_smallcin_table_sits_on_its_threshold():
    """The rows' position counts against the launcher's threshold (16384), before anything is launched."""
    count = {r[0]: r[1] * ((r[3] + 2 * r[8] - r[6]) // r[7] + 1) * ((r[4] + 2 * r[8] - r[6]) // r[7] + 1) for r in SC_ROWS}
    assert count["s-16383"] == 16383 and count["s-16384"] == 16384 and count["s-disc"] == 13 * 36 * 36 and count["s-w1"] == 16386
    assert count["s-ragged"] % 64 != 0 and count["s-ragged"] >= 16384 and count["s-pad0"] >= 16384 and count["s-2ch"] >= 16384
    for T in (count["s-disc"], count["s-w1"], count["s-ragged"]):   # short last slices, never empty ones (module docstring)
        chunk = -(-T // 64)
        assert 0 < T - 63 * chunk < chunk


@pytest.mark.parametrize("rid", SC_IDS)
def test_smallcin_wgrad(dbm, rid):
    d, _lib, ctx = dbm
    row = SC_ROWS[SC_IDS.index(rid)]
    _, N, Cc, H, W, O, k, stride, pad, scratch, want, has_gb = row
    sd = sc_data(row)
    tol = tolerances()[0]
    x, gy = Guarded(d, sd["x"]), Guarded(d, sd["gy"])
    gW, gb = Guarded(d, sd["gW0"]), Guarded(d, sd["gb0"])
    runs = []
    for _ in range(2):
        gW.set(sd["gW0"])
        gb.set(sd["gb0"])
        f = C.c_int(-99)
        ctx.call("dbm_op_smallcin_wgrad", x.ptr, gy.ptr, gW.ptr, gb.ptr if has_gb else None, N, Cc, H, W, O, k, stride, pad, scratch, C.byref(f))
        runs.append((gW.get(), gb.get(), f.value))
    assert same_bytes(x.get(), sd["x"]) and same_bytes(gy.get(), sd["gy"])
    assert runs[0][2] == runs[1][2] == want, (rid, "form_out", runs[0][2], "expected", want)
    assert same_bytes(runs[0][0], runs[1][0]) and same_bytes(runs[0][1], runs[1][1]), "two launches from the same prefill differ"
    eW = worst_rel(runs[0][0].astype(np.float64) - sd["gW0"] - sd["gW"], sd["mW"] + np.abs(sd["gW0"]), "gW")
    if has_gb:
        eb = worst_rel(runs[0][1].astype(np.float64) - sd["gb0"] - sd["gb"], sd["mb"] + np.abs(sd["gb0"]), "gb")
    else:
        assert same_bytes(runs[0][1], sd["gb0"]), "gb was NULL, the buffer beside it changed"
        eb = 0.0
    print(f"SC {rid:14s} form {want} gW {eW:.3e} (tol {tol['gW']:.3e}) gb {eb:.3e} (tol {tol['gb']:.3e})")
    assert eW <= tol["gW"], (eW, tol["gW"])
    assert eb <= tol["gb"], (eb, tol["gb"])


def test_tolerances_of_this_file():
    tol, worst = tolerances()
    print("float32 oracle's worst " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("tolerances             " + " ".join(f"{k} {v:.2e}" for k, v in tol.items()))
    assert all(TOL_FLOOR <= v <= TOL_CAP for v in tol.values())


# ------------------------------------------------------------------------------------------------------------------------
# backward of the nearest x2 resize, LeakyReLU derivative fused in
# ------------------------------------------------------------------------------------------------------------------------
SUMPOOL_NC = 130   # channel planes: more than one workgroup from the 9 x 9 plane on


@pytest.mark.parametrize("masked", [0, 1], ids=["plain", "masked"])
@pytest.mark.parametrize("H,W", [(1, 1), (9, 9), (5, 7), (18, 18)])
def test_sumpool2(dbm, H, W, masked):
    """Bit for bit against NumPy float32 in the kernel's association, (g00 + g01) + (g10 + g11); the derivative is 1 for mask >= 0 --
    both zeros included, the rule stated in test_gpu_conv_launches.py -- and 0.2 below, denormals of either sign counted by their sign."""
    d, _lib, ctx = dbm
    rs = np.random.RandomState([H, W, masked])
    g = rs.normal(size=(SUMPOOL_NC, 2 * H, 2 * W)).astype(np.float32)
    mask = rs.normal(size=(SUMPOOL_NC, H, W)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45], np.float32)
    flat = mask.reshape(-1)
    where = rs.permutation(flat.size)[:min(flat.size // 2, 48)]
    flat[where] = special[np.arange(where.size) % special.size]
    assert np.signbit(flat[where[1]]) and flat[where[1]] == 0 and flat[where[3]] < 0
    want = (g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + (g[:, 1::2, 0::2] + g[:, 1::2, 1::2])
    assert want.dtype == np.float32
    if masked:
        want = np.where(mask >= 0, want, np.float32(0.2) * want)
        zeros = mask == 0
        assert zeros.any() and same_bytes(want[zeros], ((g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + (g[:, 1::2, 0::2] + g[:, 1::2, 1::2]))[zeros])
    dg, dm = Guarded(d, g), Guarded(d, mask)
    out = Guarded(d, np.full((SUMPOOL_NC, H, W), np.nan, np.float32))
    ctx.call("dbm_op_sumpool2", dg.ptr, dm.ptr if masked else None, out.ptr, SUMPOOL_NC, H, W)
    got = out.get()
    assert same_bytes(dg.get(), g) and same_bytes(dm.get(), mask)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:4], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]], mask.reshape(-1)[bad[:4]])
