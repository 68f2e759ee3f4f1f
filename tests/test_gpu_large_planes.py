"""-m gpu: the deformable layers on planes past the index limits of their LDS-window kernels.

deform_conv64_fusedw_kernel (fp32, planes up to ~36 wide) and deform_conv64_x3w_kernel (split-bf16) read the corners of a sample that
leaves their window at 32-bit byte offsets from the image's first pixel (wrap past 2^24 pixels) and carry a tap's corner packed as
(y0 + 2) << 16 | (x0 + 2) (wrong past 32765 rows or 65533 columns).  The launchers take the gathering kernels (64-bit offsets, the same
bits) past those limits, and refuse a caller that forces a window kernel there (form 3).  Every case checks a band of output rows (or
columns) just past a limit and one well before it against the oracle, evaluated at those positions only with the full plane's
coordinate normalisation (ops.deform_conv2d_at), and pins which kernel ran on each side of each limit (profiler tags).  Offsets put many
samples outside the window: normal with scale 4, or scale 0.5 with a quarter of the taps at scale 6.
"""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import model as omodel
from oracle import ops

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_BOUND = 3e-2   # the bf16 inference mode against the fp32 oracle (test_gpu_model.py::test_generator_bf16_inference_mode)
PIX_LIMIT = 1 << 24  # pixels of one image the window kernels' byte offsets reach


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _inputs(N, H, W, offsets, seed):
    g = np.random.default_rng(seed)
    x = g.random((N, 64, H, W), dtype=np.float32)
    x *= 2
    x -= 1
    off = g.standard_normal((N, 18, H, W), dtype=np.float32)
    if offsets == "normal4":
        off *= 4
    else:   # "mixed": scale 0.5, a quarter of the taps at scale 6
        far = g.random((N, 18, H, W), dtype=np.float32) < 0.25
        off *= np.where(far, np.float32(6), np.float32(0.5))
        del far
    w = (g.standard_normal((64, 64, 3, 3)) / np.sqrt(64 * 9)).astype(np.float32)
    b = g.standard_normal(64).astype(np.float32)
    return x, off, w, b


def _rows(d, _lib, ctx, y, N, O, H, W, r0, r1):
    """Rows r0 .. r1 - 1 of every (image, channel) plane of the device tensor y (N, O, H, W)."""
    out = np.empty((N, O, r1 - r0, W), np.float32)
    lib = _lib.lib()
    for n in range(N):
        for o in range(O):
            src = y.ptr + 4 * (((n * O + o) * H + r0) * W)
            _lib.check(lib.dbm_memcpy_d2h(ctx.handle, out[n, o].ctypes.data_as(C.c_void_p), C.c_void_p(src), 4 * (r1 - r0) * W),
                       ctx.handle)
    return out


def _profiled(_lib, ctx, call):
    """Runs call() inside a profiler bracket; returns (status, message, tags of the deformable forward launches)."""
    lib = _lib.lib()
    _lib.check(lib.dbm_profile_begin(ctx.handle), ctx.handle)
    rc = call()
    msg = lib.dbm_last_error(ctx.handle).decode() if rc else ""
    tags = [r["tag"] for r in ctx.profile_records() if r["tag"].startswith("deform")]
    return rc, msg, tags


def _window_ok(H, W):
    return 256 * H * W < (1 << 32) and H <= 32765 and W <= 65533


# name: N, H, W, offsets, [(plane (H, W) the case also runs on the same buffers, just inside the limits)], row bands, column bands
CASES = {
    # the row field of the packed corner (fusedw: W <= 36; x3w): rows >= 32766 wrap
    "rows_32800x36": (1, 32800, 36, "normal4", [(32765, 36)], [(100, 108), (32770, 32800)], None),
    "rows_32800x4": (1, 32800, 4, "mixed", [(32765, 4)], [(100, 116), (32760, 32800)], None),
    # the column field (x3w only: fusedw's window cannot hold the row): columns >= 65534 carry into the row
    "cols_8x65540": (1, 8, 65540, "normal4", [(8, 65533)], [(0, 8)], [(1000, 1064), (65470, 65540)]),
    # 32-bit byte offsets of one image: pixels >= 2^24 (x3w; fp32 takes the gathering kernel on a plane this wide anyway)
    "bytes_4100x4100": (1, 4100, 4100, "mixed", [(4096, 4095)], [(2000, 2004), (4093, 4100)], None),
    # ... and fusedw's (also past the row limit: the band before the limits lies in the first 32765 rows)
    "bytes_466100x36": (1, 466100, 36, "normal4", [], [(1000, 1008), (466080, 466100)], None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_deform_forward_past_the_window_limits(dbm, case):
    """dbm_op_deform_conv2d (fp32, O = 64), dbm_op_deform_conv2d_form forms 2 / 3 / 4 (split-bf16, O = 64) and form 1 (O = 1 and 3,
    premultiplied: the generator's last layer) against the oracle on both bands; form 2 = form 4 bit for bit; form 3 refused past a
    limit (DBM_CHECK naming it) and bitwise form 4 where it runs; the launchers' kernel choice pinned by the profiler tags.
    (The case runs in a frame of its own: a failure's traceback does not keep its gigabytes of host and device arrays alive.)"""
    try:
        failures = _forward_case(dbm, case)
    except AssertionError as e:
        failures = [f"{type(e).__name__}: {e}"]
    gc.collect()
    assert not failures, failures


def _forward_case(dbm, case):
    d, _lib, ctx = dbm
    lib = _lib.lib()
    N, H, W, offsets, inside, bands, cbands = CASES[case]
    x, off, w, b = _inputs(N, H, W, offsets, seed=len(case) * 1000 + H % 997)
    dx, doff, dw, db = d.to_device(x), d.to_device(off), d.to_device(w), d.to_device(b)
    y, y4 = d.DeviceArray((N, 64, H, W)), d.DeviceArray((N, 64, H, W))
    failures = []

    def check(label, got, ref, tol):
        err = _rel(got, ref)
        if not err < tol:
            failures.append(f"{label}: {err:.3g}")

    refs = {}

    def bands_of(dev, O, lrelu, label):
        for r0, r1 in bands:
            got = _rows(d, _lib, ctx, dev, N, O, H, W, r0, r1)
            for c0, c1 in (cbands or [(0, W)]):
                key = (O, r0, r1, c0, c1)
                if key not in refs:
                    refs[key] = ops.deform_conv2d_at(x, off, w[:O], b[:O], rows=np.arange(r0, r1), cols=np.arange(c0, c1))
                ref = refs[key]
                if lrelu:
                    ref = np.where(ref >= 0, ref, np.float32(0.2) * ref)
                check(f"{label} rows {r0}:{r1} cols {c0}:{c1}", got[..., c0:c1], ref, TOL)

    # fp32 64 -> 64 (fusedw on narrow planes inside the limits, the gathering kernel otherwise)
    rc, msg, tags = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, y.ptr, N, 64, H, W, 64))
    assert rc == 0, msg
    bands_of(y, 64, 0, "fp32")
    fp32_tags = tags
    # split-bf16: form 4 (gathering), form 2 (the launcher's choice), form 3 (forced window)
    rc, msg, tags4 = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, y4.ptr, N, H, W, 64, 4, 1))
    assert rc == 0, msg
    bands_of(y4, 64, 1, "form 4")
    rc, msg, tags2 = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, y.ptr, N, H, W, 64, 2, 1))
    assert rc == 0, msg
    bands_of(y, 64, 1, "form 2")
    for r0, r1 in bands:
        if not np.array_equal(_rows(d, _lib, ctx, y, N, 64, H, W, r0, r1), _rows(d, _lib, ctx, y4, N, 64, H, W, r0, r1)):
            failures.append(f"form 2 != form 4 on rows {r0}:{r1}")
    rc3, msg3, tags3 = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, y.ptr, N, H, W, 64, 3, 1))
    if rc3 == 0:
        bands_of(y, 64, 1, "form 3 (should have been refused)")
        failures.append("form 3 ran past the window limits")
    else:
        assert "LDS-window kernel" in msg3 and "H <= 32765, W <= 65533, H * W < 2^24" in msg3, msg3
    # which kernel ran past the limits: the gathering ones (not the window kernels)
    for label, tg, prefix in (("fp32", fp32_tags, "deform64_"), ("form 4", tags4, "deform64x3_"), ("form 2", tags2, "deform64x3_")):
        if not (tg and all(t.startswith(prefix) for t in tg)):
            failures.append(f"{label} ran {tg}")
    # form 1: the generator's last layer (O = 1, and 3 for GeneratorModel(out_channels=3))
    for O in (1, 3):
        wo = w[:O].copy()
        dwo, dbo, yo = d.to_device(wo), d.to_device(b[:O]), d.DeviceArray((N, O, H, W))
        rc, msg, _ = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dwo.ptr, dbo.ptr, yo.ptr, N, H, W, O, 1, 0))
        assert rc == 0, msg
        bands_of(yo, O, 0, f"form 1 O={O}")
        del dwo, dbo, yo
    # the same buffers as a plane just inside the limits: the window kernels run there, bitwise the gathering kernel, on the oracle
    for Hi, Wi in inside:
        assert _window_ok(Hi, Wi) and Hi * Wi <= H * W
        xi = x.reshape(-1)[:N * 64 * Hi * Wi].reshape(N, 64, Hi, Wi)
        oi = off.reshape(-1)[:N * 18 * Hi * Wi].reshape(N, 18, Hi, Wi)
        yi3, yi4 = y, y4   # (the full plane's outputs are checked: their buffers hold the smaller plane)
        rc, msg, ti3 = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, yi3.ptr, N, Hi, Wi, 64, 3, 1))
        assert rc == 0, msg
        assert any(t.startswith(f"deform64x3w_{Hi}x{Wi}_") for t in ti3), ti3
        rc, msg, ti2 = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, yi4.ptr, N, Hi, Wi, 64, 2, 1))
        assert rc == 0, msg
        assert any(t.startswith(f"deform64x3w_{Hi}x{Wi}_") for t in ti2), ti2   # the launcher's choice there: the window
        lo, hi = (Hi - 16, Hi) if Hi > 8 else (0, Hi)
        a3 = _rows(d, _lib, ctx, yi3, N, 64, Hi, Wi, lo, hi)
        rc, msg, _ = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, yi4.ptr, N, Hi, Wi, 64, 4, 1))
        assert rc == 0, msg
        if not np.array_equal(a3, _rows(d, _lib, ctx, yi4, N, 64, Hi, Wi, lo, hi)):
            failures.append(f"form 3 != form 4 on {Hi}x{Wi}")
        cols = np.arange(Wi - 64, Wi) if Wi > 4096 else np.arange(Wi)
        ref = ops.deform_conv2d_at(xi, oi, w, b, rows=np.arange(lo, hi), cols=cols)
        check(f"form 3 on {Hi}x{Wi}", a3[..., cols], np.where(ref >= 0, ref, np.float32(0.2) * ref), TOL)
        # one row / column / pixel more: refused when forced, the gathering kernel when chosen
        Ho, Wo = (Hi + 1, Wi) if Hi == 32765 else (Hi, Wi + 1)
        assert not _window_ok(Ho, Wo) and Ho * Wo <= H * W
        rc, msg, _ = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, yi3.ptr, N, Ho, Wo, 64, 3, 1))
        if rc == 0:
            failures.append(f"form 3 ran on {Ho}x{Wo}")
        else:
            assert "H <= 32765, W <= 65533, H * W < 2^24" in msg, msg
        rc, msg, tags = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d_form(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, yi3.ptr, N, Ho, Wo, 64, 2, 1))
        assert rc == 0, msg
        if not (tags and all(t.startswith(f"deform64x3_{Ho}x{Wo}_") for t in tags)):
            failures.append(f"form 2 on {Ho}x{Wo} ran {tags}")
    return failures


def test_fp32_window_kernel_on_both_sides_of_the_row_limit(dbm):
    """deform_conv64_fusedw_kernel (the fp32 64 -> 64 layer on narrow planes) serves 32765 rows and hands 32766 to the gathering
    kernel: tags on both sides, bitwise DBM_DEFORM_FWD_WINDOW's two kernels where both may run (checked by the oracle on the last rows)."""
    d, _lib, ctx = dbm
    lib = _lib.lib()
    N, W = 1, 4
    x, off, w, b = _inputs(N, 32766, W, "normal4", seed=5)
    dx, doff, dw, db = d.to_device(x), d.to_device(off), d.to_device(w), d.to_device(b)
    y = d.DeviceArray((N, 64, 32766, W))
    for H, kind in ((32765, "deform64w_"), (32766, "deform64_")):
        xi = x.reshape(-1)[:N * 64 * H * W].reshape(N, 64, H, W)
        oi = off.reshape(-1)[:N * 18 * H * W].reshape(N, 18, H, W)
        rc, msg, tags = _profiled(_lib, ctx, lambda: lib.dbm_op_deform_conv2d(ctx.handle, dx.ptr, doff.ptr, dw.ptr, db.ptr, y.ptr, N, 64, H, W, 64))
        assert rc == 0, msg
        assert tags and all(t.startswith(kind) for t in tags), (H, tags)
        got = _rows(d, _lib, ctx, y, N, 64, H, W, H - 24, H)
        assert _rel(got, ops.deform_conv2d_at(xi, oi, w, b, rows=np.arange(H - 24, H))) < TOL, H


def test_deform_backward_on_a_tall_strip(dbm):
    """dbm_op_deform_conv2d_backward (O = 64) on 32800 x 4: past the CSR kernel's plane guard (the sampler + GEMM + atomic kernels).
    gy is zero outside two bands (one past the window kernels' row limit): the backward is linear in gy, so the oracle on those bands
    is the whole answer."""
    d, _lib, ctx = dbm
    lib = _lib.lib()
    N, H, W = 1, 32800, 4
    x, off, w, b = _inputs(N, H, W, "mixed", seed=9)
    rows = np.r_[200:216, 32768:32800]
    g = np.random.default_rng(10)
    gyb = g.standard_normal((N, 64, len(rows), W), dtype=np.float32)
    gy = np.zeros((N, 64, H, W), np.float32)
    gy[:, :, rows] = gyb
    dx, doff, dw, dgy = d.to_device(x), d.to_device(off), d.to_device(w), d.to_device(gy)
    gx, goff = d.DeviceArray(x.shape), d.DeviceArray(off.shape)
    gw, gb = d.to_device(np.zeros_like(w)), d.to_device(np.zeros(64, np.float32))
    _lib.check(lib.dbm_op_deform_conv2d_backward(ctx.handle, dx.ptr, doff.ptr, dw.ptr, dgy.ptr, gx.ptr, goff.ptr, gw.ptr, gb.ptr,
                                                 N, 64, H, W, 64), ctx.handle)
    ctx.synchronize()
    gx_ref, goff_ref, gw_ref, gb_ref = ops.deform_conv2d_backward(x, off, w, gyb, rows=rows)
    assert _rel(gx.get(), gx_ref) < TOL
    goff_h = goff.get()
    assert _rel(goff_h[:, :, rows], goff_ref) < 5e-4   # (test_gpu_ops.py's bound for the coordinate gradient)
    goff_h[:, :, rows] = 0
    assert not goff_h.any()                              # zero wherever gy is
    assert _rel(gw.get(), gw_ref) < TOL
    assert _rel(gb.get(), gb_ref) < TOL


def _bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


@pytest.mark.parametrize("H,W,runs", [(2047, 4098, True), (2048, 4096, False)])
def test_cl16_trunk_conv_on_both_sides_of_its_plane_limit(dbm, H, W, runs):
    """conv_cl16 (the bf16 mode's trunk) reaches one image's fp32 operands through 32-bit byte offsets: it serves planes of < 2^23
    pixels (256 bytes per pixel < 2^31) and refuses the rest with a DBM_CHECK (never a dropped store).  Inside: the last rows against
    the oracle on bf16-rounded operands (test_gpu_cl16.py's bound)."""
    d, _lib, ctx = dbm
    N, Cc, O = 1, 32, 32
    g = np.random.default_rng(H)
    x = g.standard_normal((N, Cc, H, W), dtype=np.float32)
    w = (g.standard_normal((O, Cc, 3, 3)) / np.sqrt(9 * Cc)).astype(np.float32)
    b = g.standard_normal(O).astype(np.float32)
    dx, dw, db, y = d.to_device(x), d.to_device(w), d.to_device(b), d.DeviceArray((N, O, H, W))
    rc = _lib.lib().dbm_op_conv2d_cl16(ctx.handle, dx.ptr, dw.ptr, db.ptr, None, 1.0, y.ptr, N, Cc, H, W, O, 1)
    if not runs:
        assert rc != 0 and "32-bit epilogue offsets" in _lib.lib().dbm_last_error(ctx.handle).decode()
        return
    _lib.check(rc, ctx.handle)
    r0 = H - 8
    got = _rows(d, _lib, ctx, y, N, O, H, W, r0, H)
    ref = ops.conv2d(_bf16_round(x[:, :, r0 - 1:]).astype(np.float64), _bf16_round(w).astype(np.float64), b.astype(np.float64), 1, 1)
    ref = ref[:, :, 1:]   # (row r0 - 1 only fed its neighbours; the bottom row's zero padding is the plane's own)
    ref = np.where(ref >= 0, ref, 0.2 * ref)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 2e-5


def test_bf16_generator_refuses_trunk_planes_past_the_cl16_limit(dbm):
    """The bf16 mode's trunk plane (H - 2) x (W - 2) must stay <= 5592405 pixels (conv_cl16's 192-channel bf16 concat at 32-bit byte
    offsets: 384 bytes per pixel < 2^31).  dbm_gen_forward refuses a larger one up front, before any buffer is sized for it; the fp32
    mode serves it.  (The side inside the limit -- a 9440 x 9448 output, ~140 GB of activations -- is beyond a test's budget: the
    launcher's own check of the same expression runs on both sides in the test above.)"""
    d = dbm[0]
    g = d.GeneratorModel(num_residual_blocks=1)
    h = w = 2367                                 # trunk plane 2365 x 2365 = 5593225 pixels
    ins = (np.zeros((1, 1, h, w), np.float32), np.zeros((1, 1, 10 * h, 10 * w), np.float32),
           np.zeros((1, 2, 2 * h, 2 * w), np.float32), np.zeros((1, 1, h, w), np.float32))   # (never touched: calloc pages)
    with pytest.raises(dbm[1].DbmError, match="DBM_BF16 needs"), d.using_config("enable_backprop", False), \
            d.using_config("dtype", "bfloat16"):
        g.forward(*ins)


# ---- generator level: GeneratorModel.forward, 1 RRDB, N = 1 ----

def _scaled_oracle_generator():
    """test_gpu_model.py's scaled_oracle_generator(1, 1.0), with offset convolutions that move the samples by several pixels (biases
    of scale 4, weights x 30): many samples leave the window kernels' windows.  (With the reference's scale the offsets stay within a
    pixel, inside the windows, where no limit but the row / column fields bites.)"""
    g = omodel.GeneratorModel(num_residual_blocks=1, residual_scaling=0.1, seed=3)
    r = np.random.RandomState(4)
    for k in g.params:
        if "offset_conv" in k:
            g.params[k] = (g.params[k] * np.float32(30.0) if k.endswith("/W") else r.normal(0, 4, g.params[k].shape)).astype(np.float32)
        elif not k.endswith("/W"):
            g.params[k] += r.normal(0, 0.1, g.params[k].shape).astype(np.float32)
    return g


def _generator_inputs(h, w, seed):
    g = np.random.default_rng(seed)
    return (g.random((1, 1, h, w), dtype=np.float32), g.random((1, 1, 10 * h, 10 * w), dtype=np.float32),
            g.random((1, 2, 2 * h, 2 * w), dtype=np.float32), g.random((1, 1, h, w), dtype=np.float32))


_GEN_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import deepbedmap_amd as d
from test_gpu_large_planes import _scaled_oracle_generator, _generator_inputs
h, w, mode, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
og = _scaled_oracle_generator()
g = d.GeneratorModel(num_residual_blocks=1, residual_scaling=0.1, initialize=False)
for name, p in g._tensors.items():
    p.array = og.params[name]
ins = _generator_inputs(h, w, 7)
with d.using_config("enable_backprop", False), d.using_config("dtype", "bfloat16" if mode == "bf16" else "float32"):
    y = g.forward(*ins).array
np.save(out, np.asarray(y))
"""


def _generator_in_child(tmp_path, h, w, mode, env):
    script = tmp_path / "gen.py"
    script.write_text(_GEN_SCRIPT)
    out = str(tmp_path / f"y_{mode}_{len(env)}.npy")
    res = subprocess.run([sys.executable, str(script), ROOT, str(h), str(w), mode, out], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    y = np.load(out)
    os.remove(out)
    return y


@pytest.mark.parametrize("h,w", [(8197, 3), (3, 16389)])
def test_generator_on_strips_past_the_row_and_column_limits(dbm, tmp_path, h, w):
    """Outputs 32780 x 4 (the packed corner's row field) and 4 x 65548 (its column field): fp32 against the oracle's whole-strip
    forward at TOL, bf16 at the bf16 mode's bound, and both bit for bit a process on the gathering kernels (DBM_DEFORM_FWD_WINDOW=0,
    DBM_DEFORM_X3_WINDOW=0): a wrong band of a few dozen pixels hides under the bf16 bound."""
    d = dbm[0]
    og = _scaled_oracle_generator()
    g = d.GeneratorModel(num_residual_blocks=1, residual_scaling=0.1, initialize=False)
    for name, p in g._tensors.items():
        p.array = og.params[name]
    ins = _generator_inputs(h, w, 7)
    ref = og.forward(*ins)
    assert ref.shape == (1, 1, 4 * (h - 2), 4 * (w - 2))
    with d.using_config("enable_backprop", False):
        y32 = g.forward(*ins).array
        with d.using_config("dtype", "bfloat16"):
            y16 = g.forward(*ins).array
    errs = {"fp32": _rel(y32, ref), "bf16": _rel(y16, ref)}
    # the part past the limit on its own (max-abs against the whole output's range: a band-local error is not diluted)
    past = (slice(None), slice(None), slice(32766, None)) if h > w else (slice(None), slice(None), slice(None), slice(65530, None))
    errs["fp32 past"] = float(np.abs(y32[past] - ref[past]).max() / np.abs(ref).max())
    errs["bf16 past"] = float(np.abs(y16[past] - ref[past]).max() / np.abs(ref).max())
    errs["fp32 = gathering"] = np.array_equal(y32, _generator_in_child(tmp_path, h, w, "fp32", {"DBM_DEFORM_FWD_WINDOW": "0"}))
    errs["bf16 = gathering"] = np.array_equal(y16, _generator_in_child(tmp_path, h, w, "bf16", {"DBM_DEFORM_X3_WINDOW": "0"}))
    assert errs["fp32"] < TOL and errs["fp32 past"] < TOL and errs["bf16"] < BF16_BOUND and errs["bf16 past"] < BF16_BOUND, errs
    assert errs["fp32 = gathering"] and errs["bf16 = gathering"], errs


@pytest.mark.parametrize("h,w", [(1027, 1027), (116600, 11)])
def test_generator_past_2_24_pixels_equals_the_gathering_kernels(dbm, tmp_path, h, w):
    """Outputs 4100 x 4100 and 466392 x 36 (more than 2^24 pixels, past the window kernels' byte offsets): bf16 bit for bit a process
    with DBM_DEFORM_X3_WINDOW=0, fp32 bit for bit one with DBM_DEFORM_FWD_WINDOW=0 (the gathering kernels), and bf16 against fp32 at
    the bf16 mode's bound on the rows past 2^24 pixels on their own as well as on the whole plane."""
    y16 = _generator_in_child(tmp_path, h, w, "bf16", {})
    y16g = _generator_in_child(tmp_path, h, w, "bf16", {"DBM_DEFORM_X3_WINDOW": "0"})
    same16 = np.array_equal(y16, y16g)
    del y16g
    y32 = _generator_in_child(tmp_path, h, w, "fp32", {})
    y32g = _generator_in_child(tmp_path, h, w, "fp32", {"DBM_DEFORM_FWD_WINDOW": "0"})
    same32 = np.array_equal(y32, y32g)
    del y32g
    gc.collect()
    H, W = y32.shape[2:]
    assert H * W > PIX_LIMIT
    r = -(-PIX_LIMIT // W)   # the first row with pixels past 2^24
    scale = np.abs(y32).max()
    err_all = float(np.abs(y16 - y32).max() / scale)
    err_past = float(np.abs(y16[:, :, r:] - y32[:, :, r:]).max() / scale)
    assert same16 and same32 and err_all < BF16_BOUND and err_past < BF16_BOUND, (same16, same32, err_all, err_past)
