"""-m gpu: the non-GEMM half of the training step (norm_loss.hip) at op level against the float64 NumPy oracle -- every
training-mode BatchNorm form at its edges, the sync_batch_stats kernels, the discriminator's dense head in both backward
sequences, the relativistic loss past one round of its stride loop, and Adam on a whole discriminator arena.

The entry points (dbm_op_batchnorm_train*, dbm_op_disc_head*) run the model's own launch choices: the form is
bn_train_form's, reported through form_out and asserted here against a Python restatement of the selector (`expected_form`),
which pins its thresholds.

BatchNorm tolerances are not taken from the kernels: per quantity, 16 x the worst deviation of the FLOAT32 NumPy oracle from
the float64 one over the whole table (`bn_tolerances`), floor 8 * 2^-24, cap 1e-4 (y, gz, sums) / 1e-5 (statistics).  The
kernels sum <= 32 strided terms per thread, a 64-lane tree, then <= 16 waves in sequence where NumPy sums pairwise: a depth
ratio below 8, with 2 x on top.  Every element is compared: inputs are nudged so that no pre-activation lies within
delta = 1e-5 * max(1, max|v|) of the LeakyReLU's kink (`bn_data`), hence the mask is the reference's alone.

What is compared, per channel (one workgroup owns one channel):
  y                  max|d| / max|ref y|
  gz                 max|d| / (|gamma * inv_std| * max|g~|),  g~ the masked gradient
  ggamma, gbeta      |d| / sum|g~ * xhat|,  |d| / sum|g~|      (float64 L1 mass of the summed terms)
  mean, inv_std, avg_mean, avg_var    |d| / max(|ref|, 1e-3)

Figures of the run on an MI355X (gfx950) that accompanied this file; the tolerances are computed at run time, these are theirs:
  quantity     float32 oracle's worst   tolerance   kernels' worst (all forms; DBM_BN_REG=0 gave the same figures)
  y                  4.58e-07           7.33e-06         4.5e-07
  gz                 2.51e-07           4.02e-06         2.0e-07
  ggamma             1.14e-07           1.83e-06         1.2e-07
  gbeta              4.06e-08           6.50e-07         5.7e-08
  mean               5.10e-06           1.00e-05 (cap)   7.2e-06   (channels whose |mean| < 1e-3: the floor of the denominator)
  inv_std            1.87e-07           2.99e-06         1.2e-07
  avg_mean           5.42e-07           8.67e-06         1.1e-06
  avg_var            1.14e-07           1.82e-06         1.1e-07
Cases per form according to form_out, forward and backward alike (":small" z * 1e-3, ":shift" z + 10):
  reg<2>           (9,3,81) (1,3,64) (64,2,128) (17,2,65) (63,1,127) (9,3,81):small (9,3,81):shift
  reg<6>           (9,2,324) (1,3,129) (64,2,384) (33,1,383) (9,2,324):small (9,2,324):shift
  flat<1>          (16,3,16) (1,2,1) (2,3,1) (256,2,1) (3,257,81) (5,1,51) (4,2,63) (16,3,16):small (16,3,16):shift
  flat<4>          (33,3,16) (257,1,1) (64,2,16) (17,2,60) (12,257,81) (129,2,4) (33,3,16):small (33,3,16):shift
  <1024> cached    (8,3,400) (1,2,385) (64,1,512) (8,3,400):small (8,3,400):shift
  <1024> uncached  (70,1,324) (65,2,64) (2,2,513) (1,1,1296) (129,1,81) (70,1,324):small (70,1,324):shift
  <256>            (65,2,16) (1025,1,1) (20,1,63) (13,257,81) (300,2,4) (65,2,16):small (65,2,16):shift
  sync (bn_sync_*) (9,3,81) (9,2,324) (16,3,16) (33,3,16) (8,3,400) (70,1,324) (65,2,16)
  DBM_BN_REG=0     <1024>: every case of the reg and <1024> rows; <256>: every case of the flat and <256> rows
Between 0 and 13 elements per case were moved off the LeakyReLU's kink, in one pass.
Dense head: fused backward at N = 1, 2, 63, 64, 122, two launches at N = 123, 129, 200.  Worst max-norm deviations l1 1.3e-07,
logits 1.9e-07, gx 4.6e-07, gW1 4.0e-07, gb1 7.1e-07, gW2 3.3e-07, gb2 4.3e-06 (TOL = 1e-4); worst per entry against the L1 mass
gW1 3.8e-07, gb1 1.7e-07, gW2 2.3e-07, gb2 8.3e-08 (1e-5: the worst case did not bite).
Relativistic loss: at most 0.06 of the allowed 2e-6 * max(1, |ref|) on the loss, 4.5e-08 on the gradients (1e-7).
Adam: worst error 0.65 of the per-element bound (gradients of scale 1e-6: 0.65, 1e-3: 0.50, 1: 0.48).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ops
from oracle import train as otrain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4          # the project's criterion for every dbm_op_* contraction (tests/test_gpu_ops.py)
STAT_CAP = 1e-5     # ... and for BatchNorm statistics (tests/test_gpu_model.py)
EPS24 = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------------------
# BatchNorm: the table, the selector's restatement, inputs, references, tolerances
# ------------------------------------------------------------------------------------------------------------------------
FORM_NAMES = ("reg<2>", "reg<6>", "flat<1>", "flat<4>", "<1024>", "<256>")   # BnForm (kernels.h), form_out's values
BN_TABLE = [  # row, expected form, cases (N, C, plane); the row's FIRST case also runs z * 1e-3, z + 10 and sync = 1
    ("reg<2>", 0, [(9, 3, 81), (1, 3, 64), (64, 2, 128), (17, 2, 65), (63, 1, 127)]),
    ("reg<6>", 1, [(9, 2, 324), (1, 3, 129), (64, 2, 384), (33, 1, 383)]),
    ("flat<1>", 2, [(16, 3, 16), (1, 2, 1), (2, 3, 1), (256, 2, 1), (3, 257, 81), (5, 1, 51), (4, 2, 63)]),
    ("flat<4>", 3, [(33, 3, 16), (257, 1, 1), (64, 2, 16), (17, 2, 60), (12, 257, 81), (129, 2, 4)]),
    ("<1024> cached", 4, [(8, 3, 400), (1, 2, 385), (64, 1, 512)]),
    ("<1024> uncached", 4, [(70, 1, 324), (65, 2, 64), (2, 2, 513), (1, 1, 1296), (129, 1, 81)]),
    ("<256>", 5, [(65, 2, 16), (1025, 1, 1), (20, 1, 63), (13, 257, 81), (300, 2, 4)]),
]
BN_RUNS = [(row, case, "plain") for row, _, cases in BN_TABLE for case in cases]
BN_RUNS += [(row, cases[0], v) for row, _, cases in BN_TABLE for v in ("small", "shift", "sync")]
ROW_FORM = {row: form for row, form, _ in BN_TABLE}


def expected_form(N, C, plane, reg_on=True):
    """bn_train_form (norm_loss.hip) restated: bn_reg_slots, then bn_flat_slots, then the general kernels' split."""
    m = N * plane
    small = 4 * m * C < 2 ** 31
    wide = plane >= 64 and C <= 256
    if reg_on and small and N <= 64 and wide and plane <= 384:
        return 0 if plane <= 128 else 1
    if reg_on and small and not wide and m <= 1024:
        return 2 if m <= 256 else 3
    return 4 if wide else 5


def wide_cached(N, plane):
    """bn_train_*_kernel<1024> keeps a thread's elements in registers for <= 64 images of <= 512 positions"""
    return N <= 64 and plane <= 512


def bn_reference(z, gamma, beta, avg_mean, avg_var, gh, dtype):
    """The oracle's chain in `dtype`: batchnorm_train -> leaky_relu; leaky_relu_backward -> batchnorm_train_backward."""
    z, gamma, beta, gh = (np.asarray(a, dtype) for a in (z, gamma, beta, gh))
    am, av = np.array(avg_mean, dtype), np.array(avg_var, dtype)
    v, (xhat, inv_std) = ops.batchnorm_train(z, gamma, beta, am, av)
    y = ops.leaky_relu(v)
    gt = ops.leaky_relu_backward(y, gh)
    gz, ggamma, gbeta = ops.batchnorm_train_backward(gt, gamma, (xhat, inv_std))
    return {"y": y, "gz": gz, "ggamma": ggamma, "gbeta": gbeta, "mean": z.mean(axis=(0, 2, 3)), "inv_std": inv_std,
            "avg_mean": am, "avg_var": av, "v": v, "gt": gt, "xhat": xhat}


@functools.lru_cache(maxsize=None)
def bn_data(case, variant):
    """float32 inputs of one case and their float64 reference, shared by every test that needs them (never modified).
    variant: "plain" | "small" (z * 1e-3: the variance falls below eps) | "shift" (z + 10: the two-pass variance)."""
    N, Cc, plane = case
    rs = np.random.RandomState([N, Cc, plane, ("plain", "small", "shift").index(variant)])
    z = rs.normal(size=(N, Cc, plane, 1))
    if variant == "small":
        z *= 1e-3
    if variant == "shift":
        z += 10.0
    z = z.astype(np.float32)
    gamma = (rs.uniform(0.5, 1.5, Cc) * rs.choice([-1.0, 1.0], Cc)).astype(np.float32)
    beta = rs.normal(0, 0.5, Cc).astype(np.float32)
    gh = rs.normal(size=z.shape).astype(np.float32)
    avg_mean = rs.normal(size=Cc).astype(np.float32)
    avg_var = rs.uniform(0.5, 2.0, Cc).astype(np.float32)
    # the LeakyReLU mask is discontinuous: move every z whose pre-activation v lies within delta of zero away from it by
    # 8 delta (in v), so that float32 rounding of v (~ delta / 30) cannot flip a mask and the reference alone decides it
    moved = 0
    for _ in range(8):
        ref = bn_reference(z, gamma, beta, avg_mean, avg_var, gh, np.float64)
        v = ref["v"]
        delta = 1e-5 * max(1.0, np.abs(v).max())
        bad = np.abs(v) < delta
        if not bad.any():
            break
        moved += int(bad.sum())
        g64 = gamma.astype(np.float64)
        step = 8 * delta / (np.abs(g64) * ref["inv_std"])
        push = np.where(v >= 0, 1.0, -1.0) * (np.sign(g64) * step)[None, :, None, None]
        z = (z.astype(np.float64) + np.where(bad, push, 0.0)).astype(np.float32)
    assert not bad.any(), (case, variant, "pre-activations within delta of the LeakyReLU's kink remain")
    # prefill of the accumulated sums: random, of each channel's own gradient scale (its L1 mass)
    l1g = np.abs(ref["gt"] * ref["xhat"]).sum(axis=(0, 2, 3))
    l1b = np.abs(ref["gt"]).sum(axis=(0, 2, 3))
    gg0 = (rs.uniform(-1, 1, Cc) * np.where(l1g > 0, l1g, 1.0)).astype(np.float32)
    gb0 = (rs.uniform(-1, 1, Cc) * np.where(l1b > 0, l1b, 1.0)).astype(np.float32)
    for a in (z, gamma, beta, gh, avg_mean, avg_var, gg0, gb0):
        a.setflags(write=False)
    return {"case": case, "variant": variant, "z": z, "gamma": gamma, "beta": beta, "gh": gh, "avg_mean": avg_mean,
            "avg_var": avg_var, "gg0": gg0, "gb0": gb0, "ref": ref, "moved": moved}


BN_QUANTITIES = ("y", "gz", "ggamma", "gbeta", "mean", "inv_std", "avg_mean", "avg_var")


def bn_metrics(got, data):
    """Per-channel deviations of `got` from the float64 reference, each in its own unit (module docstring)."""
    ref = data["ref"]
    cmax = lambda a: np.abs(a).max(axis=(0, 2, 3))  # noqa: E731
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    kscale = np.abs(data["gamma"].astype(np.float64) * ref["inv_std"])
    out = {
        "y": cmax(f64(got["y"]) - ref["y"]) / np.maximum(cmax(ref["y"]), 1e-30),
        "gz": cmax(f64(got["gz"]) - ref["gz"]) / np.maximum(kscale * cmax(ref["gt"]), 1e-30),
        "ggamma": np.abs(f64(got["ggamma"]) - ref["ggamma"]) / np.maximum(np.abs(ref["gt"] * ref["xhat"]).sum(axis=(0, 2, 3)), 1e-30),
        "gbeta": np.abs(f64(got["gbeta"]) - ref["gbeta"]) / np.maximum(np.abs(ref["gt"]).sum(axis=(0, 2, 3)), 1e-30),
    }
    for k in ("mean", "inv_std", "avg_mean", "avg_var"):
        out[k] = np.abs(f64(got[k]) - ref[k]) / np.maximum(np.abs(ref[k]), 1e-3)
    return out


@functools.lru_cache(maxsize=None)
def bn_tolerances():
    """16 x the float32 oracle's worst deviation from the float64 one over the whole table, per quantity, floor 8 * 2^-24,
    cap TOL / STAT_CAP.  Table-wide, not per case: single cases deviate by as little as 5e-12 by chance."""
    worst = dict.fromkeys(BN_QUANTITIES, 0.0)
    for _, case, variant in BN_RUNS:
        if variant != "plain":
            continue
        dd = bn_data(case, "plain")
        o32 = bn_reference(dd["z"], dd["gamma"], dd["beta"], dd["avg_mean"], dd["avg_var"], dd["gh"], np.float32)
        for k, v in bn_metrics(o32, dd).items():
            worst[k] = max(worst[k], float(v.max()))
    cap = {k: (STAT_CAP if k in ("mean", "inv_std", "avg_mean", "avg_var") else TOL) for k in BN_QUANTITIES}
    return {k: min(cap[k], max(8 * EPS24, 16 * worst[k])) for k in BN_QUANTITIES}, worst


def bn_check(data, got, variant):
    """Deviations per quantity and the list of quantities out of tolerance.  variant "shift": y and gz additionally get
    16 * 2^-24 * |mean| * inv_std per channel, the float32 rounding of the mean itself."""
    tol, _ = bn_tolerances()
    met = bn_metrics(got, data)
    ref = data["ref"]
    extra = 16 * EPS24 * np.abs(ref["mean"]) * ref["inv_std"] if variant == "shift" else 0.0
    figures, failed = {}, []
    for k in BN_QUANTITIES:
        allow = tol[k] + (extra if k in ("y", "gz") else 0.0)
        figures[k] = float(met[k].max())
        if not np.all(met[k] <= allow):   # (NaN fails)
            c = int(np.argmax(np.where(np.isnan(met[k]), np.inf, met[k] - allow)))
            failed.append(f"{k}: {met[k][c]:.3e} > {float(np.broadcast_to(allow, met[k].shape)[c]):.3e} (channel {c})")
    return figures, failed


# ------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------
PAD = 256
SENTINEL = np.float32(-6.0221e23)


class Guarded:
    """A float32 device tensor inside a larger allocation, PAD sentinel floats on either side; `get` checks them."""

    def __init__(self, d, host):
        host = np.ascontiguousarray(host, dtype=np.float32)
        self.shape, self.n = host.shape, host.size
        self.arr = d.to_device(self._padded(host))
        self.ptr = C.c_void_p(self.arr.ptr + 4 * PAD)

    def _padded(self, host):
        buf = np.full(self.n + 2 * PAD, SENTINEL, np.float32)
        buf[PAD:PAD + self.n] = host.ravel()
        return buf

    def set(self, host):
        self.arr.set(self._padded(np.ascontiguousarray(host, dtype=np.float32)))

    def get(self):
        full = self.arr.get()
        guard = np.concatenate([full[:PAD], full[PAD + self.n:]])
        assert np.array_equal(guard.view(np.uint32), np.full(2 * PAD, SENTINEL).view(np.uint32)), "a sentinel beside the tensor was overwritten"
        return full[PAD:PAD + self.n].reshape(self.shape).copy()


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def bn_run_gpu(dbm, data, sync):
    """Forward, then the backward pass twice from the same prefill.  Returns (results, forward form, backward form)."""
    d, _lib, ctx = dbm
    N, Cc, plane = data["case"]
    G = lambda a: Guarded(d, a)  # noqa: E731
    nan = lambda shape: np.full(shape, np.nan, np.float32)  # noqa: E731
    z, gamma, beta, gh = G(data["z"]), G(data["gamma"]), G(data["beta"]), G(data["gh"])
    am, av = G(data["avg_mean"]), G(data["avg_var"])
    y, mean, istd = G(nan(data["z"].shape)), G(nan(Cc)), G(nan(Cc))
    gz, gg, gb = G(nan(data["z"].shape)), G(data["gg0"]), G(data["gb0"])
    f_fwd, f_bwd = C.c_int(-99), C.c_int(-99)
    ctx.call("dbm_op_batchnorm_train", z.ptr, gamma.ptr, beta.ptr, am.ptr, av.ptr, y.ptr, mean.ptr, istd.ptr, N, Cc, plane, int(sync),
             C.byref(f_fwd))
    runs = []
    for _ in range(2):
        gz.set(nan(data["z"].shape))
        gg.set(data["gg0"])
        gb.set(data["gb0"])
        ctx.call("dbm_op_batchnorm_train_backward", z.ptr, gh.ptr, gamma.ptr, beta.ptr, mean.ptr, istd.ptr, gz.ptr, gg.ptr, gb.ptr, N, Cc,
                 plane, int(sync), C.byref(f_bwd))
        runs.append((gz.get(), gg.get(), gb.get()))
    assert all(same_bytes(a, b) for a, b in zip(*runs)), "two backward passes from the same prefill differ"
    for t, src in ((z, "z"), (gamma, "gamma"), (beta, "beta"), (gh, "gh")):   # inputs and their sentinels: untouched
        assert same_bytes(t.get(), data[src]), src
    got = {"y": y.get(), "mean": mean.get(), "inv_std": istd.get(), "avg_mean": am.get(), "avg_var": av.get(), "gz": runs[0][0],
           "ggamma": runs[0][1].astype(np.float64) - data["gg0"], "gbeta": runs[0][2].astype(np.float64) - data["gb0"]}
    return got, f_fwd.value, f_bwd.value


def bn_run_and_check(dbm, row, case, variant, reg_on=True):
    """One line of figures and the list of failures (empty: the case passes)."""
    data = bn_data(case, "plain" if variant == "sync" else variant)
    got, f_fwd, f_bwd = bn_run_gpu(dbm, data, variant == "sync")
    figures, failed = bn_check(data, got, variant)
    want = -1 if variant == "sync" else expected_form(*case, reg_on=reg_on)
    if (f_fwd, f_bwd) != (want, want):
        failed.append(f"form_out {f_fwd} / {f_bwd}, selector restatement {want}")
    if reg_on and variant != "sync":
        if want != ROW_FORM[row] or ("<1024>" in row and wide_cached(case[0], case[2]) != ("uncached" not in row)):
            failed.append(f"the selector puts {case} outside its row {row}")
    line = f"BN {row:16s} {str(case):15s} {variant:5s} form {f_fwd:2d} moved {data['moved']:2d} " + " ".join(f"{k} {v:.2e}" for k, v in figures.items())
    return line, failed


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


def test_bn_table_lands_in_its_rows():
    """The case table against the selector's restatement, before anything is launched."""
    for row, form, cases in BN_TABLE:
        for N, Cc, plane in cases:
            assert expected_form(N, Cc, plane) == form, (row, N, Cc, plane)
            assert expected_form(N, Cc, plane, reg_on=False) in (4, 5)
            if form == 4:
                assert wide_cached(N, plane) == (row == "<1024> cached"), (row, N, Cc, plane)


@pytest.mark.parametrize("row,case,variant", BN_RUNS, ids=[f"{r.replace(' ', '_')}-{'x'.join(map(str, c))}-{v}" for r, c, v in BN_RUNS])
def test_batchnorm_train_forward_backward(dbm, row, case, variant):
    """(1, 2, 1) is the m = 1 edge: variance 0, y = beta, gz = 0 exactly, and the correction m / max(m - 1, 1) needs its max.
    The small-m cases of every row make the tolerances bite on that correction and on the 1/m terms: an off-by-one there is a
    relative error of at least 1e-4 at m <= 1025."""
    line, failed = bn_run_and_check(dbm, row, case, variant)
    print(line)
    if row == "flat<1>" and case == (1, 2, 1) and variant == "plain":
        print("BN tolerances " + " ".join(f"{k} {v:.2e}" for k, v in bn_tolerances()[0].items()))
        print("BN float32 oracle's worst " + " ".join(f"{k} {v:.2e}" for k, v in bn_tolerances()[1].items()))
    assert not failed, failed


_BN_REG_OFF_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_norm_ops as t
import deepbedmap_amd as d
from deepbedmap_amd import _lib
dbm = (d, _lib, _lib.default_context())
out = []
for row, case, variant in t.BN_RUNS:
    line, failed = t.bn_run_and_check(dbm, row, case, variant, reg_on=False)
    out.append({"line": line, "failed": failed})
json.dump(out, open(sys.argv[2], "w"))
"""


def test_batchnorm_table_under_dbm_bn_reg_0(tmp_path):
    """The A/B side of the DBM_BN_REG switch under the same reference and tolerances: the whole table once in a fresh process
    with DBM_BN_REG=0, where form_out never names a register-resident form (the restatement with reg_on=False allows only the
    two general kernels, and bn_run_and_check asserts form_out against it)."""
    script, out = tmp_path / "bn_reg_off.py", tmp_path / "bn_reg_off.json"
    script.write_text(_BN_REG_OFF_SCRIPT)
    res = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=dict(os.environ, DBM_BN_REG="0"), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    results = json.load(open(out))
    assert len(results) == len(BN_RUNS)
    for r in results:
        print("REG=0 " + r["line"])
    forms = {int(r["line"].split(" form ")[1].split()[0]) for r in results}
    assert forms <= {4, 5, -1}, forms
    assert not [r for r in results if r["failed"]], [r for r in results if r["failed"]]


# ------------------------------------------------------------------------------------------------------------------------
# the discriminator's dense head, 512 -> 100 -> 1
# ------------------------------------------------------------------------------------------------------------------------
HEAD_K, HEAD_O = 512, 100


@functools.lru_cache(maxsize=None)
def head_data(N):
    """Inputs at the model's scales (x: a LeakyReLU's output, weights HeNormal(0.1)-like but large enough to matter) from the
    first seed of 0..19 whose float64 pre-activation of linear_1 has nothing within delta of the LeakyReLU's kink."""
    for seed in range(20):
        rs = np.random.RandomState([N, seed])
        x = ops.leaky_relu(rs.normal(size=(N, HEAD_K))).astype(np.float32)
        W1 = (rs.normal(size=(HEAD_O, HEAD_K)) * np.sqrt(2.0 / HEAD_K)).astype(np.float32)
        b1 = rs.normal(0, 0.1, HEAD_O).astype(np.float32)
        W2 = (rs.normal(size=(1, HEAD_O)) * np.sqrt(2.0 / HEAD_O)).astype(np.float32)
        b2 = rs.normal(0, 0.1, 1).astype(np.float32)
        gl = rs.normal(size=(N, 1)).astype(np.float32)
        x6, W16, b16, W26, b26, gl6 = (a.astype(np.float64) for a in (x, W1, b1, W2, b2, gl))
        pre = ops.linear(x6, W16, b16)
        if np.abs(pre).min() >= 1e-5 * max(1.0, np.abs(pre).max()):
            break
    else:
        raise AssertionError(f"no seed of 0..19 keeps linear_1's pre-activations off the kink at N = {N}")
    l1 = ops.leaky_relu(pre)
    logits = ops.linear(l1, W26, b26)
    # l1 is an INPUT of the backward pass: it gets the reference's l1 rounded to float32, and the backward reference starts from
    # that array (with the forward's own l1 an entry of gW2 = sum_n glogit[n] l1[n][o] whose l1 is nearly zero would be judged
    # by the rounding of linear_1's 512-term sum, not by the backward kernel: 9.8e-4 of its L1 mass at N = 1)
    l1_in = l1.astype(np.float32)
    l16 = l1_in.astype(np.float64)
    g_l1, gW2, gb2 = ops.linear_backward(l16, W26, gl6)
    gt = ops.leaky_relu_backward(l16, g_l1)
    gx, gW1, gb1 = ops.linear_backward(x6, W16, gt)
    ref = {"l1": l1, "logits": logits[:, 0], "gx": gx, "gW1": gW1, "gb1": gb1, "gW2": gW2[0], "gb2": gb2}
    mass = {"gW1": np.abs(gt).T @ np.abs(x6), "gb1": np.abs(gt).sum(axis=0), "gW2": (np.abs(gl6) * np.abs(l16)).sum(axis=0),
            "gb2": np.abs(gl6).sum(axis=0)}
    pre0 = {k: (rs.uniform(-1, 1, mass[k].shape) * np.where(mass[k] > 0, mass[k], 1.0)).astype(np.float32) for k in mass}
    return {"x": x, "W1": W1, "b1": b1, "W2": W2, "b2": b2, "gl": gl, "l1_in": l1_in, "ref": ref, "mass": mass, "pre0": pre0, "seed": seed}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 122, 123, 129, 200])
def test_disc_head_forward_backward(dbm, N):
    """122 is the last batch whose masked gradient fits the fused backward's 48 KiB of LDS, 123 the first that takes the two
    launch_linear_bwd launches (the second in its non-staged instantiation).  l1, logits, gx: TOL in the max norm; the four
    parameter gradients (accumulated: compared net of a random prefill) additionally per entry against the L1 mass of their
    terms at 1e-5 -- an N <= 200-term fma chain is bounded by 200 * 2^-24 = 1.2e-5 in the worst case, typically far below."""
    d, _lib, ctx = dbm
    hd = head_data(N)
    ref = hd["ref"]
    G = lambda a: Guarded(d, a)  # noqa: E731
    x, W1, b1, W2, b2, gl = (G(hd[k]) for k in ("x", "W1", "b1", "W2", "b2", "gl"))
    l1, logits = G(np.full((N, HEAD_O), np.nan, np.float32)), G(np.full(N, np.nan, np.float32))
    ctx.call("dbm_op_disc_head", x.ptr, W1.ptr, b1.ptr, W2.ptr, b2.ptr, l1.ptr, logits.ptr, N)
    got = {"l1": l1.get(), "logits": logits.get()}
    assert np.array_equal(got["l1"] >= 0, hd["l1_in"] >= 0)   # (the forward's own mask is the reference's)
    l1 = G(hd["l1_in"])
    gx = G(np.full((N, HEAD_K), np.nan, np.float32))
    acc = {k: G(hd["pre0"][k]) for k in ("gW1", "gb1", "gW2", "gb2")}
    fused = C.c_int(-99)
    ctx.call("dbm_op_disc_head_backward", x.ptr, W1.ptr, W2.ptr, gl.ptr, l1.ptr, gx.ptr, acc["gW1"].ptr, acc["gb1"].ptr, acc["gW2"].ptr,
             acc["gb2"].ptr, N, C.byref(fused))
    got["gx"] = gx.get()
    for k in acc:
        got[k] = acc[k].get().astype(np.float64) - hd["pre0"][k]
    for t, k in ((x, "x"), (W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2"), (gl, "gl"), (l1, "l1_in")):
        assert same_bytes(t.get(), hd[k]), k
    figures = {k: rel(got[k], ref[k]) for k in ("l1", "logits", "gx", "gW1", "gb1", "gW2", "gb2")}
    entry = {k: float((np.abs(got[k] - ref[k]) / np.maximum(hd["mass"][k], 1e-30)).max()) for k in hd["mass"]}
    print(f"HEAD N {N:3d} seed {hd['seed']} fused {fused.value} " + " ".join(f"{k} {v:.2e}" for k, v in figures.items()) + " | per entry " +
          " ".join(f"{k} {v:.2e}" for k, v in entry.items()))
    assert fused.value == int(4 * N * HEAD_O <= 49152)
    assert all(v < TOL for v in figures.values()), figures
    assert all(v <= 1e-5 for v in entry.values()), entry


# ------------------------------------------------------------------------------------------------------------------------
# relativistic loss (ragan_loss_kernel) past one round of its 256-thread stride loop
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0, 30.0])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 700])
def test_relativistic_loss(dbm, N, scale):
    """Constant, mixed 0/1 and partly ignored (-1) targets; logits ~ 2 N(0,1) and 30 N(0,1) -- the saturated sigmoid, expf
    overflowing to inf -- against the float64 oracle with the tolerances of test_per_sample_targets_in_both_losses."""
    d, _lib, ctx = dbm
    rs = np.random.RandomState([N, int(scale)])
    real = (rs.normal(size=(N, 1)) * scale).astype(np.float32)
    fake = (rs.normal(size=(N, 1)) * scale).astype(np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for name, t_rf, t_fr in (("constant", np.ones((N, 1)), np.zeros((N, 1))),
                             ("mixed", rs.randint(0, 2, (N, 1)), rs.randint(0, 2, (N, 1))),
                             ("ignored", rs.randint(-1, 2, (N, 1)), rs.randint(-1, 2, (N, 1)))):
        t_rf, t_fr = np.ascontiguousarray(t_rf, np.int32), np.ascontiguousarray(t_fr, np.int32)
        out, gr, gf = np.full(2, np.nan, np.float32), np.full(N, np.nan, np.float32), np.full(N, np.nan, np.float32)
        ctx.call("dbm_discriminator_loss_t", p(real), p(fake), N, p(t_rf), p(t_fr), p(out), p(gr), p(gf), 0)
        r6, f6 = real.astype(np.float64), fake.astype(np.float64)
        ref = float(otrain.calculate_discriminator_loss(r6, f6, t_rf, t_fr))
        gr_ref, gf_ref = otrain.calculate_discriminator_loss_backward(r6, f6, t_rf, t_fr)
        correct = int((real >= 0).sum() + (fake < 0).sum())   # F.binary_accuracy on [real; fake] against [1; 0]
        acc_ref = float(ops.binary_accuracy(np.concatenate([r6, f6]), np.concatenate([np.ones((N, 1), np.int32), np.zeros((N, 1), np.int32)])))
        eg, ef = np.abs(gr - gr_ref.ravel()).max(), np.abs(gf - gf_ref.ravel()).max()
        print(f"LOSS N {N:3d} scale {scale:4.1f} {name:8s} loss {out[0]:.7g} ref {ref:.7g} d {abs(float(out[0]) - ref):.2e} "
              f"allowed {2e-6 * max(1.0, abs(ref)):.2e} g_real {eg:.2e} g_fake {ef:.2e} acc {out[1]:.6f}")
        assert abs(float(out[0]) - ref) < 2e-6 * max(1.0, abs(ref)), (name, float(out[0]), ref)
        assert eg < 1e-7 and ef < 1e-7, (name, eg, ef)
        assert abs(acc_ref - correct / (2.0 * N)) < 1e-12
        assert out[1] == np.float32(correct / (2.0 * N)), (name, out[1], correct)


# ------------------------------------------------------------------------------------------------------------------------
# Adam on a whole discriminator arena: bias correction, grad_scale, every round of the grid-stride loop
# ------------------------------------------------------------------------------------------------------------------------
def test_adam_three_steps_on_the_discriminator_arena(dbm):
    """dbm_adam_setup(1e-3, 0.9, 0.999, 1e-7), three updates with grad_scale 1, 0.5, 0.25 on gradients written into the
    gradient arena (N(0, s), s per tensor from {1e-6, 1e-3, 1}; one tensor zero in all three steps, as the biases in front of
    a BatchNorm are), against ops.adam_update in float64.  Per element: 4 * 2^-24 * max(|p0|, |p_ref|) -- three roundings of
    p -- plus 1e-5 * sum_t |step_t| -- an 8-operation float32 chain with 20 x margin.  The zero-gradient tensor stays
    bitwise.  The arena (10.4 M floats) is twenty rounds of the kernel's 2048 x 256 grid-stride loop."""
    d, _lib, ctx = dbm
    np.random.seed(5)
    m = d.DiscriminatorModel()
    spans, off = [], 0
    for name, t in m._tensors.items():   # parameter tensors lie in the arenas contiguously, in tensor order
        if t.kind == 0:
            spans.append((name, off, off + t.size))
            off += t.size
    params, grads = m.param_arena(), m.grad_arena()
    n = params.size
    assert n == off == grads.size and n > 2 * 2048 * 256
    rs = np.random.RandomState(77)
    p0 = rs.normal(0, 0.05, n).astype(np.float32)
    ctx.upload(params.ptr, p0)
    m.mark_params_changed()
    biases = [s for s in spans if s[0].endswith("/b")]
    zname, z0, z1 = biases[len(biases) // 2]
    assert same_bytes(m._tensors[zname].array.ravel(), p0[z0:z1])   # (the spans are the arena's)
    scales = np.empty(n, np.float32)
    for _, a, b in spans:
        scales[a:b] = rs.choice([1e-6, 1e-3, 1.0])
    scales[z0:z1] = 0.0
    alpha, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-7
    _lib.check(_lib.lib().dbm_adam_setup(m._h, alpha, b1, b2, eps), ctx.handle)
    p_ref, m_ref, v_ref = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    moved = np.zeros(n)
    for t, gs in enumerate((1.0, 0.5, 0.25), start=1):
        g = (rs.normal(size=n).astype(np.float32) * scales).astype(np.float32)
        ctx.upload(grads.ptr, g)
        _lib.check(_lib.lib().dbm_adam_update(m._h, gs), ctx.handle)
        before = p_ref.copy()
        ops.adam_update(p_ref, g.astype(np.float64) * gs, m_ref, v_ref, t, alpha, b1, b2, eps)
        moved += np.abs(p_ref - before)
    ctx.synchronize()
    got = ctx.download(params.ptr, np.float32, (n,))
    err = np.abs(got.astype(np.float64) - p_ref)
    bound = 4 * EPS24 * np.maximum(np.abs(p0), np.abs(p_ref)) + 1e-5 * moved
    worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"ADAM n {n} zero tensor {zname} worst err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f} at {worst}: err {err[worst]:.3e} "
          f"bound {bound[worst]:.3e}; per scale " + " ".join(f"{s:g}: {np.max((err / np.maximum(bound, 1e-300))[scales == np.float32(s)]):.3f}"
                                                           for s in (1e-6, 1e-3, 1.0)))
    assert same_bytes(got[z0:z1], p0[z0:z1]), "the zero-gradient tensor moved"
    assert np.all(err <= bound), (worst, err[worst], bound[worst])
    assert moved[scales > 0].min() > 0 and np.median(moved[scales > 0]) > 1e-3   # (every other element moved: about alpha per step)
