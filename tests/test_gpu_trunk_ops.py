"""-m gpu: the persistent trunk kernels (trunk_fused.hip: the RRDB trunk forward in its three forms; trunk_fused_bwd.hip: the
data-gradient chain) at op level, block by block, against the float64 restatement of tests/trunk_restatement.py (proven against
oracle/model.py by tests/test_trunk_host.py).

dbm_op_trunk_forward / dbm_op_trunk_backward run the models' own path (pack kernels, Generator's launch loops, persist_begin / _end,
the context's error words) on one inbox that lives as long as the process, and report per launch the form that ran and its grid.
Every call's report is asserted (`expected_reports`): a moved threshold takes coverage away loudly.

What is compared -- teacher-forced, so that the tolerance does not grow with depth and a fault in block 7 shows in block 7:
  forward with keep   layer k of block j against the float64 convolution of the kernel's OWN cat[j][:, :64 + 32 k]; cat[j + 1][:, :64]
                      against a5 * rs + a0 [* rs + the RRDB's input] of the kernel's own cat[j] (and cat[j - 2])
  backward            dA[j], all 192 channels, against the float64 block backward of the kernel's own dA[j + 1][:, :64] (the top block
                      of the first launch: gin); the skip operand is the kernel's own as well
EVERY element against its own L1 mass (trunk_restatement), never against a tensor maximum.  The backward's LeakyReLU masks are
operands (arbitrary cat[j] arrays with exact +0.0 and -0.0 cells): no exclusions.  Rows 5 and 22 and columns 9, 50, 77, 110, 150, 180 of
every weight tensor and channels 5, 9, 22, 50 of x / gin / g_a3 are 1e-3 of the others: a tensor maximum would hide them.
Forms that store no intermediates: the plain form's `out` without keep is bitwise cat[nrdb][:, :64] of the keep run; so is the
helper form's against ITS keep run, and it is compared with the float64 chain end to end as well (tensor-maximum normalisation is
accepted for that one figure: it is the only one that is not teacher-forced, and a per-element mass nine blocks deep bounds nothing).
Sentinels (a NaN with a payload, compared bitwise): cat[0][:, 64:] on entry (overwritten under keep; without keep `in` comes back
unchanged), cat[nrdb][:, 64:], out[:, 64:], every image outside a launch that runs alone, every dA[j] outside the launches, channels
64..191 of a 192-strided gin (they are NaN: reading one poisons the result).

Tolerance, not taken from the kernels: per quantity 16 x the worst deviation of the FLOAT32 restatement from the float64 one over
TOL_TABLE in the same (teacher-forced, per-element mass) normalisation, floor 8 * 2^-24, cap 1e-4, computed at run time.

Figures of the run on an MI355X (gfx950) that accompanied this file (the tolerances are computed at run time; these are theirs):
  quantity                      float32 restatement's worst   tolerance   kernels' worst per form
  layer outputs (|d| / mass)          2.35e-07               3.76e-06    tp27 1.27e-07, tp27 + helper 1.27e-07, tp32 1.20e-07
  block outputs (|d| / mass)          1.72e-07               2.75e-06    tp27 1.10e-07, tp27 + helper 1.18e-07, tp32 1.22e-07
  dA (|d| / mass)                     1.88e-07               3.01e-06    chain 2.41e-07
  helper form without keep, end to end (tensor maximum): float32 chain's worst 5.8e-08 .. 1.16e-07 per case, tolerances 9.3e-07 ..
  1.85e-06, the kernel's worst 1.04e-07
No form needs more than the 16 x margin: the worst kernel figure (the chain's) is 1.3 x the float32 restatement's own.  An image of a
batch equals the image alone bit for bit in all three forms, tiles of 32 included: a tile's position decides in which MFMA column and
workgroup an element is summed, not in which order.
The module takes 18 s there (43 cases; the slowest, 2.1 s, is helper-n17 with its 153 float64 reference blocks and two float64 / float32
chains); nearly all of it is the CPU's float64 reference.

Mutations tried on a scratch copy, one at a time, none committed (cases of THIS module that failed | test_fused_trunk_forward_backward_parity,
three shapes, and test_fused_trunk_matches_layerwise_path of test_gpu_model.py):
  1 halo_ptr's destination one column to the right        every backward case (17: geometry x 12, alone, regrouping, one inbox, wrap,
                                                          depth)                                              | parity 3 of 3 fail
  2 `fin0` of conv_layer4's data gradient 128 -> 112      the same 17                                         | parity 3 of 3 fail
  3 `maskv[r] >= 0.f` -> `> 0.f`                          the same 17 (the exact zeros in the masks)          | ALL FOUR PASS
  4 `rs * rs` -> `rs` for the third block                 the same 17                                         | parity 3 of 3 fail
  5 `8 - tap` -> `tap` in pack_trunk_fused_bwd_kernel     the same 17                                         | parity 3 of 3 fail
  6 skip registers not updated at a first block           the 7 whose launches span two RRDBs or more (n1-one, n8-two, n9-one, n11-chunks,
                                                          alone, regrouping, depth); one launch per RRDB passes, as it must: a launch
                                                          takes its skip from its own gin             | parity fails with 2 and 3 RRDBs
  7 forward: halo slot (after, 3) never fetched           all 18 forward-form cases, alone, tp32's image-alone case, one inbox, wrap,
                                                          depth (23)                                          | all four fail
  8 forward, helper form: a band takes the helper's       the 6 helper cases, alone, one inbox, wrap (9)      | layerwise A/B fails,
    channels 32..63 from the neighbouring wavefront's quad                                                      parity 3 of 3 PASS
(8 stands in for "the helper's channels from the wrong parity": the granule's tag names its layer, so a read from the other parity is a
wait for a tag that never comes, not a wrong value -- by the code; it was not run.  2 moves fin0 down: moved up, the sixteen channels in
between would never be published and their readers would wait.)
"""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest

from oracle import model as omodel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import trunk_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_CAP = 1e-4
TOL_FLOOR = 8 * 2.0 ** -24
MARGIN = 16.0
SENT = 0x7FC00ABC                      # the sentinel: a quiet NaN with a payload
QUIET_ROWS, QUIET_COLS, QUIET_DATA = (5, 22), (9, 50, 77, 110, 150, 180), (5, 9, 22, 50)
FORMS = {"tp27": (27, 0, 0), "tp27_helper": (27, 1, 1), "tp32": (32, 0, 2)}   # tile, helper, report code
CHAIN = 3
WORST = {}                             # (quantity, form) -> worst |d| / mass seen in this run (printed by the last test)


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    ctx = _lib.default_context()
    return d, _lib, ctx


# ------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(nrdb, N, seed=0):
    """He-initialised weights scaled by 1.5 with non-zero biases (as scaled_oracle_generator(..., 1.5) of test_gpu_model.py), x / gin /
    g_a3 ~ N(0, 1), mask arrays ~ N(0, 1) with exact zeros of both signs; quiet rows, columns and channels (module docstring)."""
    r = np.random.RandomState(1000 * nrdb + 10 * N + seed)
    W, b = [], []
    for i in range(nrdb * 5):
        k = i % 5
        w = omodel.he_normal(r, (32 if k < 4 else 64, 64 + 32 * k, 3, 3)) * np.float32(1.5)
        bias = r.normal(0, 0.1, (w.shape[0],)).astype(np.float32)
        for q in QUIET_ROWS:
            w[q] *= np.float32(1e-3)
            bias[q] *= np.float32(1e-3)
        for q in QUIET_COLS:
            if q < w.shape[1]:
                w[:, q] *= np.float32(1e-3)
        W.append(np.ascontiguousarray(w))
        b.append(bias)

    def data():
        a = r.normal(0, 1, (N, 64, 9, 9)).astype(np.float32)
        a[:, QUIET_DATA] *= np.float32(1e-3)
        return a

    masks = []
    for _ in range(nrdb):
        m = r.normal(0, 1, (N, 192, 9, 9)).astype(np.float32)
        u = r.rand(*m.shape)
        m[u < 0.02] = 0.0
        m[u > 0.995] = -0.0
        masks.append(m)
    P = types.SimpleNamespace(nrdb=nrdb, N=N, W=W, b=b, x=data(), gin=data(), g_a3=data(), masks=masks)
    P.W64 = [w.astype(np.float64) for w in W]
    P.b64 = [v.astype(np.float64) for v in b]
    return P


def f64(a):
    return np.asarray(a, dtype=np.float64)


def rs64(rs):
    return float(np.float32(rs))      # the kernels' operand is the float32 value


# ------------------------------------------------------------------------------------------------------------------------
# tolerances: the float32 restatement against the float64 one, teacher-forced on the float32 chain's own buffers
# ------------------------------------------------------------------------------------------------------------------------
TOL_TABLE = ((9, 8, 0.1), (3, 7, 0.3))


def clamp_tol(worst):
    return min(max(MARGIN * worst, TOL_FLOOR), TOL_CAP)


@functools.lru_cache(maxsize=None)
def tolerances():
    worst = {"layer": 0.0, "out": 0.0, "dA": 0.0}
    for nrdb, N, rs in TOL_TABLE:
        P = problem(nrdb, N)
        cat32, _ = tr.trunk_forward(P.x, P.W, P.b, np.float32(rs))
        for j in range(nrdb):
            sl = slice(5 * j, 5 * j + 5)
            xin32 = cat32[j - 2][:, :64] if j % 3 == 2 else None
            a32, o32, _, _ = tr.dense_block_forward(cat32[j][:, :64], P.W[sl], P.b[sl], np.float32(rs), j % 3 == 2, xin32, forced=cat32[j])
            a64, o64, ma, mo = tr.dense_block_forward(f64(cat32[j][:, :64]), P.W64[sl], P.b64[sl], rs64(rs), j % 3 == 2,
                                                      None if xin32 is None else f64(xin32), forced=f64(cat32[j]))
            for k in range(4):
                worst["layer"] = max(worst["layer"], float((np.abs(a32[k] - a64[k]) / ma[k]).max()))
            worst["out"] = max(worst["out"], float((np.abs(o32 - o64) / mo).max()))
        dA32, _ = tr.trunk_backward(P.gin, P.masks, P.W, np.float32(rs), P.g_a3)
        for j in range(nrdb):
            g = P.gin if j == nrdb - 1 else dA32[j + 1][:, :64]
            skip = None
            if j % 3 == 0:
                skip = P.gin if j + 3 == nrdb else dA32[j + 3][:, :64]
            D, M = tr.dense_block_backward(f64(g), f64(P.masks[j]), P.W64[5 * j:5 * j + 5], rs64(rs), j % 3,
                                           None if skip is None else f64(skip), f64(P.g_a3) if j == 0 else None)
            worst["dA"] = max(worst["dA"], float((np.abs(dA32[j] - D) / M).max()))
    return worst, {k: clamp_tol(v) for k, v in worst.items()}


@functools.lru_cache(maxsize=None)
def chain_reference(nrdb, N, rs):
    """float64 chain from x, and the end-to-end tolerance (tensor-maximum normalisation) from the float32 chain's deviation"""
    P = problem(nrdb, N)
    c64, _ = tr.trunk_forward(f64(P.x), P.W64, P.b64, rs64(rs))
    c32, _ = tr.trunk_forward(P.x, P.W, P.b, np.float32(rs))
    ref = c64[nrdb][:, :64]
    worst = float(np.abs(c32[nrdb][:, :64] - ref).max() / np.abs(ref).max())
    return ref, worst, clamp_tol(worst)


# ------------------------------------------------------------------------------------------------------------------------
# the two ops
# ------------------------------------------------------------------------------------------------------------------------
def sentinel(shape):
    a = np.empty(shape, dtype=np.float32)
    a.view(np.uint32)[...] = SENT
    return a


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENT).all())


def same_bits(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def table(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def chunks(N, ipl, only):
    return [(i0, min(ipl, N - i0)) for c, i0 in enumerate(range(0, N, ipl)) if only < 0 or c == only]


def expected_reports(code, N, ipl, only, ngroups=1):
    reps = []
    for _ in range(ngroups):
        for _, nimg in chunks(N, ipl, only):
            cl = (nimg + 7) // 8
            grid = {0: 24 * cl, 1: 32 * cl, 2: 8 * (((nimg * 81 + 31) // 32 + 7) // 8), CHAIN: 24 * cl}[code]
            reps.append((code, grid))
    return reps


def read_report(report):
    return [(report[1 + 2 * i], report[2 + 2 * i]) for i in range(report[0])]


def run_forward(dbm, P, rs, form, keep, imgs=None, ipl=None, only=-1, epoch0=-1, agent=0, ctx=None):
    """One dbm_op_trunk_forward call on sentinel-filled buffers: (cat list, out or None), every buffer (N, 192, 9, 9); ctx: the context
    to run on instead of the default one"""
    _, _lib, ctx = dbm if ctx is None else (dbm[0], dbm[1], ctx)
    x = P.x if imgs is None else P.x[imgs]
    N = len(x)
    ipl = N if ipl is None else ipl
    tile, helper, code = FORMS[form]
    cat = [sentinel((N, 192, 9, 9)) for _ in range(P.nrdb + 1 if keep else 1)]
    cat[0][:, :64] = x
    entry = cat[0].copy()
    out = None if keep else sentinel((N, 192, 9, 9))
    a = _lib.TrunkForward()
    a.nrdb, a.N, a.rs, a.imgs_per_launch, a.only_launch, a.epoch0 = P.nrdb, N, rs, ipl, only, epoch0
    a.keep, a.tile, a.helper, a.agent_stores = int(keep), tile, helper, agent
    tw, tb, tc = table(P.W), table(P.b), table(cat)
    a.w, a.b, a.cat = C.cast(tw, _lib.c_void_pp), C.cast(tb, _lib.c_void_pp), C.cast(tc, _lib.c_void_pp)
    a.out = None if keep else out.ctypes.data
    report = (C.c_int * 129)()
    ctx.synchronize()
    _lib.check(_lib.lib().dbm_op_trunk_forward(ctx.handle, C.byref(a), report, 129), ctx.handle)
    ctx.synchronize()
    assert read_report(report) == expected_reports(code, N, ipl, only), (form, N, ipl, read_report(report))
    # what every forward must leave alone
    assert same_bits(cat[0][:, :64], entry[:, :64])
    live = np.zeros(N, dtype=bool)
    for i0, n in chunks(N, ipl, only):
        live[i0:i0 + n] = True
    if keep:
        assert untouched(cat[P.nrdb][:, 64:])
        for j in range(P.nrdb + 1):
            assert untouched(cat[j][~live][:, 0 if j else 64:]), f"cat[{j}]: an image outside the launch was written"
        assert not np.isnan(np.stack([c[live] for c in cat[:P.nrdb]])).any() and not np.isnan(cat[P.nrdb][live][:, :64]).any()
    else:
        assert same_bits(cat[0], entry), "`in` changed without keep"
        assert untouched(out[:, 64:]) and untouched(out[~live])
        assert not np.isnan(out[live][:, :64]).any()
    return cat, out


def run_backward(dbm, P, rs, launches, imgs=None, ipl=None, only=-1, epoch0=-1, agent=0, gin192=False):
    """One dbm_op_trunk_backward call on sentinel-filled dA buffers: the list of dA[j] (N, 192, 9, 9)"""
    _, _lib, ctx = dbm
    sl = slice(None) if imgs is None else imgs
    gin64, g_a3 = np.ascontiguousarray(P.gin[sl]), np.ascontiguousarray(P.g_a3[sl])
    masks = [np.ascontiguousarray(m[sl]) for m in P.masks]
    N = len(gin64)
    ipl = N if ipl is None else ipl
    gin = gin64
    if gin192:
        gin = sentinel((N, 192, 9, 9))
        gin[:, :64] = gin64
    dA = [sentinel((N, 192, 9, 9)) for _ in range(P.nrdb)]
    a = _lib.TrunkBackward()
    a.nrdb, a.N, a.rs, a.imgs_per_launch, a.only_launch, a.epoch0, a.agent_stores = P.nrdb, N, rs, ipl, only, epoch0, agent
    a.nlaunch = len(launches)
    j0 = (C.c_int * len(launches))(*[l[0] for l in launches])
    j1 = (C.c_int * len(launches))(*[l[1] for l in launches])
    a.j0, a.j1 = j0, j1
    tw, tc, td = table(P.W), table(masks), table(dA)
    a.w, a.cat, a.dA = C.cast(tw, _lib.c_void_pp), C.cast(tc, _lib.c_void_pp), C.cast(td, _lib.c_void_pp)
    a.gin, a.gin_sn, a.g_a3 = gin.ctypes.data, (192 if gin192 else 64) * 81, g_a3.ctypes.data
    report = (C.c_int * 129)()
    ctx.synchronize()
    _lib.check(_lib.lib().dbm_op_trunk_backward(ctx.handle, C.byref(a), report, 129), ctx.handle)
    ctx.synchronize()
    assert read_report(report) == expected_reports(CHAIN, N, ipl, only, len(launches)), (launches, N, ipl, read_report(report))
    live = np.zeros(N, dtype=bool)
    for i0, n in chunks(N, ipl, only):
        live[i0:i0 + n] = True
    covered = set(j for lo, hi in launches for j in range(lo, hi))
    for j in range(P.nrdb):
        if j in covered:
            assert untouched(dA[j][~live]), f"dA[{j}]: an image outside the launch was written"
            assert not np.isnan(dA[j][live]).any(), f"dA[{j}] holds NaN: a sentinel was read, or a cell was not written"
        else:
            assert untouched(dA[j]), f"dA[{j}] lies outside the launches and was written"
    return dA


def note(quantity, form, worst):
    WORST[(quantity, form)] = max(WORST.get((quantity, form), 0.0), worst)


def check_forward(cat, P, rs, form, imgs=slice(None), src=slice(None)):
    """the teacher-forced comparison of a keep run; imgs: the images of `cat` that a launch covered"""
    _, tol = tolerances()
    for j in range(P.nrdb):
        forced = f64(cat[j][imgs])
        xin = f64(cat[j - 2][imgs][:, :64]) if j % 3 == 2 else None
        a, out, ma, mo = tr.dense_block_forward(forced[:, :64], P.W64[5 * j:5 * j + 5], P.b64[5 * j:5 * j + 5], rs64(rs), j % 3 == 2, xin,
                                                forced=forced)
        for k in range(4):
            d = float((np.abs(forced[:, 64 + 32 * k:96 + 32 * k] - a[k]) / ma[k]).max())
            note("layer", form, d)
            assert d <= tol["layer"], f"{form}: block {j} conv_layer{k + 1}: |d| / mass {d:.3g} > {tol['layer']:.3g}"
        d = float((np.abs(f64(cat[j + 1][imgs][:, :64]) - out) / mo).max())
        note("out", form, d)
        assert d <= tol["out"], f"{form}: block {j} output: |d| / mass {d:.3g} > {tol['out']:.3g}"


def check_backward(dA, P, rs, launches, imgs=slice(None), src=slice(None)):
    """the teacher-forced comparison of a chain; imgs: the images of dA a launch covered, src: the same images of the problem"""
    _, tol = tolerances()
    top = launches[0][1]
    gin = f64(P.gin[src])

    def gsrc(j):
        return gin if j == top else f64(dA[j][imgs][:, :64])

    for lo, hi in launches:
        for j in range(hi - 1, lo - 1, -1):
            D, M = tr.dense_block_backward(gsrc(j + 1), f64(P.masks[j][src]), P.W64[5 * j:5 * j + 5], rs64(rs), j % 3,
                                           gsrc(j + 3) if j % 3 == 0 else None, f64(P.g_a3[src]) if j == 0 else None)
            r = np.abs(f64(dA[j][imgs]) - D) / M
            d = float(r.max())
            note("dA", "chain", d)
            where = np.unravel_index(int(r.argmax()), r.shape)
            assert d <= tol["dA"], f"chain {launches}: dA[{j}] at (image, channel, row, column) {where}: |d| / mass {d:.3g} > {tol['dA']:.3g}"


# ------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------
ONE, THREE, TWO = ((0, 9),), ((6, 9), (3, 6), (0, 3)), ((3, 9), (0, 3))
# id -> nrdb, N, launches, imgs_per_launch, rs, agent-scope stores, 192-strided gin
BWD_CASES = {
    "n1-one": (9, 1, ONE, None, 0.1, 0, False),
    "n7-three": (9, 7, THREE, None, 0.3, 1, True),
    "n8-two": (9, 8, TWO, None, 0.1, 0, True),
    "n9-one": (9, 9, ONE, None, 0.3, 1, False),
    "n17-three": (9, 17, THREE, None, 0.1, 0, False),
    "n11-chunks": (9, 11, TWO, 8, 0.1, 0, True),          # img0 = 8, nimg = 3
    "top-only": (9, 7, ((6, 9),), None, 0.1, 0, False),   # dA[0..5] stay as they were
    "r3-n1": (3, 1, ((0, 3),), None, 0.3, 1, True),
    "r3-n7": (3, 7, ((0, 3),), None, 0.1, 0, False),
    "r3-n8": (3, 8, ((0, 3),), None, 0.3, 0, True),
    "r3-n9": (3, 9, ((0, 3),), None, 0.1, 1, False),
    "r3-n17": (3, 17, ((0, 3),), None, 0.3, 0, False),
}


@pytest.mark.parametrize("cid", sorted(BWD_CASES))
def test_backward_geometry(dbm, cid):
    nrdb, N, launches, ipl, rs, agent, gin192 = BWD_CASES[cid]
    P = problem(nrdb, N)
    dA = run_backward(dbm, P, rs, launches, ipl=ipl, agent=agent, gin192=gin192)
    check_backward(dA, P, rs, launches)


def test_backward_launch_alone_leaves_the_other_images(dbm):
    P = problem(9, 11)
    dA = run_backward(dbm, P, 0.1, TWO, ipl=8, only=1)     # (run_backward asserts images 0..7 untouched)
    check_backward(dA, P, 0.1, TWO, imgs=slice(8, 11), src=slice(8, 11))


def test_backward_regrouping_and_rechunking_are_bitwise(dbm):
    """the chain has no atomics and no split-K: every launch list, chunking and store scope of one problem gives the same bits"""
    P = problem(9, 9)
    base = run_backward(dbm, P, 0.1, ONE)
    check_backward(base, P, 0.1, ONE)
    for launches, ipl, agent, gin192 in ((THREE, None, 0, False), (TWO, None, 1, True), (ONE, 8, 0, True), (THREE, 4, 1, False),
                                          (TWO, 1, 0, False), (ONE, None, 0, False)):
        dA = run_backward(dbm, P, 0.1, launches, ipl=ipl, agent=agent, gin192=gin192)
        for j in range(9):
            assert same_bits(dA[j], base[j]), (launches, ipl, agent, j)


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
# id -> form, nrdb, N, imgs_per_launch, rs, agent-scope stores
FWD_CASES = {}
for _n, _rs, _agent in ((1, 0.1, 0), (7, 0.3, 1), (8, 0.1, 0), (9, 0.3, 0), (17, 0.1, 1)):
    FWD_CASES[f"tp27-n{_n}"] = ("tp27", 9, _n, None, _rs, _agent)
    FWD_CASES[f"helper-n{_n}"] = ("tp27_helper", 9, _n, None, _rs, _agent)
for _n, _rs, _agent in ((1, 0.3, 0), (2, 0.1, 1), (5, 0.3, 0), (9, 0.1, 0)):
    FWD_CASES[f"tp32-n{_n}"] = ("tp32", 9, _n, None, _rs, _agent)
FWD_CASES["tp27-n11-chunks"] = ("tp27", 9, 11, 8, 0.1, 0)
FWD_CASES["helper-n11-chunks"] = ("tp27_helper", 3, 11, 8, 0.3, 0)
FWD_CASES["tp32-n11-chunks"] = ("tp32", 3, 11, 8, 0.1, 1)
FWD_CASES["tp27-r3-n17"] = ("tp27", 3, 17, None, 0.3, 0)


@pytest.mark.parametrize("cid", sorted(FWD_CASES))
def test_forward_forms(dbm, cid):
    form, nrdb, N, ipl, rs, agent = FWD_CASES[cid]
    P = problem(nrdb, N)
    cat, _ = run_forward(dbm, P, rs, form, True, ipl=ipl, agent=agent)
    check_forward(cat, P, rs, form)
    # without keep: the same arithmetic, only `out` is stored
    _, out = run_forward(dbm, P, rs, form, False, ipl=ipl, agent=agent)
    assert same_bits(out[:, :64], cat[nrdb][:, :64]), f"{form}: `out` without keep differs from cat[nrdb] with keep"
    if form == "tp27_helper":  # ... and the one form nothing else sees without stored intermediates, end to end
        ref, _, tol = chain_reference(nrdb, N, rs)
        d = float(np.abs(f64(out[:, :64]) - ref).max() / np.abs(ref).max())
        note("end to end (tensor max)", form, d)
        assert d <= tol, f"helper form without keep, end to end: {d:.3g} > {tol:.3g}"


def test_forward_launch_alone_leaves_the_other_images(dbm):
    P = problem(3, 11)
    for form in FORMS:
        cat, _ = run_forward(dbm, P, 0.1, form, True, ipl=8, only=1)   # (run_forward asserts images 0..7 untouched)
        check_forward(cat, P, 0.1, form, imgs=slice(8, 11))
        run_forward(dbm, P, 0.1, form, False, ipl=8, only=0)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_forward_image_of_a_batch_equals_the_image_alone(dbm, form):
    """tiles of 27 never cross an image; tiles of 32 do, but every output element is the same sum in the same order wherever its
    column lies: bitwise in all three forms"""
    P = problem(3, 5)
    cat, _ = run_forward(dbm, P, 0.3, form, True)
    for i in range(5):
        one, _ = run_forward(dbm, P, 0.3, form, True, imgs=slice(i, i + 1))
        for j in range(4):
            hi = 64 if j == 3 else 192
            assert same_bits(one[j][:, :hi], cat[j][i:i + 1, :hi]), (form, i, j)


def test_repeat_is_bitwise(dbm):
    P = problem(3, 9)
    for form in FORMS:
        for keep in (True, False):
            a = run_forward(dbm, P, 0.1, form, keep)
            b = run_forward(dbm, P, 0.1, form, keep)
            if keep:
                assert all(same_bits(u, v) for u, v in zip(a[0], b[0])), form
            else:
                assert same_bits(a[1], b[1]), form
    a = run_backward(dbm, P, 0.1, ((0, 3),))
    b = run_backward(dbm, P, 0.1, ((0, 3),))
    assert all(same_bits(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------
# the inbox over time
# ------------------------------------------------------------------------------------------------------------------------
def test_one_inbox_launches_of_varying_size(dbm):
    """sizes 8, 3, 8, 1 in succession on different data, forward and backward interleaved, on the one inbox: a launch meets the
    granules of larger and smaller launches of both directions and of every form"""
    for k, (N, form) in enumerate(((8, "tp27"), (3, "tp27_helper"), (8, "tp32"), (1, "tp27_helper"))):
        P = problem(3, N, seed=1 + k)
        cat, _ = run_forward(dbm, P, 0.1, form, True)
        check_forward(cat, P, 0.1, form)
        dA = run_backward(dbm, P, 0.1, ((0, 3),))
        check_backward(dA, P, 0.1, ((0, 3),))


def test_epoch_wrap(dbm):
    """consecutive launches with epochs 0xFFFFE, 0xFFFFF, 0x100000, 0x100001 on the used inbox (the kernels keep 20 bits: the tags
    fall back to 0 and 1), forward and backward in turn, then the op's counter goes on from there"""
    P = problem(3, 8, seed=7)
    run_backward(dbm, P, 0.1, ((0, 3),))                       # (the inbox has been used, whatever ran before)
    epoch = 0xFFFFE
    for form in ("tp27", "tp27_helper"):
        cat, _ = run_forward(dbm, P, 0.1, form, True, epoch0=epoch)
        check_forward(cat, P, 0.1, form)
        dA = run_backward(dbm, P, 0.1, ((0, 3),), epoch0=epoch + 1)
        check_backward(dA, P, 0.1, ((0, 3),))
        epoch += 2
    cat, _ = run_forward(dbm, P, 0.1, "tp32", True)
    check_forward(cat, P, 0.1, "tp32")
    dA = run_backward(dbm, problem(3, 9), 0.1, ((0, 3),), ipl=1)   # nine launches further
    check_backward(dA, problem(3, 9), 0.1, ((0, 3),))


# ------------------------------------------------------------------------------------------------------------------------
# the depth limit
# ------------------------------------------------------------------------------------------------------------------------
def test_depth_limit_forward(dbm):
    """nrdb = 63: the last value TRUNK_FUSED_MAXCAT admits, the last slot of the pointer tables, the highest layer serials"""
    P = problem(63, 1)
    cat, _ = run_forward(dbm, P, 0.1, "tp27", True)
    check_forward(cat, P, 0.1, "tp27")


def test_depth_limit_backward(dbm):
    P = problem(63, 1)
    dA = run_backward(dbm, P, 0.1, ((0, 63),))
    check_backward(dA, P, 0.1, ((0, 63),))


def test_one_rrdb_too_many_is_refused(dbm):
    _, _lib, ctx = dbm
    P = problem(63, 1)
    Q = types.SimpleNamespace(**vars(P))
    Q.nrdb, Q.W, Q.b, Q.masks = 66, P.W + P.W[:15], P.b + P.b[:15], P.masks + P.masks[:3]
    with pytest.raises(_lib.DbmError, match="too many dense blocks") as e:
        run_forward(dbm, Q, 0.1, "tp27", True)
    assert e.value.code == 1
    with pytest.raises(_lib.DbmError, match="too many dense blocks") as e:
        run_backward(dbm, Q, 0.1, ((0, 66),))
    assert e.value.code == 1
    ctx.check_timeout()


def test_zz_figures():
    """prints what the run measured (pytest -s): the float32 restatement's worst, the tolerances, the kernels' worst per form"""
    worst, tol = tolerances()
    for k in sorted(worst):
        print(f"\n  {k:8s} float32 restatement's worst {worst[k]:.3g}   tolerance {tol[k]:.3g}", end="")
    for (q, form), v in sorted(WORST.items()):
        print(f"\n  kernels' worst  {q:26s} {form:12s} {v:.3g}", end="")
    for nrdb, N, rs in sorted(set((c[1], c[2], c[4]) for c in FWD_CASES.values() if c[0] == "tp27_helper")):
        _, w, t = chain_reference(nrdb, N, rs)
        print(f"\n  end to end nrdb {nrdb} N {N} rs {rs}: float32 chain's worst {w:.3g}   tolerance {t:.3g}", end="")
    print()
