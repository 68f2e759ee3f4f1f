"""Seeded op-level cases of the three kernels on the generator's own path in the training step (wgrad_wave_dma_kernel, trunk_fused_bwd_kernel,
deform_csr_gather_kernel), shared by tools/record_parent_bits.py (which records what a library computes) and
tests/test_gpu_exposed_kernels_bitwise.py (which compares a library with the record).  Not a test module.

Every run_* function yields (key, outputs, extra): `outputs` is a dict of float32 arrays, `extra` whatever the float64 check of the
test needs.  summarise() turns an output into what the fixture keeps: a CRC-32 of its bytes and 128 evenly spaced values.
"""
import ctypes as C
import functools
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

SAMPLES = 128


def summarise(a):
    """(crc32 of the bytes, SAMPLES evenly spaced values) of a float32 array: the CRC pins every bit, the samples say where two libraries part"""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    idx = np.unique(np.linspace(0, a.size - 1, min(SAMPLES, a.size)).astype(np.int64))
    return np.uint32(zlib.crc32(a.tobytes())), a[idx].copy()


def load():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


def restore_deterministic(ctx):
    from deepbedmap_amd import srgan

    srgan._applied_deterministic[0] = None   # what srgan.apply_config sets, so that later modules see the default
    srgan.apply_config(ctx)


# ------------------------------------------------------------------------------------------------------------------------
# weight gradients: dbm_op_conv2d_wgrad_batch, 3x3 / stride 1 / pad 1
# ------------------------------------------------------------------------------------------------------------------------
CAT_BUF = 192   # channels of the concat buffer every x is a slice of


def _layer(H, W, C_in, O, c0, gb):
    return dict(H=H, W=W, C=C_in, O=O, c0=c0, gb=gb)


def wgrad_cases():
    """name -> (N, layers).  x of a layer: channels c0 .. c0 + C of an (N, 192, H, W) buffer (image stride 192 H W)."""
    cases = {}
    for N in (1, 3, 64):
        for C_in, O in ((32, 32), (96, 32), (192, 64), (64, 16)):
            for gb in (1, 0):
                # (a 192-channel layer fills the buffer: its offset is 0; every other slice starts at channel 32)
                cases[f"p9-n{N}-c{C_in}-o{O}-gb{gb}"] = (N, [_layer(9, 9, C_in, O, min(32, CAT_BUF - C_in), gb)])
    cases["dense-block-n8"] = (8, [_layer(9, 9, 64 + 32 * k, 32 if k < 4 else 64, 0, 1) for k in range(5)])
    cases["mixed-9x9-8x8-n3"] = (3, [_layer(9, 9, 64, 32, 32, 1), _layer(8, 8, 64, 32, 32, 1)])
    cases["p8x8-n3"] = (3, [_layer(8, 8, 64, 32, 32, 1)])
    cases["p9x10-n3"] = (3, [_layer(9, 10, 64, 32, 32, 1)])
    return cases


WGRAD_MODES = [(det, cleared) for det in (1, 0) for cleared in (0, 1)]


@functools.lru_cache(maxsize=4)
def wgrad_operands(name):
    N, layers = wgrad_cases()[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 2**31)
    ops = []
    for L in layers:
        x = rs.normal(size=(N, CAT_BUF, L["H"], L["W"])).astype(np.float32)
        dy = rs.normal(size=(N, L["O"], L["H"], L["W"])).astype(np.float32)
        gW0 = rs.normal(size=(L["O"], L["C"], 3, 3)).astype(np.float32)
        gb0 = rs.normal(size=(L["O"],)).astype(np.float32)
        for a in (x, dy, gW0, gb0):
            a.setflags(write=False)
        ops.append((x, dy, gW0, gb0))
    return N, layers, ops


def wgrad_reference(x, dy, L, scale):
    """float64 gW, gb and their L1 masses (sum of |terms|), for the bound of the test"""
    N = x.shape[0]
    H, W, C_in, c0 = L["H"], L["W"], L["C"], L["c0"]
    xs = np.zeros((N, C_in, H + 2, W + 2))
    xs[:, :, 1:-1, 1:-1] = x[:, c0:c0 + C_in]
    d = dy.astype(np.float64).transpose(1, 0, 2, 3).reshape(L["O"], -1)
    gW = np.empty((L["O"], C_in, 3, 3))
    mW = np.empty_like(gW)
    for t in range(9):
        xt = xs[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W].transpose(0, 2, 3, 1).reshape(-1, C_in)
        gW[:, :, t // 3, t % 3] = d @ xt
        mW[:, :, t // 3, t % 3] = np.abs(d) @ np.abs(xt)
    return scale * gW, scale * mW, scale * d.sum(1), scale * np.abs(d).sum(1)


WGRAD_SCALE = 0.5


def run_wgrad(dbm, name):
    """yields ((name, det, cleared), {gW<i>, gb<i>}, (cat, S)) for the four modes"""
    d, _lib, ctx = dbm
    N, layers, ops = wgrad_operands(name)
    n = len(layers)
    dev_x = [d.to_device(x.reshape(-1)) for x, _, _, _ in ops]
    dev_y = [d.to_device(dy.reshape(-1)) for _, dy, _, _ in ops]
    dev_W = [d.to_device(gW0) for _, _, gW0, _ in ops]
    dev_b = [d.to_device(gb0) for _, _, _, gb0 in ops]
    arr = (_lib.WgradDesc * n)()
    for i, L in enumerate(layers):
        a, plane = arr[i], L["H"] * L["W"]
        a.x, a.xsn = dev_x[i].ptr + 4 * L["c0"] * plane, CAT_BUF * plane
        a.dy, a.dysn = dev_y[i].ptr, L["O"] * plane
        a.N, a.C, a.H, a.W, a.O, a.k, a.stride, a.pad, a.ups = N, L["C"], L["H"], L["W"], L["O"], 3, 1, 1, 0
        a.scale = WGRAD_SCALE
        a.gW = dev_W[i].ptr
        a.gb = dev_b[i].ptr if L["gb"] else None
    try:
        for det, cleared in WGRAD_MODES:
            _lib.check(_lib.lib().dbm_set_deterministic(ctx.handle, det), ctx.handle)
            for i, (_, _, gW0, gb0) in enumerate(ops):
                dev_W[i].set(np.zeros_like(gW0) if cleared else gW0)
                dev_b[i].set(np.zeros_like(gb0) if cleared else gb0)
            cat, S = (C.c_int * n)(), (C.c_int * n)()
            _lib.check(_lib.lib().dbm_op_conv2d_wgrad_batch(ctx.handle, arr, n, int(cleared), cat, S), ctx.handle)
            ctx.synchronize()
            out = {}
            for i, L in enumerate(layers):
                out[f"gW{i}"] = dev_W[i].get()
                if L["gb"]:
                    out[f"gb{i}"] = dev_b[i].get()
            yield (name, det, cleared), out, (list(cat), list(S))
    finally:
        restore_deterministic(ctx)


def wgrad_is_bitwise(det, cleared, S):
    """Are the bits of this layer fixed?  Deterministic mode: always.  Atomic mode: the K slices of a layer add to the same words in
    any order -- one slice is always the same sum, two slices are when they add to zeros ((0 + a) + b == (0 + b) + a)."""
    return bool(det) or S == 1 or (S == 2 and bool(cleared))


# ------------------------------------------------------------------------------------------------------------------------
# the data-gradient chain: dbm_op_trunk_backward on the smallest geometry of tests/test_gpu_trunk_ops.py (three dense blocks = one RRDB)
# ------------------------------------------------------------------------------------------------------------------------
SENT = 0x7FC00ABC
# id -> nrdb (dense blocks), N, launches (j0, j1) from the top down, residual scale
CHAIN_CASES = {
    "rrdb1-n1": (3, 1, ((0, 3),), 0.3),
    "rrdb1-n2": (3, 2, ((0, 3),), 0.1),
    "rrdb1-n5": (3, 5, ((0, 3),), 0.3),
    "rrdb2-n1": (6, 1, ((0, 6),), 0.1),
    "rrdb2-n2": (6, 2, ((0, 6),), 0.3),
    "rrdb2-n5": (6, 5, ((0, 6),), 0.1),
    "rrdb2-n2-two-launches": (6, 2, ((3, 6), (0, 3)), 0.1),   # the first launch starts at j0 = 3
}


@functools.lru_cache(maxsize=None)
def chain_problem(nrdb, N):
    """He-initialised weights scaled by 1.5, gin / g_a3 ~ N(0, 1), mask arrays ~ N(0, 1) with exact zeros of both signs"""
    from oracle import model as omodel

    r = np.random.RandomState(7000 + 100 * nrdb + N)
    W = []
    for i in range(nrdb * 5):
        k = i % 5
        W.append(np.ascontiguousarray(omodel.he_normal(r, (32 if k < 4 else 64, 64 + 32 * k, 3, 3)) * np.float32(1.5)))
    masks = []
    for _ in range(nrdb):
        m = r.normal(0, 1, (N, 192, 9, 9)).astype(np.float32)
        u = r.rand(*m.shape)
        m[u < 0.02] = 0.0
        m[u > 0.995] = -0.0
        masks.append(m)
    gin = r.normal(0, 1, (N, 64, 9, 9)).astype(np.float32)
    g_a3 = r.normal(0, 1, (N, 64, 9, 9)).astype(np.float32)
    return types.SimpleNamespace(nrdb=nrdb, N=N, W=W, masks=masks, gin=gin, g_a3=g_a3, W64=[w.astype(np.float64) for w in W])


def _table(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def run_chain(dbm, cid):
    """-> (cid, {dA<j>}, problem): one dbm_op_trunk_backward call on sentinel-filled dA buffers (N, 192, 9, 9)"""
    _, _lib, ctx = dbm
    nrdb, N, launches, rs = CHAIN_CASES[cid]
    P = chain_problem(nrdb, N)
    dA = []
    for _ in range(nrdb):
        a = np.empty((N, 192, 9, 9), np.float32)
        a.view(np.uint32)[...] = SENT
        dA.append(a)
    a = _lib.TrunkBackward()
    a.nrdb, a.N, a.rs, a.imgs_per_launch, a.only_launch, a.epoch0, a.agent_stores = nrdb, N, rs, N, -1, -1, 0
    a.nlaunch = len(launches)
    j0 = (C.c_int * len(launches))(*[l[0] for l in launches])
    j1 = (C.c_int * len(launches))(*[l[1] for l in launches])
    a.j0, a.j1 = j0, j1
    tw, tc, td = _table(P.W), _table(P.masks), _table(dA)
    a.w, a.cat, a.dA = C.cast(tw, _lib.c_void_pp), C.cast(tc, _lib.c_void_pp), C.cast(td, _lib.c_void_pp)
    a.gin, a.gin_sn, a.g_a3 = P.gin.ctypes.data, 64 * 81, P.g_a3.ctypes.data
    report = (C.c_int * 129)()
    ctx.synchronize()
    _lib.check(_lib.lib().dbm_op_trunk_backward(ctx.handle, C.byref(a), report, 129), ctx.handle)
    ctx.synchronize()
    return cid, {f"dA{j}": dA[j] for j in range(nrdb)}, P


# ------------------------------------------------------------------------------------------------------------------------
# the stored-list gather: dbm_op_deform_conv2d_backward, C = 64, O = 64, deterministic mode (the default)
# ------------------------------------------------------------------------------------------------------------------------
def offsets_zero(rs, N, H, W):
    return np.zeros((N, 18, H, W), np.float32)


def offsets_uniform(rs, N, H, W):
    return rs.uniform(-1.5, 1.5, size=(N, 18, H, W)).astype(np.float32)


def offsets_quarter_out(rs, N, H, W):
    """U(-1.5, 1.5), and a quarter of the samples sent far outside the image: empty lists for the pixels they leave, and the others drawn
    towards the centre pixel's neighbourhood so that some lists are long"""
    off = rs.uniform(-1.5, 1.5, size=(N, 18, H, W)).astype(np.float32)
    t = np.arange(9)
    bx = np.arange(W)[None, None, :] + (t % 3)[:, None, None] - 1 + np.zeros((9, H, W))
    by = np.arange(H)[None, :, None] + (t // 3)[:, None, None] - 1 + np.zeros((9, H, W))
    u = rs.rand(N, 9, H, W)
    out, centre = u < 0.25, u > 0.75
    cx = W // 2 + rs.uniform(-0.95, 0.95, size=(N, 9, H, W))
    cy = H // 2 + rs.uniform(-0.95, 0.95, size=(N, 9, H, W))
    off[:, :9] = np.where(centre, cx - bx[None], off[:, :9])
    off[:, 9:] = np.where(centre, cy - by[None], off[:, 9:])
    off[:, :9] = np.where(out, 1e6, off[:, :9])
    return off.astype(np.float32)


GATHER_OFFSETS = {"zero": offsets_zero, "uniform": offsets_uniform, "quarter_out": offsets_quarter_out}
# N, H, W: the training tile; smaller than a wavefront; one pixel; past the kernels with lists in LDS (plane > 1476), still on the fused
# backward (launch_deform_input_grad); plane 2134, the first on launch_deform_backward's global-list branch
GATHER_SHAPES = [(2, 36, 36), (1, 5, 7), (1, 1, 1), (1, 45, 47), (1, 22, 97)]
GATHER_CASES = [(s, r) for s in GATHER_SHAPES for r in GATHER_OFFSETS]


def gather_id(shape, regime):
    return f"n{shape[0]}-{shape[1]}x{shape[2]}-{regime}"


@functools.lru_cache(maxsize=2)
def gather_operands(shape, regime):
    N, H, W = shape
    rs = np.random.RandomState(zlib.crc32(repr(("gather", shape, regime)).encode()) % 2**31)
    x = rs.normal(size=(N, 64, H, W)).astype(np.float32)
    off = GATHER_OFFSETS[regime](rs, N, H, W)
    w = (rs.normal(size=(64, 64, 3, 3)) / np.sqrt(64 * 9)).astype(np.float32)
    gy = rs.normal(size=(N, 64, H, W)).astype(np.float32)
    for a in (x, off, w, gy):
        a.setflags(write=False)
    return x, off, w, gy


def run_gather(dbm, shape, regime):
    """-> (id, {gx, goff, gw, gb}, operands): one call on NaN-filled gx / goff and zero gw / gb"""
    d, _lib, ctx = dbm
    x, off, w, gy = gather_operands(shape, regime)
    N, _, H, W = x.shape
    dev = lambda a: d.to_device(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    dx, doff, dw, dgy = dev(x), dev(off), dev(w), dev(gy)
    gx, goff = dev(np.full(x.shape, np.nan, np.float32)), dev(np.full(off.shape, np.nan, np.float32))
    gw, gb = dev(np.zeros(w.shape, np.float32)), dev(np.zeros(64, np.float32))
    rc = _lib.lib().dbm_op_deform_conv2d_backward(ctx.handle, dx.ptr, doff.ptr, dw.ptr, dgy.ptr, gx.ptr, goff.ptr, gw.ptr, gb.ptr, N, 64, H, W, 64)
    _lib.check(rc, ctx.handle)
    ctx.synchronize()
    return gather_id(shape, regime), {"gx": gx.get(), "goff": goff.get(), "gw": gw.get(), "gb": gb.get()}, (x, off, w, gy)


# ------------------------------------------------------------------------------------------------------------------------
# the record
# ------------------------------------------------------------------------------------------------------------------------
def record(dbm, progress=None):
    """name -> array, as tests/golden/perf_parent_bits.npz keeps it: '<part>/<case>/<output>/crc' (uint32) and '/val' (float32),
    'wgrad/<case>/cat' and '/S' (int32)"""
    rec = {}

    def put(prefix, outputs):
        for k, a in outputs.items():
            crc, val = summarise(a)
            rec[f"{prefix}/{k}/crc"], rec[f"{prefix}/{k}/val"] = crc, val

    for name in wgrad_cases():
        for (_, det, cleared), out, (cat, S) in run_wgrad(dbm, name):
            prefix = f"wgrad/{name}/det{det}-cleared{cleared}"
            rec[prefix + "/cat"], rec[prefix + "/S"] = np.asarray(cat, np.int32), np.asarray(S, np.int32)
            keep = {k: a for k, a in out.items() if wgrad_is_bitwise(det, cleared, S[int(k[2:])])}
            put(prefix, keep)
        if progress:
            progress("wgrad " + name)
    for cid in CHAIN_CASES:
        _, out, _ = run_chain(dbm, cid)
        put(f"chain/{cid}", out)
        if progress:
            progress("chain " + cid)
    for shape, regime in GATHER_CASES:
        gid, out, _ = run_gather(dbm, shape, regime)
        put(f"gather/{gid}", out)
        if progress:
            progress("gather " + gid)
    return rec
