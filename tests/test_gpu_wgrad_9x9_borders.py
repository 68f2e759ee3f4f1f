"""-m gpu: the borders of wgrad_wave_dma_9x9_kernel.  Its x tile is an unframed slab, so a tap that leaves the plane reads a cell of the
neighbouring row or plane and must meet a zero A value (deepbedmap_amd/csrc/wgrad_9x9_index.h); tools/wgrad_9x9_index_check.cpp replays the
indices on the CPU, this file asks the kernel.  dbm_op_conv2d_wgrad_batch as tests/exposed_kernel_cases.py calls it: x is a channel slice
of an (N, 192, 9, 9) buffer, scale 0.5.  9 x 9 planes, N in {1, 2, 3}, with and without bias gradient, deterministic mode (onto a prefilled
target) and atomic mode with a cleared target.

  exact         x and dy are small integers, every cell of every x plane is distinct (a permutation of -40 .. 40), the prefill is integer:
                every fp32 sum is exact (the reference's sum of |terms| is checked against 2^24 on the CPU), so the result must EQUAL the
                float64 gradient -- in any order of the K slices, hence also in atomic mode.
  border probes dy is non-zero at one position only (each corner, one edge cell, the centre), x only on the plane's outer ring: what the
                kernel adds comes from the taps of that position alone, and the ring is where a wrapped read finds a non-zero cell.
  kernel against kernel   the same layer in a launch that also holds an 8 x 8 layer: a mixed launch takes the general kernel
                (wgrad_wave_dma_kernel, framed planes, every MFMA issued).  Random normal inputs, deterministic mode: bit-equal gradients.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exposed_kernel_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (64, 32), (96, 32), (160, 32), (192, 64), (64, 16), (36, 32)]
NS = (1, 2, 3)
MODES = [(1, 0), (0, 1)]   # (deterministic, cleared target)
PROBES = {"corner00": (0, 0), "corner08": (0, 8), "corner80": (8, 0), "corner88": (8, 8), "edge04": (0, 4), "centre": (4, 4)}


@pytest.fixture(scope="module")
def dbm():
    return cases.load()


def layer9(C_in, O, gb):
    return cases._layer(9, 9, C_in, O, min(32, cases.CAT_BUF - C_in), gb)


def launch(dbm, N, layers, ops, det, cleared):
    """one dbm_op_conv2d_wgrad_batch call -> ({gW<i>, gb<i>}, categories, K slices); ops: per layer (x buffer, dy, gW prefill, gb prefill)"""
    d, _lib, ctx = dbm
    n = len(layers)
    dev_x = [d.to_device(np.ascontiguousarray(x).reshape(-1)) for x, _, _, _ in ops]
    dev_y = [d.to_device(np.ascontiguousarray(dy).reshape(-1)) for _, dy, _, _ in ops]
    dev_W = [d.to_device(np.zeros_like(gW0) if cleared else gW0) for _, _, gW0, _ in ops]
    dev_b = [d.to_device(np.zeros_like(gb0) if cleared else gb0) for _, _, _, gb0 in ops]
    arr = (_lib.WgradDesc * n)()
    for i, L in enumerate(layers):
        a, plane = arr[i], L["H"] * L["W"]
        a.x, a.xsn = dev_x[i].ptr + 4 * L["c0"] * plane, cases.CAT_BUF * plane
        a.dy, a.dysn = dev_y[i].ptr, L["O"] * plane
        a.N, a.C, a.H, a.W, a.O, a.k, a.stride, a.pad, a.ups = N, L["C"], L["H"], L["W"], L["O"], 3, 1, 1, 0
        a.scale = cases.WGRAD_SCALE
        a.gW = dev_W[i].ptr
        a.gb = dev_b[i].ptr if L["gb"] else None
    try:
        _lib.check(_lib.lib().dbm_set_deterministic(ctx.handle, det), ctx.handle)
        cat, S = (C.c_int * n)(), (C.c_int * n)()
        _lib.check(_lib.lib().dbm_op_conv2d_wgrad_batch(ctx.handle, arr, n, int(cleared), cat, S), ctx.handle)
        ctx.synchronize()
        out = {}
        for i, L in enumerate(layers):
            out[f"gW{i}"] = dev_W[i].get()
            if L["gb"]:
                out[f"gb{i}"] = dev_b[i].get()
        return out, list(cat), list(S)
    finally:
        cases.restore_deterministic(ctx)


def integer_prefill(rs, C_in, O):
    return rs.randint(-8, 9, size=(O, C_in, 3, 3)).astype(np.float32), rs.randint(-8, 9, size=(O,)).astype(np.float32)


def check_exact(dbm, N, C_in, O, x, dy, rs, what):
    """every mode and bias setting on one pair of integer operands: got == float64 reference (+ prefill)"""
    gW0, gb0 = integer_prefill(rs, C_in, O)
    L = layer9(C_in, O, 1)
    gW, mW, gb, mb = cases.wgrad_reference(x, dy, L, cases.WGRAD_SCALE)
    # exactness of every fp32 partial sum in any order: the sum of |terms| (before the scale, a power of two) plus the prefill stays below 2^24
    assert (mW / cases.WGRAD_SCALE).max() + 8 < 2 ** 24 and (mb / cases.WGRAD_SCALE).max() + 8 < 2 ** 24
    for with_gb in (1, 0):
        for det, cleared in MODES:
            out, cat, S = launch(dbm, N, [layer9(C_in, O, with_gb)], [(x, dy, gW0, gb0)], det, cleared)
            assert cat == [3], (what, cat)
            pre = 0.0 if cleared else 1.0
            got = out["gW0"].astype(np.float64)
            want = gW + pre * gW0
            bad = np.argwhere(got != want)
            assert bad.size == 0, (what, f"gb{with_gb} det{det} cleared{cleared} S{S}", "first differing (o, c, ty, tx):", bad[:4].tolist(),
                                   got[tuple(bad[0])], want[tuple(bad[0])])
            if with_gb:
                assert np.array_equal(out["gb0"].astype(np.float64), gb + pre * gb0), (what, det, cleared)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C_in,O", SHAPES)
def test_exact_integers(dbm, C_in, O, N):
    rs = np.random.RandomState(1000 * C_in + 10 * O + N)
    x = np.empty((N, cases.CAT_BUF, 81), np.float32)
    for n in range(N):
        for c in range(cases.CAT_BUF):
            x[n, c] = rs.permutation(81) - 40   # every cell of a plane distinct
    x = x.reshape(N, cases.CAT_BUF, 9, 9)
    dy = rs.randint(-3, 4, size=(N, O, 9, 9)).astype(np.float32)
    check_exact(dbm, N, C_in, O, x, dy, rs, f"exact c{C_in} o{O} n{N}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C_in,O", SHAPES)
def test_border_probes(dbm, C_in, O, N):
    rs = np.random.RandomState(2000 * C_in + 10 * O + N)
    ring = np.ones((9, 9), bool)
    ring[1:-1, 1:-1] = False
    x = np.zeros((N, cases.CAT_BUF, 9, 9), np.float32)
    vals = rs.randint(1, 60, size=(N, cases.CAT_BUF, int(ring.sum()))) * rs.choice([-1, 1], size=(N, cases.CAT_BUF, int(ring.sum())))
    x[:, :, ring] = vals
    for name, (py, px) in PROBES.items():
        dy = np.zeros((N, O, 9, 9), np.float32)
        dy[:, :, py, px] = rs.randint(1, 4, size=(N, O)) * rs.choice([-1, 1], size=(N, O))
        check_exact(dbm, N, C_in, O, x, dy, rs, f"probe {name} c{C_in} o{O} n{N}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C_in,O", SHAPES)
def test_9x9_kernel_against_general_kernel(dbm, C_in, O, N):
    rs = np.random.RandomState(3000 * C_in + 10 * O + N)
    L9, L8 = layer9(C_in, O, 1), cases._layer(8, 8, 64, 32, 32, 1)
    ops = []
    for L in (L9, L8):
        ops.append((rs.normal(size=(N, cases.CAT_BUF, L["H"], L["W"])).astype(np.float32), rs.normal(size=(N, L["O"], L["H"], L["W"])).astype(np.float32),
                    rs.normal(size=(L["O"], L["C"], 3, 3)).astype(np.float32), rs.normal(size=(L["O"],)).astype(np.float32)))
    alone, cat_a, S_a = launch(dbm, N, [L9], ops[:1], 1, 0)         # every plan 9 x 9: wgrad_wave_dma_9x9_kernel
    mixed, cat_m, S_m = launch(dbm, N, [L9, L8], ops, 1, 0)         # an 8 x 8 plan among them: wgrad_wave_dma_kernel
    assert cat_a == [3] and cat_m == [3, 3], (cat_a, cat_m)
    assert S_a[0] == S_m[0], f"the two launches split K differently ({S_a[0]}, {S_m[0]}): their bits cannot be compared"
    for k in ("gW0", "gb0"):
        a, m = alone[k].view(np.uint32), mixed[k].view(np.uint32)
        assert np.array_equal(a, m), (k, "first differing:", np.argwhere(a != m)[:4].tolist())
