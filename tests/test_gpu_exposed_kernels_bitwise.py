"""-m gpu: the three kernels on the generator's own path in the training step -- the trunk's weight gradients (wgrad_wave_dma_kernel and its
9 x 9 body wgrad_wave_dma_9x9_kernel), the data-gradient chain (trunk_fused_bwd_kernel) and the deformable backward's stored-list gather
(deform_csr_gather_kernel) -- against the bits the PARENT commit's library gave for the same seeded op-level cases:
tests/golden/perf_parent_bits.npz, written by tools/record_parent_bits.py on an MI355X from a checkout of the parent.  Speed work on
these kernels re-orders instructions, never sums: every output must come back bit for bit (a CRC-32 over the whole array, and 128 evenly
spaced values that say where two libraries part).  No second code path is kept in the library for the comparison.

So that a wrong record cannot pass silently, every case is also held against float64:
  weight gradients   |got - ref| <= (K + 2) * 2^-24 * mass per element, K = N * OH * OW terms, mass = scale * sum |dy| |x| (+ |prefill|): the
                     worst-case bound of a float32 sum of K products in any order (each product and each addition rounds once; first
                     order in 2^-24), so it holds for every K split and fold.  This is the only check of the atomic mode where the order
                     of the K slices' additions is not fixed (exposed_kernel_cases.wgrad_is_bitwise says where it is).
  chain              dA[j] teacher-forced against the float64 block backward of tests/trunk_restatement.py, every element over its L1
                     mass, tolerance as tests/test_gpu_trunk_ops.py takes it: 16 x the float32 restatement's own worst deviation on the
                     cases' problems, floor 8 * 2^-24, cap 1e-4
  gather             gx and goff against the float64 oracle with the bounds of tests/test_gpu_deform_backward.py (1e-4, 5e-4 of the
                     tensor maximum)
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exposed_kernel_cases as cases  # noqa: E402
import trunk_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "perf_parent_bits.npz")


@pytest.fixture(scope="module")
def dbm():
    return cases.load()


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def assert_parent_bits(prefix, outputs):
    g = golden()
    for k, a in outputs.items():
        crc, val = cases.summarise(a)
        want = g[f"{prefix}/{k}/val"]
        assert val.shape == want.shape and np.array_equal(val.view(np.uint32), want.view(np.uint32)), \
            f"{prefix}/{k}: sampled values differ from the parent's at sample indices {np.flatnonzero(val.view(np.uint32) != want.view(np.uint32))[:8]}"
        assert np.uint32(crc) == g[f"{prefix}/{k}/crc"], f"{prefix}/{k}: the samples agree but the array's CRC-32 differs from the parent's"


# ---- weight gradients ----
@pytest.mark.parametrize("name", list(cases.wgrad_cases()))
def test_wgrad_bits(dbm, name):
    N, layers, ops = cases.wgrad_operands(name)
    refs = [cases.wgrad_reference(x, dy, L, cases.WGRAD_SCALE) for L, (x, dy, _, _) in zip(layers, ops)]
    g = golden()
    seen = 0
    for (_, det, cleared), out, (cat, S) in cases.run_wgrad(dbm, name):
        prefix = f"wgrad/{name}/det{det}-cleared{cleared}"
        assert cat == list(g[prefix + "/cat"]) and S == list(g[prefix + "/S"]), (prefix, cat, S)
        for i, L in enumerate(layers):
            if (L["H"], L["W"]) in ((9, 9), (8, 8)):
                assert cat[i] == 3, (prefix, i, cat)
            K = N * L["H"] * L["W"]
            gW, mW, gb, mb = refs[i]
            gW0, gb0 = ops[i][2].astype(np.float64), ops[i][3].astype(np.float64)
            pre = 0.0 if cleared else 1.0
            eW = np.abs(out[f"gW{i}"].astype(np.float64) - (gW + pre * gW0)) / (mW + pre * np.abs(gW0) + 1e-30)
            assert eW.max() <= (K + 2) * 2.0 ** -24, (prefix, i, float(eW.max()))
            if L["gb"]:
                eb = np.abs(out[f"gb{i}"].astype(np.float64) - (gb + pre * gb0)) / (mb + pre * np.abs(gb0) + 1e-30)
                assert eb.max() <= (K + 2) * 2.0 ** -24, (prefix, i, float(eb.max()))
        keep = {k: a for k, a in out.items() if cases.wgrad_is_bitwise(det, cleared, S[int(k[2:])])}
        assert det == 0 or len(keep) == len(out)
        assert_parent_bits(prefix, keep)
        seen += 1
    assert seen == len(cases.WGRAD_MODES)


# ---- the chain ----
@functools.lru_cache(maxsize=None)
def chain_tolerance():
    """16 x the float32 restatement's worst |d| / mass against the float64 one, teacher-forced, over the problems of the cases"""
    worst = 0.0
    for nrdb, N, rs in ((3, 5, 0.3), (6, 2, 0.1)):
        P = cases.chain_problem(nrdb, N)
        dA32, _ = tr.trunk_backward(P.gin, P.masks, P.W, np.float32(rs), P.g_a3)
        for j in range(nrdb):
            gsrc = P.gin if j == nrdb - 1 else dA32[j + 1][:, :64]
            skip = None
            if j % 3 == 0:
                skip = P.gin if j + 3 == nrdb else dA32[j + 3][:, :64]
            D, M = tr.dense_block_backward(gsrc.astype(np.float64), P.masks[j].astype(np.float64), P.W64[5 * j:5 * j + 5], float(np.float32(rs)),
                                           j % 3, None if skip is None else skip.astype(np.float64), P.g_a3.astype(np.float64) if j == 0 else None)
            worst = max(worst, float((np.abs(dA32[j] - D) / M).max()))
    return min(max(16.0 * worst, 8 * 2.0 ** -24), 1e-4)


@pytest.mark.parametrize("cid", list(cases.CHAIN_CASES))
def test_chain_bits(dbm, cid):
    nrdb, N, launches, rs = cases.CHAIN_CASES[cid]
    _, out, P = cases.run_chain(dbm, cid)
    tol = chain_tolerance()
    f64 = lambda a: np.asarray(a, np.float64)   # noqa: E731
    for j in range(nrdb - 1, -1, -1):
        assert not np.isnan(out[f"dA{j}"]).any(), f"dA[{j}] holds NaN: a sentinel was read, or a cell was not written"
        gsrc = P.gin if j == nrdb - 1 else out[f"dA{j + 1}"][:, :64]
        skip = None
        if j % 3 == 0:
            skip = P.gin if j + 3 == nrdb else out[f"dA{j + 3}"][:, :64]
        D, M = tr.dense_block_backward(f64(gsrc), f64(P.masks[j]), P.W64[5 * j:5 * j + 5], float(np.float32(rs)), j % 3,
                                       None if skip is None else f64(skip), f64(P.g_a3) if j == 0 else None)
        e = float((np.abs(f64(out[f"dA{j}"]) - D) / M).max())
        assert e <= tol, f"{cid}: dA[{j}]: |d| / mass {e:.3g} > {tol:.3g}"
    assert_parent_bits(f"chain/{cid}", out)


# ---- the gather ----
@pytest.mark.parametrize("shape,regime", cases.GATHER_CASES, ids=[cases.gather_id(s, r) for s, r in cases.GATHER_CASES])
def test_gather_bits(dbm, shape, regime):
    from oracle import ops

    gid, out, (x, off, w, gy) = cases.run_gather(dbm, shape, regime)
    with np.errstate(over="ignore"):
        ref = dict(zip(("gx", "goff", "gw", "gb"), ops.deform_conv2d_backward(x.astype(np.float64), off, w.astype(np.float64), gy.astype(np.float64))))
    for k, bound in (("gx", 1e-4), ("goff", 5e-4)):
        assert np.isfinite(out[k]).all(), k
        e = float(np.abs(out[k].astype(np.float64) - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30))
        assert e < bound, (gid, k, e)
    assert_parent_bits(f"gather/{gid}", out)
