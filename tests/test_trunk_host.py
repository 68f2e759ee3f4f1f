"""CPU: tests/trunk_restatement.py (the block-by-block reference of test_gpu_trunk_ops.py) reproduces oracle/model.py's trunk in float64.

The oracle keeps the forward concat buffers (`rdb_cat`) and the trunk's output (`a2`); of its backward pass it keeps only parameter
gradients, so the gradients that flow through the trunk are recorded where it hands them to ops.conv2d_backward: conv_layer1..4 of
dense block j receive dA[j][:, 64 + 32 k : 96 + 32 k], conv_layer5 of block j receives dA[j + 1][:, :64] times rs (rs * rs for the last
block of an RRDB), pre_residual_conv_layer receives dA[0][:, :64].  Every element agrees to 1e-12 of its L1 mass.
"""
import os
import sys

import numpy as np
import pytest

from oracle import model as omodel
from oracle import ops

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import trunk_restatement as tr  # noqa: E402

RS = 0.3


def oracle_trunk(n_rrdb, N=2, seed=5):
    g = omodel.GeneratorModel(num_residual_blocks=n_rrdb, residual_scaling=RS, seed=seed, dtype=np.float64)
    r = np.random.RandomState(seed + 1)
    for k in g.params:
        if k.endswith("/W"):
            g.params[k] = g.params[k] * 1.5
        else:
            g.params[k] = g.params[k] + r.normal(0, 0.1, g.params[k].shape)
    x, w1, w2, w3 = r.rand(N, 1, 11, 11), r.rand(N, 1, 110, 110), r.rand(N, 2, 22, 22), r.rand(N, 1, 11, 11)
    y = g.forward(x, w1, w2, w3, keep=True)
    names = {id(v): k[:-2] for k, v in g.params.items() if k.endswith("/W")}
    seen = {}
    plain = ops.conv2d_backward

    def recording(xin, W, gy, *args, **kw):
        out = plain(xin, W, gy, *args, **kw)
        seen[names[id(W)]] = (np.array(gy), None if out[0] is None else np.array(out[0]))
        return out

    ops.conv2d_backward = recording
    try:
        g.backward(r.normal(0, 1, y.shape))
    finally:
        ops.conv2d_backward = plain
    return g, seen


def trunk_tensors(g, n_rrdb):
    W, b = [], []
    for i in range(n_rrdb):
        for d in (1, 2, 3):
            for k in (1, 2, 3, 4, 5):
                base = f"residual_network/{i}/residual_dense_block{d}/conv_layer{k}"
                W.append(g.params[base + "/W"])
                b.append(g.params[base + "/b"])
    return W, b


def assert_within_mass(got, want, mass, what):
    assert got.shape == want.shape == mass.shape, what
    assert np.isfinite(got).all() and (mass > 0).all(), what
    worst = float((np.abs(got - want) / mass).max())
    assert worst <= 1e-12, (what, worst)


@pytest.mark.parametrize("nrdb", [3, 6])
def test_block_functions_reproduce_the_oracle_trunk(nrdb):
    n_rrdb = nrdb // 3
    g, seen = oracle_trunk(n_rrdb)
    c = g.cache
    W, b = trunk_tensors(g, n_rrdb)
    cat, mass = tr.trunk_forward(c["a1"], W, b, RS)
    assert len(cat) == nrdb + 1
    for j in range(nrdb):
        assert_within_mass(cat[j], c["rdb_cat"][j], mass[j], f"cat[{j}]")
    assert_within_mass(cat[nrdb][:, :64], c["a2"], mass[nrdb][:, :64], "a2")
    assert not cat[nrdb][:, 64:].any()

    g_a3, gin = seen["post_residual_conv_layer"]
    dA, dmass = tr.trunk_backward(gin, c["rdb_cat"], W, RS, g_a3)
    assert sorted(dA) == list(range(nrdb))
    for j in range(nrdb):
        base = f"residual_network/{j // 3}/residual_dense_block{j % 3 + 1}/conv_layer"
        for k in range(4):
            lo = 64 + 32 * k
            assert_within_mass(dA[j][:, lo:lo + 32], seen[base + str(k + 1)][0], dmass[j][:, lo:lo + 32], f"dA[{j}] layer {k + 1}")
        sc = RS * RS if j % 3 == 2 else RS
        gout = gin if j == nrdb - 1 else dA[j + 1][:, :64]
        gmass = np.abs(gin) if j == nrdb - 1 else dmass[j + 1][:, :64]
        assert_within_mass(gout * sc, seen[base + "5"][0], gmass * sc, f"gradient of block {j}'s output")
    assert_within_mass(dA[0][:, :64], seen["pre_residual_conv_layer"][0], dmass[0][:, :64], "dA[0][:, :64]")


def test_forced_layers_equal_the_chained_ones_on_the_chain_s_own_buffers():
    """teacher forcing changes where a layer reads, not what it computes"""
    r = np.random.RandomState(0)
    W = [r.normal(0, 0.05, (32 if k < 4 else 64, 64 + 32 * k, 3, 3)) for k in range(5)]
    b = [r.normal(0, 0.1, (32 if k < 4 else 64,)) for k in range(5)]
    x, xin = r.normal(0, 1, (2, 64, 9, 9)), r.normal(0, 1, (2, 64, 9, 9))
    a, out, ma, mo = tr.dense_block_forward(x, W, b, RS, True, xin)
    forced = np.concatenate([x] + a, axis=1)
    a2, out2, ma2, mo2 = tr.dense_block_forward(x, W, b, RS, True, xin, forced=forced)
    for k in range(4):
        assert np.array_equal(a[k], a2[k]) and np.array_equal(ma[k], ma2[k])
    assert np.array_equal(out, out2) and np.array_equal(mo, mo2)


def test_mask_zero_counts_as_positive_and_masses_bound_the_values():
    r = np.random.RandomState(1)
    W = [r.normal(0, 0.05, (32 if k < 4 else 64, 64 + 32 * k, 3, 3)) for k in range(5)]
    cat = r.normal(0, 1, (1, 192, 9, 9))
    cat[0, 70, 4, 4] = 0.0
    cat[0, 71, 4, 4] = -0.0
    cat[0, 72, 4, 4] = -1e-30
    f = tr.lrelu_factor(cat)
    assert f[0, 70, 4, 4] == 1 and f[0, 71, 4, 4] == 1 and f[0, 72, 4, 4] == tr.SLOPE
    g = r.normal(0, 1, (1, 64, 9, 9))
    for pos in (0, 1, 2):
        D, M = tr.dense_block_backward(g, cat, W, RS, pos, skip=g if pos == 0 else None, g_a3=g)
        assert (np.abs(D) <= M * (1 + 1e-12)).all()
