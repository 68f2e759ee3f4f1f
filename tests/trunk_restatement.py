"""The RRDB trunk on 9 x 9 planes, one dense block at a time, restated in plain NumPy (srgan_train.py:333-360 ResidualDenseBlock,
:393-404 ResInResDenseBlock) -- the reference of tests/test_gpu_trunk_ops.py, proven against oracle/model.py by tests/test_trunk_host.py.

Everything runs in the dtype of the operands (float64 for the reference, float32 for the figure the tolerances are derived from).
Every function also returns the L1 MASS of each output element: the same computation on absolute values (|x|, |W|, |b|, |rs|, a
LeakyReLU mask as the factor 1 or |slope|), i.e. the sum of the magnitudes of the terms that make the element up.  A forward
LeakyReLU is 1-Lipschitz: its output's mass is its argument's.

A concat buffer is (N, 192, 9, 9): channels 0..63 the block's input, 64 + 32 k .. 95 + 32 k conv_layer(k + 1)'s output after its
LeakyReLU.  The concat GRADIENT dA[j] has the same shape: channels 0..63 the gradient of the block's input, the others the gradients
of conv_layer1..4's outputs in front of their LeakyReLU (what their weight gradients are taken from).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SLOPE = 0.2


def conv3(x, W, b=None):
    """3 x 3 cross-correlation, stride 1, zero padding 1: x (N, C, H, W), W (O, C, 3, 3) -> (N, O, H, W), in the operands' dtype"""
    N, C, H, Wd = x.shape
    O = W.shape[0]
    col = sliding_window_view(np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1))), (3, 3), axis=(2, 3))
    colm = np.ascontiguousarray(col.transpose(0, 2, 3, 1, 4, 5)).reshape(N * H * Wd, C * 9)
    y = colm @ np.ascontiguousarray(W.reshape(O, C * 9).T)
    if b is not None:
        y = y + b
    return np.ascontiguousarray(y.reshape(N, H, Wd, O).transpose(0, 3, 1, 2))


def conv3_dgrad(g, W):
    """gradient of conv3's input: g (N, O, H, W), W (O, C, 3, 3) -> (N, C, H, W)"""
    return conv3(g, np.ascontiguousarray(W.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]))


def lrelu(t):
    return np.where(t >= 0, t, t * t.dtype.type(SLOPE))


def lrelu_factor(y):
    """derivative of LeakyReLU by its retained OUTPUT, as oracle/ops.py: y >= 0 gives 1 (both zeros included)"""
    return np.where(y >= 0, y.dtype.type(1), y.dtype.type(SLOPE))


def dense_block_forward(x, W, b, rs, third=False, rrdb_in=None, forced=None):
    """One dense block.  x (N, 64, 9, 9): the block's input; W, b: conv_layer1..5's five tensors; third: the last block of its RRDB,
    whose output is scaled once more and takes the RRDB's input rrdb_in.  forced (N, 192, 9, 9): every layer reads its input from this
    concat buffer instead of from the layers computed here (teacher forcing; x is then forced[:, :64]).
    Returns (a, out, mass_a, mass_out): a[k] = lrelu(conv_layer(k + 1)), out = a5 * rs + x [third: (...) * rs + rrdb_in]."""
    dt = x.dtype.type
    rs = dt(rs)
    aW = [np.abs(w) for w in W]
    ab = [np.abs(v) for v in b]
    cat = x if forced is None else forced[:, :64]
    a, mass_a = [], []
    for k in range(4):
        src = cat if forced is None else forced[:, :64 + 32 * k]
        a.append(lrelu(conv3(src, W[k], b[k])))
        mass_a.append(conv3(np.abs(src), aW[k], ab[k]))
        if forced is None:
            cat = np.concatenate([cat, a[k]], axis=1)
    src = cat if forced is None else forced
    out = conv3(src, W[4], b[4]) * rs + src[:, :64]
    mass = conv3(np.abs(src), aW[4], ab[4]) * abs(rs) + np.abs(src[:, :64])
    if third:
        out = out * rs + rrdb_in
        mass = mass * abs(rs) + np.abs(rrdb_in)
    return a, out, mass_a, mass


def dense_block_backward(gout, cat, W, rs, pos, skip=None, g_a3=None):
    """Data gradients of one dense block.  gout (N, 64, 9, 9): gradient of the block's output -- for the third block of an RRDB
    (pos = 2) the gradient of the RRDB's output, which reaches conv_layer5 through rs * rs and the block's input through rs; cat
    (N, 192, 9, 9): the forward concat buffer, used for its signs only; W: the five weights; pos = j % 3; skip: for pos = 0 the
    gradient of the RRDB's output, which the RRDB's input receives unscaled; g_a3: for block 0 of the trunk, added to the input's
    gradient, which then passes the LeakyReLU in front of the trunk (the mask of cat[:, :64]).
    Returns (dA, mass), both (N, 192, 9, 9)."""
    dt = gout.dtype.type
    rs = dt(rs)
    third = pos == 2
    sc, r1s = (rs * rs, rs) if third else (rs, dt(1))
    f = lrelu_factor(cat)
    D = conv3_dgrad(gout, W[4]) * sc
    M = conv3_dgrad(np.abs(gout), np.abs(W[4])) * abs(sc)
    D[:, :64] += r1s * gout
    M[:, :64] += abs(r1s) * np.abs(gout)
    for k in (3, 2, 1, 0):
        lo = 64 + 32 * k
        D[:, lo:lo + 32] *= f[:, lo:lo + 32]
        M[:, lo:lo + 32] *= f[:, lo:lo + 32]
        D[:, :lo] += conv3_dgrad(D[:, lo:lo + 32], W[k])
        M[:, :lo] += conv3_dgrad(M[:, lo:lo + 32], np.abs(W[k]))
    if pos == 0:
        D[:, :64] += skip
        M[:, :64] += np.abs(skip)
    if g_a3 is not None:
        D[:, :64] = (D[:, :64] + g_a3) * f[:, :64]
        M[:, :64] = (M[:, :64] + np.abs(g_a3)) * f[:, :64]
    return D, M


def trunk_forward(x, W, b, rs):
    """The chain of len(W) // 5 dense blocks from x (N, 64, 9, 9).  Returns (cat, mass): nrdb + 1 concat buffers (the last one holds
    the trunk's output in channels 0..63 and zeros behind it) and the masses of the same shape."""
    nrdb = len(W) // 5
    cat, mass = [], []
    h, mh, rrdb_in = x, np.abs(x), None
    for j in range(nrdb):
        if j % 3 == 0:
            rrdb_in = h
        a, out, ma, mo = dense_block_forward(h, W[5 * j:5 * j + 5], b[5 * j:5 * j + 5], rs, j % 3 == 2, rrdb_in)
        cat.append(np.concatenate([h] + a, axis=1))
        mass.append(np.concatenate([mh] + ma, axis=1))
        h, mh = out, mo
    pad = np.zeros((x.shape[0], 128) + x.shape[2:], dtype=x.dtype)
    cat.append(np.concatenate([h, pad], axis=1))
    mass.append(np.concatenate([mh, pad], axis=1))
    return cat, mass


def trunk_backward(gin, cat, W, rs, g_a3, j_top=None, j_bottom=0):
    """The data-gradient chain over dense blocks j_top - 1 .. j_bottom (whole RRDBs) from gin (N, 64, 9, 9), the gradient of block
    j_top - 1's output.  g_a3 is used at block 0 only.  Returns ({j: dA[j]}, {j: mass})."""
    nrdb = len(W) // 5
    j_top = nrdb if j_top is None else j_top
    dA, mass = {}, {}
    g = skip = gin
    for j in range(j_top - 1, j_bottom - 1, -1):
        if j % 3 == 2:
            skip = g
        dA[j], mass[j] = dense_block_backward(g, cat[j], W[5 * j:5 * j + 5], rs, j % 3, skip if j % 3 == 0 else None,
                                              g_a3 if j == 0 else None)
        g = dA[j][:, :64]
    return dA, mass
