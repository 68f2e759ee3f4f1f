"""Float64 NumPy restatement of the maps' vector layers (dbm_image_overlay in include/dbm.h; reference
paper_figures.py:533-562, :1039-1045).

Not collected by pytest (no test_ prefix): the CPU tests check it against closed forms and check `draw_layers_host` against it; the GPU
tests check the kernels against it byte for byte.  Brute force -- every sub-sample of a chunk of rows against every primitive at once,
by broadcasting -- written from the rule, not from overlay.py or the kernel: no culling, no binning, no windows, no shortcut.  Every
operation is one float64 NumPy ufunc, so each is rounded once.

A layer is a tuple (kind, table, size, rgba): kind "segments" with table (n, 4) rows (xa, ya, xb, yb), or "discs" with table (n, >= 2)
rows (x, y, ...); size in pixels; rgba four integers 0..255.
"""
import numpy as np


def pixel_units(geom, table, kind):
    """Step 1: u = (x - x0) / dx, v = (y - y0) / dy, a subtraction and a division.  Returns (ua, va, ub, vb); discs: b is a."""
    x0, y0, dx, dy = (np.float64(v) for v in geom[:4])
    t = np.asarray(table, dtype=np.float64).reshape(len(table), -1)
    with np.errstate(all="ignore"):
        ua, va = (t[:, 0] - x0) / dx, (t[:, 1] - y0) / dy
        if kind == "segments":
            return ua, va, (t[:, 2] - x0) / dx, (t[:, 3] - y0) / dy
    return ua, va, ua, va


def sub_samples(first, count, S):
    """Step 2 along one axis: (count, S) coordinates, index + ((j + 0.5) / S - 0.5)."""
    j = np.arange(S, dtype=np.float64)
    return np.arange(first, first + count, dtype=np.float64)[:, None] + ((j + 0.5) / S - 0.5)[None, :]


def coverage(geom, shape, kind, table, size, S, rows=None, cells_per_chunk=3_000_000):
    """Step 3: m (rows, W) = the number of the S x S sub-samples of every pixel that some primitive covers.  rows = (r0, r1): only
    the rows r0 .. r1 - 1 of the (H, W) image."""
    H, W = shape
    r0, r1 = (0, H) if rows is None else rows
    m = np.zeros((r1 - r0, W), dtype=np.int64)
    n = len(table)
    if n == 0:
        return m
    ua, va, ub, vb = (a[None, None, None, None, :] for a in pixel_units(geom, table, kind))
    half = np.float64(size) / np.float64(2.0)
    limit = half * half
    su = sub_samples(0, W, S)[None, None, :, :, None]                      # [1, 1, c, j, 1]
    step = max(1, int(cells_per_chunk // max(1, W * S * S * n)))
    with np.errstate(all="ignore"):
        if kind == "segments":
            ex, ey = ub - ua, vb - va
            L = ex * ex + ey * ey
            Lsafe = np.where(L > 0, L, 1.0)
        for a in range(r0, r1, step):
            b = min(a + step, r1)
            sv = sub_samples(a, b - a, S)[:, :, None, None, None]          # [r, i, 1, 1, 1]
            px, py = su - ua, sv - va
            if kind == "segments":
                t = np.where(L > 0, (px * ex + py * ey) / Lsafe, 0.0)
                t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
                qx, qy = px - t * ex, py - t * ey
                d2 = qx * qx + qy * qy
            else:
                d2 = px * px + py * py
            covered = (d2 <= limit).any(axis=4)                            # [r, i, c, j]
            m[a - r0:b - r0] = covered.sum(axis=(1, 3))
    return m


def blend_value(m, A, src, dst, S):
    """Step 4 for one channel, in Python integers."""
    D = S * S * 255
    w = int(m) * int(A)
    return (w * int(src) + (D - w) * int(dst) + D // 2) // D


def blend(image, m, rgba, S):
    """Step 4 on a (rows, W, channels) uint8 image: returns the new bytes; pixels with m = 0 keep theirs."""
    out = np.array(image, dtype=np.uint8, copy=True)
    D = S * S * 255
    w = m.astype(np.int64) * int(rgba[3])
    hit = m > 0
    for ch in range(image.shape[2]):
        src = int(rgba[ch]) if ch < 3 else 255
        value = (w * src + (D - w) * image[:, :, ch].astype(np.int64) + D // 2) // D
        out[:, :, ch][hit] = value[hit].astype(np.uint8)
    return out


def paint(image, geom, layers, S, rows=None):
    """Step 5: the layers in list order, each over the result of the ones before.  rows = (r0, r1): `image` is that band of rows of
    an (H, W) image, H = rows[2]."""
    out = np.array(image, dtype=np.uint8, copy=True)
    shape = (out.shape[0], out.shape[1]) if rows is None else (rows[2], out.shape[1])
    for kind, table, size, rgba in layers:
        m = coverage(geom, shape, kind, table, size, S, rows=None if rows is None else rows[:2])
        out = blend(out, m, rgba, S)
    return out
