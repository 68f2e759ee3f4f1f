"""Float64 NumPy restatement of the buffered-polygon node mask (dbm_grid_polygon_mask in include/dbm.h; reference
data_prep.py:582-616).

Not collected by pytest (no test_ prefix): the CPU tests check it against matplotlib's point-in-polygon test and against closed forms;
the GPU tests check the kernels against it bit for bit.  Brute force -- every node against every edge, chunked over rows -- written from
the rules, not from the kernel: no culling, no binning, no shortcut.  Every operation is one float64 NumPy ufunc, so each is rounded once.
"""
import numpy as np


def node_axes(geom, shape):
    """x[c] = x0 + c dx, y[r] = y0 + r dy: one multiplication and one addition, each rounded."""
    x0, y0, dx, dy = (np.float64(v) for v in geom[:4])
    H, W = shape
    return np.arange(W, dtype=np.float64) * dx + x0, np.arange(H, dtype=np.float64) * dy + y0


def inside_near(geom, shape, edges, buffer, rows_per_chunk=None):
    """(inside, near) bool (H, W): even-odd parity of the crossings to the east, and d2 <= buffer * buffer for some edge."""
    H, W = shape
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    xs, ys = node_axes(geom, shape)
    inside = np.zeros((H, W), dtype=bool)
    near = np.zeros((H, W), dtype=bool)
    if len(e) == 0:
        return inside, near
    b2 = np.float64(buffer) * np.float64(buffer)
    xa, ya, xb, yb = (e[:, k][None, None, :] for k in range(4))
    ex, ey = xb - xa, yb - ya
    L = ex * ex + ey * ey
    Lsafe = np.where(L > 0, L, 1.0)
    eysafe = np.where(ey != 0, ey, 1.0)
    if rows_per_chunk is None:
        rows_per_chunk = max(1, int(4e6 // max(1, W * len(e))))
    with np.errstate(all="ignore"):
        for r0 in range(0, H, rows_per_chunk):
            y = ys[r0:r0 + rows_per_chunk][:, None, None]
            x = xs[None, :, None]
            straddle = (ya <= y) != (yb <= y)
            xint = xa + ((y - ya) * ex) / eysafe
            inside[r0:r0 + rows_per_chunk] = ((straddle & (x < xint)).sum(axis=2) % 2) == 1
            px, py = x - xa, y - ya
            t = np.where(L > 0, (px * ex + py * ey) / Lsafe, 0.0)
            t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
            qx, qy = px - t * ex, py - t * ey
            d2 = qx * qx + qy * qy
            near[r0:r0 + rows_per_chunk] = (d2 <= b2).any(axis=2)
    return inside, near


def mask(geom, shape, edges, buffer):
    """buffer >= 0 (-0.0 included): inside | near; buffer < 0: inside & ~near; no edges: all False."""
    inside, near = inside_near(geom, shape, edges, buffer)
    return (inside | near) if np.float64(buffer) >= 0 else (inside & ~near)


def mask_grid(grid, m):
    """NaN (the quiet float32 NaN 0x7fc00000) where the mask is 0, every other node's bits untouched."""
    out = np.array(grid, dtype=np.float32, copy=True)
    out.view(np.uint32)[~np.asarray(m, dtype=bool)] = 0x7FC00000
    return out


def ring_edges(rings):
    """All rings pooled as (E, 4) edges; each ring is closed (last vertex joined to the first unless it repeats it)."""
    out = []
    for ring in rings:
        p = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
        if len(p) > 1 and np.array_equal(p[0], p[-1]):
            p = p[:-1]
        q = np.roll(p, -1, axis=0)
        out.append(np.concatenate([p, q], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4))


def filled_windows(ok, size, step):
    """A plain Python window scan: [(uly, ulx)] of the size x size windows, moved by step from the north-west corner of a north-up
    raster, whose nodes are all True."""
    H, W = ok.shape
    return [(i, j) for i in range((H - size) // step + 1) for j in range((W - size) // step + 1)
            if ok[i * step:i * step + size, j * step:j * step + size].all()]
