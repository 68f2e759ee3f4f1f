"""SciPy / NumPy restatement of the tension surface, the distance mask and the gridline -> pixel sampler (include/dbm.h:
dbm_grid_tension_surface, dbm_grid_distance_mask, dbm_grid_to_pixel), written from the definition in DESIGN.md "Tension surface" and
sharing no code with the library: the operator is assembled from Kronecker products of 1-D difference matrices and the free nodes are
solved directly (float64 sparse LU), so it checks the conjugate-gradient kernels to rounding."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl


def difference(n, order):
    """(n - order, n): first or second differences along an axis of n nodes; only the stencils that fit inside exist"""
    if order == 1:
        return sp.diags([-np.ones(n - 1), np.ones(n - 1)], [0, 1], shape=(n - 1, n))
    return sp.diags([np.ones(n - 2), -2.0 * np.ones(n - 2), np.ones(n - 2)], [0, 1, 2], shape=(n - 2, n))


def operator(H, W, T, gradient_weight=None):
    """A = (1 - T)(Dxx' Dxx + Dyy' Dyy + 2 Dxy' Dxy) + T (Dx' Dx + Dy' Dy) on the row-major nodes of an (H, W) grid, CSR.
    gradient_weight replaces the factor T of the gradient term (0: the bending term alone)."""
    eye = sp.identity
    dxx, dyy = sp.kron(eye(H), difference(W, 2)), sp.kron(difference(H, 2), eye(W))
    dxy = sp.kron(difference(H, 1), difference(W, 1))
    dx, dy = sp.kron(eye(H), difference(W, 1)), sp.kron(difference(H, 1), eye(W))
    g = T if gradient_weight is None else gradient_weight
    return ((1.0 - T) * (dxx.T @ dxx + dyy.T @ dyy + 2.0 * (dxy.T @ dxy)) + g * (dx.T @ dx + dy.T @ dy)).tocsr()


def tension_surface(d, T=0.35):
    """float64 (H, W): the minimiser with u = d on the non-NaN nodes of d, by a direct solve on the free nodes.  The shift m is the
    first constraint node's value, as the library's (the exact minimiser does not depend on it)."""
    d = np.asarray(d)
    H, W = d.shape
    k = ~np.isnan(d).ravel()
    if not k.any():
        raise ValueError("no constraint node")
    f = ~k
    u = np.where(k, d.ravel().astype(np.float64), 0.0)
    if not f.any():
        return u.reshape(H, W)
    m = u[k][0]
    A = operator(H, W, T)
    rhs = -(A[f][:, k] @ (u[k] - m))
    out = u.copy()
    out[f] = (spl.spsolve(A[f][:, f].tocsc(), rhs) if rhs.any() else np.zeros(int(f.sum()))) + m
    return out.reshape(H, W)


def distance_mask(grid, data, radius):
    """grid (float32) with NaN wherever no non-NaN node of data lies within `radius` nodes (Euclidean, integers)"""
    grid, data = np.asarray(grid, dtype=np.float32), np.asarray(data)
    H, W = data.shape
    valid = ~np.isnan(data)
    keep = np.zeros((H, W), dtype=bool)
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            if dr * dr + dc * dc > radius * radius:
                continue
            r0, r1, c0, c1 = max(0, dr), min(H, H + dr), max(0, dc), min(W, W + dc)   # targets (r, c) whose source (r - dr, c - dc) exists
            if r0 < r1 and c0 < c1:
                keep[r0:r1, c0:c1] |= valid[r0 - dr:r1 - dr, c0 - dc:c1 - dc]
    return np.where(keep, grid, np.float32(np.nan)).astype(np.float32)


def to_pixel(grid, threshold=0.5):
    """float64 (H - 1, W - 1): Keys (a = -1/2) bicubic interpolation at the cell centres with ghost nodes extrapolated linearly (columns,
    then rows); NaN nodes: the valid nodes' weighted mean if their weight sum + 1e-9 >= threshold, else NaN"""
    g = np.asarray(grid, dtype=np.float64)
    H, W = g.shape
    e = np.empty((H + 2, W + 2))
    e[1:-1, 1:-1] = g
    e[1:-1, 0], e[1:-1, -1] = 2.0 * g[:, 0] - g[:, 1], 2.0 * g[:, -1] - g[:, -2]
    e[0], e[-1] = 2.0 * e[1] - e[2], 2.0 * e[-2] - e[-3]
    w = np.array([-1.0, 9.0, 9.0, -1.0]) / 16.0
    out = np.empty((H - 1, W - 1))
    for r in range(H - 1):
        for c in range(W - 1):
            z = e[r:r + 4, c:c + 4]
            ww = np.outer(w, w)
            ok = ~np.isnan(z)
            if ok.all():
                out[r, c] = (ww * z).sum()
            else:
                ws = ww[ok].sum()
                out[r, c] = (ww[ok] * z[ok]).sum() / ws if ws + 1e-9 >= threshold else np.nan
    return out
