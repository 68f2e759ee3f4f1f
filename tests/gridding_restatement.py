"""Float64 NumPy restatement of the gridding semantics (DESIGN.md "Gridding point clouds"; dbm_points_polar_stereographic,
dbm_points_region, dbm_points_blockmedian in include/dbm.h).  Not collected by pytest: tests/test_gridding_host.py pins it to published
and hand-computed answers and to pandas, tests/test_gpu_gridding.py holds the kernels to it."""
import numpy as np

EPSG3031 = (6378137.0, 298.257223563, -71.0, 0.0, 0.0, 0.0)
_RAD = np.pi / 180.0


def _t(lat_deg, e):
    es = e * np.sin(lat_deg * _RAD)
    # tan(pi/4 + phi/2) with the half angle formed in degrees: exactly 0 at the pole
    return np.tan((45.0 + 0.5 * lat_deg) * _RAD) / ((1.0 + es) / (1.0 - es)) ** (0.5 * e)


def projection_constants(proj):
    """e, C = sqrt((1+e)^(1+e) (1-e)^(1-e)), t_F, m_F, k0 of EPSG method 9829 variant B (Guidance Note 7-2)"""
    a, rf, lat_f = float(proj[0]), float(proj[1]), float(proj[2])
    f = 1.0 / rf
    e = np.sqrt(2.0 * f - f * f)
    cc = np.sqrt((1.0 + e) ** (1.0 + e) * (1.0 - e) ** (1.0 - e))
    sf = np.sin(lat_f * _RAD)
    t_f = float(_t(np.float64(lat_f), e))
    m_f = np.cos(lat_f * _RAD) / np.sqrt(1.0 - e * e * sf * sf)
    k0 = 1.0 if lat_f == -90.0 else m_f * cc / (2.0 * t_f)
    return {"a": a, "e": float(e), "C": float(cc), "t_F": t_f, "m_F": float(m_f), "k0": float(k0)}


def polar_stereographic(points, proj=EPSG3031, intermediates=False):
    """(n, ncol) longitude, latitude[, ...] in degrees -> easting, northing[, ...]; non-finite coordinates give NaN, NaN"""
    pts = np.array(points, dtype=np.float64, ndmin=2)
    k = projection_constants(proj)
    lon, lat = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = _t(lat, k["e"])
        rho = (2.0 * k["a"] * k["k0"] / k["C"]) * t
        dl = lon * _RAD - float(proj[3]) * _RAD
        E = float(proj[4]) + rho * np.sin(dl)
        N = float(proj[5]) + rho * np.cos(dl)
    bad = ~(np.isfinite(lon) & np.isfinite(lat))
    E[bad] = np.nan
    N[bad] = np.nan
    out = pts.copy()
    out[:, 0], out[:, 1] = E, N
    if intermediates:
        return out, dict(k, t=t, rho=rho)
    return out


def finite_rows(points):
    pts = np.asarray(points, dtype=np.float64)
    return np.isfinite(pts[:, :3]).all(axis=1)


def region(points, inc):
    """({floor(xmin/inc) inc, ceil(xmax/inc) inc, floor(ymin/inc) inc, ceil(ymax/inc) inc}, count) over the rows with finite x, y[, z]"""
    pts = np.asarray(points, dtype=np.float64)
    ok = finite_rows(pts)
    if not ok.any():
        return np.full(4, np.nan), 0
    x, y = pts[ok, 0], pts[ok, 1]
    inc = float(inc)
    return np.array([np.floor(x.min() / inc) * inc, np.ceil(x.max() / inc) * inc, np.floor(y.min() / inc) * inc,
                     np.ceil(y.max() / inc) * inc]), int(ok.sum())


def block_shape(region4, inc):
    xmin, xmax, ymin, ymax = (float(v) for v in region4)
    return int(np.rint((ymax - ymin) / inc)) + 1, int(np.rint((xmax - xmin) / inc)) + 1


def north_edge(region4, inc):
    """ymax fitted to the increment (+e): the region's own when the spacing divides it"""
    H, _ = block_shape(region4, inc)
    ymin, ymax = float(region4[2]), float(region4[3])
    span = float(H - 1) * float(inc)
    return ymax if span == ymax - ymin else ymin + span


def assign(points, region4, inc):
    """block index (row-major from the north-west node) of every row, -1 for dropped rows"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    H, W = block_shape(region4, inc)
    inc = float(inc)
    xmin, y0 = float(region4[0]), north_edge(region4, inc)
    ok = finite_rows(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.floor((pts[:, 0] - xmin) / inc + 0.5)
        row = np.floor((y0 - pts[:, 1]) / inc + 0.5)
        ok &= (col >= 0) & (col < W) & (row >= 0) & (row < H)
    blk = np.full(len(pts), -1, dtype=np.int64)
    blk[ok] = row[ok].astype(np.int64) * W + col[ok].astype(np.int64)
    return blk


def _okey(v):
    """order-preserving unsigned image of float64: -0.0 sorts before +0.0"""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def _median(v):
    """np.median's value -- the middle one, or 0.5 (lo + hi) -- in the total order of _okey (np.median leaves the sign of a zero
    median among zeros of both signs to its partition)"""
    s = v[np.argsort(_okey(v), kind="stable")]
    k = len(s)
    return s[k // 2] if k % 2 else 0.5 * (s[k // 2 - 1] + s[k // 2])


def blockmedian(points, region4, inc):
    """(table (m, 3), float32 raster (H, W) with NaN in empty blocks, int32 counts (H, W))"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    H, W = block_shape(region4, inc)
    blk = assign(pts, region4, inc)
    counts = np.bincount(blk[blk >= 0], minlength=H * W).astype(np.int32)
    order = np.argsort(blk, kind="stable")
    order = order[blk[order] >= 0]
    ids = np.flatnonzero(counts)
    table = np.empty((len(ids), 3), dtype=np.float64)
    at = 0
    for j, b in enumerate(ids):
        rows = pts[order[at:at + counts[b]]]
        at += counts[b]
        for c in range(3):
            table[j, c] = _median(rows[:, c])
    grid = np.full(H * W, np.nan, dtype=np.float32)
    with np.errstate(over="ignore"):
        grid[ids] = table[:, 2].astype(np.float32)
    return table, grid.reshape(H, W), counts.reshape(H, W)
