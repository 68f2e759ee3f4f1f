"""Two independent referees of the perspective view, in NumPy; not collected by pytest.

`rule` restates the pixel rule: vectorised over the pixels, it loops over ALL cells and ALL wall segments -- no blocks, no clipping, no
early stop, no order.  Every operation is one IEEE float64 operation in the order DESIGN.md 6o writes it, so the bytes and the ids are
compared with no tolerance.  Its cost is pixels x cells, so it referees the small planes; the large plane is refereed by `verify`.

`verify` takes ids from anywhere and checks them against the geometry, with tolerances and for every pixel:
  * the reported triangle (or a wall) is met by the ray: q* is recomputed from the triangle's plane, the point lies in the triangle within
    1e-9 (1 + |q*|) and on the ray within 1e-9 (1 + |h|);
  * nothing lies in front of it: the breakpoints of the surface profile along the ray with q >= q* + 1e-9 (all of them for a miss) --
    the crossings of integer rows, columns and cell diagonals inside the footprint -- are sorted; between two neighbours the profile is
    linear, so f = ray height - surface height is evaluated at both ends of every such piece from the piece's own triangle and
    classified as above (f > tol), below (f < -tol) or touching, tol = 1e-9 (1 + |h|).  Along a run of pieces with no hole between them
    the classes must never change from above to below or back: that would be a crossing in front of the reported one.  For a ray that
    comes from above the surface this is "ray height >= surface height - tol at every breakpoint"; a ray that entered under the surface
    through an open side (no facade) legitimately runs below it, and may meet it from below.  Holes end a run.
  * with a facade, no wall in front is pierced: at its crossing with q >= q* + 1e-9 the ray height must not lie strictly (by tol) between
    0 and the boundary profile.
"""
import numpy as np

SHAPES = [(2, 2), (1, 5), (5, 1), (37, 29), (150, 210)]
SMALL = [(2, 2), (1, 5), (5, 1), (37, 29)]
VIEWS = [(202.5, 60.0), (0.0, 60.0), (90.0, 30.0), (45.0, 35.0), (315.0, 1.0), (135.0, 89.0)]
LEVEL = -1400.0
LEVEL_ABOVE = 2600.0          # above every sample
PIXEL_SIZE = 250.0
FACADE = (128, 128, 128, 255)
BACKGROUND = (1, 2, 3, 0)


def plane_of(shape):
    """A seeded DEM at -2500 .. 2500 m, float32: long waves plus roughness; the 37 x 29 plane has a 5 x 4 NaN patch, a NaN on the
    boundary and a +inf and a -inf node."""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    r, c = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 1400.0 * np.sin(0.11 * r + 0.3) * np.cos(0.07 * c - 0.2) + 700.0 * np.sin(0.031 * (r + 2.0 * c)) + 300.0 * rng.standard_normal((H, W))
    z = np.clip(z, -2500.0, 2500.0).astype(np.float32)
    if shape == (37, 29):
        z[10:15, 8:12] = np.nan
        z[0, 20] = np.nan
        z[36, 3] = np.nan
        z[22, 17] = np.inf
        z[30, 9] = -np.inf
    return z


def drape_of(shape, channels):
    """A seeded uint8 drape (H, W, channels): smooth ramps plus noise; a fourth channel holds bytes that must not be read."""
    H, W = shape
    rng = np.random.default_rng(7 * H + 13 * W + channels)
    r, c = np.mgrid[0:H, 0:W]
    base = np.stack([(5 * r + 3 * c) % 256, (255 - 2 * r + c) % 256, (r * c) % 256] + ([(7 * r) % 256] if channels == 4 else []), axis=2)
    return ((base + rng.integers(0, 40, base.shape)) % 256).astype(np.uint8)


def rays(values, Wo, Ho):
    sin_a, cos_a, sin_e, tan_e, level, zfac, sx0, sy0, step = (float(v) for v in values)
    sx = sx0 + (np.arange(Wo, dtype=np.float64) + 0.5) * step
    sy = sy0 - (np.arange(Ho, dtype=np.float64) + 0.5) * step
    t = sy / sin_e
    SX, T = np.meshgrid(sx, t)
    a, b, c, d = SX * cos_a, T * sin_a, SX * sin_a, T * cos_a
    ox = (-a) - b
    oy = -(c - d)
    return ox.ravel(), oy.ravel(), sin_a, -cos_a


def _slab(o, d, k0, k1, lo, hi):
    if d != 0.0:
        q1, q2 = (k0 - o) / d, (k1 - o) / d
        return np.maximum(lo, np.minimum(q1, q2)), np.minimum(hi, np.maximum(q1, q2)), np.ones(o.shape, dtype=bool)
    return lo, hi, (k0 <= o) & (o <= k1)


def _take(best_q, best_id, best_al, best_be, sel, q, ident, al, be):
    better = (q > best_q[sel]) | ((q == best_q[sel]) & (ident < best_id[sel]))
    at = sel[better]
    best_q[at], best_id[at], best_al[at], best_be[at] = q[better], ident, al[better], be[better]


def rule(z, drape, values, Wo, Ho, facade, background):
    """(image uint8 (Ho, Wo, 4), ids int32 (Ho, Wo)) by DESIGN.md 6o, over all cells and all wall segments."""
    z = np.asarray(z, dtype=np.float32)
    H, W = z.shape
    sin_a, cos_a, sin_e, tan_e, level, zfac = (float(v) for v in values[:6])
    ox, oy, dx, dy = rays(values, Wo, Ho)
    P = ox.size
    best_q, best_id = np.full(P, -np.inf), np.full(P, -1, dtype=np.int64)
    best_al, best_be = np.zeros(P), np.zeros(P)
    everyone = np.arange(P)
    with np.errstate(all="ignore"):
        h = (z.astype(np.float64) - level) * zfac
        fin = np.isfinite(z)
        if H >= 2 and W >= 2:
            if facade is not None:
                walls = [(z[0], h[0], 0.0, ox, dx, oy, dy), (z[H - 1], h[H - 1], float(H - 1), ox, dx, oy, dy),
                         (z[:, 0], h[:, 0], 0.0, oy, dy, ox, dx), (z[:, W - 1], h[:, W - 1], float(W - 1), oy, dy, ox, dx)]
                for zs, hs, w, ou, du, ov, dv in walls:
                    if dv == 0.0:
                        continue
                    q = (w - ov) / dv
                    u = ou + q * du
                    hr = q * tan_e
                    for k in range(zs.size - 1):
                        if not (np.isfinite(zs[k]) and np.isfinite(zs[k + 1])):
                            continue
                        p = hs[k] + (hs[k + 1] - hs[k]) * (u - float(k))
                        ok = (float(k) <= u) & (u <= float(k + 1)) & (np.minimum(p, 0.0) <= hr) & (hr <= np.maximum(p, 0.0))
                        sel = everyone[ok]
                        _take(best_q, best_id, best_al, best_be, sel, q[ok], -2, np.zeros(sel.size), np.zeros(sel.size))
            for r in range(H - 1):
                for c in range(W - 1):
                    if not (fin[r, c] and fin[r, c + 1] and fin[r + 1, c] and fin[r + 1, c + 1]):
                        continue
                    x0, x1, y0, y1 = float(c), float(c + 1), float(r), float(r + 1)
                    lo, hi, okx = _slab(ox, dx, x0, x1, np.full(P, -np.inf), np.full(P, np.inf))
                    lo, hi, oky = _slab(oy, dy, y0, y1, lo, hi)
                    met = everyone[okx & oky & (lo <= hi)]
                    if met.size == 0:
                        continue
                    lo, hi, mx, my = lo[met], hi[met], ox[met], oy[met]
                    ha, hb, hd, he = h[r, c], h[r, c + 1], h[r + 1, c], h[r + 1, c + 1]
                    ident = 2 * (r * (W - 1) + c)
                    side0 = (mx + my) - float(c + r)
                    al0, be0, s1, s2 = mx - x0, my - y0, hb - ha, hd - ha
                    num = (ha + s1 * al0) + s2 * be0
                    den = (tan_e - s1 * dx) - s2 * dy
                    if den != 0.0:
                        q = num / den
                        al, be = al0 + q * dx, be0 + q * dy
                        ok = (lo <= q) & (q <= hi) & (side0 + q * (dx + dy) <= 1.0)
                        _take(best_q, best_id, best_al, best_be, met[ok], q[ok], ident, al[ok], be[ok])
                    al0, be0, s1, s2 = x1 - mx, y1 - my, hd - he, hb - he
                    num = (he + s1 * al0) + s2 * be0
                    den = (tan_e + s1 * dx) + s2 * dy
                    if den != 0.0:
                        q = num / den
                        al, be = al0 - q * dx, be0 - q * dy
                        ok = (lo <= q) & (q <= hi) & (side0 + q * (dx + dy) > 1.0)
                        _take(best_q, best_id, best_al, best_be, met[ok], q[ok], ident + 1, al[ok], be[ok])
    image = np.empty((P, 4), dtype=np.uint8)
    image[:] = np.asarray(background, dtype=np.uint8)
    if facade is not None:
        image[best_id == -2] = np.asarray(facade, dtype=np.uint8)
    hit = np.flatnonzero(best_id >= 0)
    if hit.size:
        cell, t = best_id[hit] >> 1, best_id[hit] & 1
        r, c = cell // (W - 1), cell % (W - 1)
        n0 = np.where(t == 0, r * W + c, (r + 1) * W + c + 1)
        n1 = np.where(t == 0, r * W + c + 1, (r + 1) * W + c)
        n2 = np.where(t == 0, (r + 1) * W + c, r * W + c + 1)
        flat = np.asarray(drape, dtype=np.uint8).reshape(H * W, -1).astype(np.float64)
        for ch in range(3):
            c0, c1, c2 = flat[n0, ch], flat[n1, ch], flat[n2, ch]
            u = (c0 + (c1 - c0) * best_al[hit]) + (c2 - c0) * best_be[hit]
            image[hit, ch] = np.clip(np.floor(u + 0.5), 0, 255).astype(np.uint8)
        image[hit, 3] = 255
    return image.reshape(Ho, Wo, 4), best_id.astype(np.int32).reshape(Ho, Wo)


# ---- the verifier ----
def _triangle_plane(h, H, W, x, y):
    """For points (x, y) inside the footprint: (valid, h0, gx, gy, x_ref, y_ref) of the triangle that holds each -- its height is
    h0 + gx (x - x_ref) + gy (y - y_ref) -- valid only where the cell has four finite nodes."""
    c = np.clip(np.floor(x), 0, W - 2).astype(np.int64)
    r = np.clip(np.floor(y), 0, H - 2).astype(np.int64)
    ha, hb, hd, he = h[r, c], h[r, c + 1], h[r + 1, c], h[r + 1, c + 1]
    valid = np.isfinite(ha) & np.isfinite(hb) & np.isfinite(hd) & np.isfinite(he)
    upper = (x - c) + (y - r) <= 1.0
    h0 = np.where(upper, ha, he)
    gx = np.where(upper, hb - ha, he - hd)
    gy = np.where(upper, hd - ha, he - hb)
    return valid, h0, gx, gy, np.where(upper, c, c + 1).astype(np.float64), np.where(upper, r, r + 1).astype(np.float64)


def verify(z, values, Wo, Ho, ids, facade_on, chunk=4096):
    """The number of pixels that fail a check, and a list of (pixel, what) for the first few; 0 and [] is a pass."""
    z = np.asarray(z, dtype=np.float32)
    H, W = z.shape
    sin_a, cos_a, sin_e, tan_e, level, zfac = (float(v) for v in values[:6])
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    ox_all, oy_all, dx, dy = rays(values, Wo, Ho)
    failures = []
    if H < 2 or W < 2:
        bad = np.flatnonzero(ids != -1)
        return bad.size, [(int(p), "a plane without cells shows nothing") for p in bad[:5]]
    with np.errstate(all="ignore"):
        h = np.where(np.isfinite(z), (z.astype(np.float64) - level) * zfac, np.nan)
    nbad = 0

    def fail(mask, pixels, what):
        nonlocal nbad
        nbad += int(mask.sum())
        failures.extend((int(p), what) for p in pixels[mask][:3])

    def wall_crossings(ox, oy):
        """per wall: (q, hr, p, p'): the boundary profile where the ray crosses the wall's plane, from the segment that holds the point
        1e-9 before it and from the one 1e-9 after it (the same but within 1e-9 of a node); NaN where there is no wall"""
        out = []
        for hs, w, ou, du, ov, dv in ((h[0], 0.0, ox, dx, oy, dy), (h[H - 1], float(H - 1), ox, dx, oy, dy),
                                      (h[:, 0], 0.0, oy, dy, ox, dx), (h[:, W - 1], float(W - 1), oy, dy, ox, dx)):
            if dv == 0.0:
                continue
            q = (w - ov) / dv
            u = ou + q * du
            inside = (u >= 0.0) & (u <= hs.size - 1.0)
            both = []
            for nudge in (-1e-9, 1e-9):
                k = np.clip(np.floor(u + nudge), 0, hs.size - 2).astype(np.int64)
                both.append(np.where(inside, hs[k] + (hs[k + 1] - hs[k]) * (u - k), np.nan))
            out.append((q, q * tan_e, both[0], both[1]))
        return out

    for start in range(0, ids.size, chunk):
        pix = np.arange(start, min(start + chunk, ids.size))
        ox, oy, ident = ox_all[pix], oy_all[pix], ids[pix]
        with np.errstate(all="ignore"):
            q_star = np.full(pix.size, -np.inf)
            # the reported triangle
            tri = ident >= 0
            cell, t = np.where(tri, ident >> 1, 0), ident & 1
            r, c = cell // (W - 1), cell % (W - 1)
            fail((tri & (r >= H - 1)) | (ident < -2), pix, "an id outside the plane")
            r = np.minimum(r, H - 2)
            ha, hb, hd, he = h[r, c], h[r, c + 1], h[r + 1, c], h[r + 1, c + 1]
            upper = t == 0
            h0, gx, gy = np.where(upper, ha, he), np.where(upper, hb - ha, he - hd), np.where(upper, hd - ha, he - hb)
            xr, yr = np.where(upper, c, c + 1).astype(np.float64), np.where(upper, r, r + 1).astype(np.float64)
            f0 = -(h0 + gx * (ox - xr) + gy * (oy - yr))                 # ray height - surface height at q = 0
            slope = tan_e - gx * dx - gy * dy
            q = -f0 / slope
            x, y = ox + q * dx, oy + q * dy
            fx, fy = x - c, y - r
            tol_p = 1e-9 * (1.0 + np.abs(q))
            hs = h0 + gx * (x - xr) + gy * (y - yr)
            inside = (fx >= -tol_p) & (fx <= 1 + tol_p) & (fy >= -tol_p) & (fy <= 1 + tol_p) & np.where(upper, fx + fy <= 1 + tol_p, fx + fy >= 1 - tol_p)
            on_ray = np.abs(q * tan_e - hs) <= 1e-9 * (1.0 + np.abs(hs))
            fail(tri & ~(np.isfinite(q) & inside & on_ray), pix, "the reported triangle is not met by the ray")
            q_star = np.where(tri, q, q_star)
            # a reported wall: the nearest wall crossing that holds
            walls = wall_crossings(ox, oy)
            wall = ident == -2
            if wall.any():
                fail(wall & (not facade_on), pix, "a wall without a facade")
                q_wall = np.full(pix.size, -np.inf)
                for q, hr, p1, p2 in walls:       # met if either segment at a node holds
                    holds = np.zeros(pix.size, dtype=bool)
                    for p in (p1, p2):
                        tol = 1e-9 * (1.0 + np.abs(p))
                        holds |= (np.minimum(p, 0.0) - tol <= hr) & (hr <= np.maximum(p, 0.0) + tol)
                    q_wall = np.where(holds & (q > q_wall), q, q_wall)
                fail(wall & ~np.isfinite(q_wall), pix, "the reported wall is not met by the ray")
                q_star = np.where(wall, q_wall, q_star)
            q_from = q_star + 1e-9
            # walls in front
            if facade_on:
                for q, hr, p1, p2 in walls:       # pierced only if both segments at a node are
                    pierced = q >= q_from
                    for p in (p1, p2):
                        tol = 1e-9 * (1.0 + np.abs(p))
                        pierced &= (np.minimum(p, 0.0) + tol < hr) & (hr < np.maximum(p, 0.0) - tol)
                    fail(pierced, pix, "a wall in front of the reported hit")
            # the surface profile in front: breakpoints, sorted from the viewer
            cols, rows, diags = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(1, W + H - 2, dtype=np.float64)
            parts = [np.where(np.isfinite(q_from), q_from, np.nan)[:, None]]
            if dx != 0.0:
                parts.append((cols[None, :] - ox[:, None]) / dx)
            if dy != 0.0:
                parts.append((rows[None, :] - oy[:, None]) / dy)
            if dx + dy != 0.0:
                parts.append((diags[None, :] - (ox + oy)[:, None]) / (dx + dy))
            qs = np.concatenate(parts, axis=1)
            X, Y = ox[:, None] + qs * dx, oy[:, None] + qs * dy
            slack = 1e-9 * (1.0 + np.abs(qs))
            keep = (qs >= q_from[:, None]) & (X >= -slack) & (X <= W - 1 + slack) & (Y >= -slack) & (Y <= H - 1 + slack)
            qs = -np.sort(-np.where(keep, qs, -np.inf), axis=1)           # descending; -inf fills the tail
            state = np.zeros(pix.size, dtype=np.int8)
            crossed = np.zeros(pix.size, dtype=bool)
            for k in range(qs.shape[1] - 1):
                qa, qb = qs[:, k], qs[:, k + 1]
                live = np.isfinite(qb)
                if not live.any():
                    break
                qm = np.where(live, qa + (qb - qa) * 0.5, 0.0)
                valid, h0, gx, gy, xr, yr = _triangle_plane(h, H, W, np.clip(ox + qm * dx, 0, W - 1), np.clip(oy + qm * dy, 0, H - 1))
                valid &= live & (qa > qb)
                state = np.where(valid | (qa == qb), state, 0)           # a hole ends the run; a piece of no length does not
                for qe in (qa, qb):
                    hs = h0 + gx * (ox + qe * dx - xr) + gy * (oy + qe * dy - yr)
                    f = qe * tan_e - hs
                    tol = 1e-9 * (1.0 + np.abs(hs))
                    cls = np.where(valid, np.where(f > tol, 1, np.where(f < -tol, -1, 0)), 0).astype(np.int8)
                    crossed |= (cls != 0) & (state != 0) & (cls != state)
                    state = np.where(cls != 0, cls, state)
            fail(crossed, pix, "the surface crosses the ray in front of the reported hit")
    return nbad, failures
