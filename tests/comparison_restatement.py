"""Float64 NumPy restatement of the comparison grids (DESIGN.md "Comparison grids"): the yardstick the GPU entry points
dbm_grid_rescale and dbm_grid_rolling_std are held to.  It imports nothing but NumPy; tests/test_comparison_host.py pins it to
scipy.ndimage (gaussian_filter, zoom) and to a numpy.nanstd brute force on the CPU.

rescale -- the scipy call chain behind current scikit-image's `rescale` / `resize` (reference deepbedmap.py:323-331, 348-356):
  out = round(scale * in) per axis (NumPy round), factor = in / out;
  optional `.astype(np.int32)` (truncation toward zero);
  anti_aliasing: gaussian_filter(sigma = max(0, (factor - 1) / 2), mode="mirror", truncate 4.0), axis 0, then axis 1, sigma 0 skipped;
  zoom(order 1 or 3, mode="mirror", grid_mode=True): output node o samples the input coordinate (o + 0.5) * in / out - 0.5;
  clip to [min, max] of the (cast) input; float64 throughout, rounded to float32 once.
standard_deviation_2d -- reference paper_figures.py:847-867: population standard deviation of the non-NaN nodes of the centred
  window cut at the grid's edges, NaN where the window holds no valid node.
"""
import numpy as np

POLE = np.sqrt(3.0) - 2.0    # the cubic B-spline's pole
START_TERMS = 64             # |POLE| ** 64 = 2.5e-37: the mirror sum's truncation is far below float64 rounding


def output_shape(shape, scale):
    """(out_h, out_w) = round(scale * in), NumPy's round, scale a scalar or one value per axis"""
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
    return tuple(int(v) for v in np.round(s * np.asarray(shape, dtype=np.float64)))


def mirror_index(i, n):
    """index of the whole-sample symmetric extension (d c b | a b c d | c b a): period 2 (n - 1)"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def mirror_coordinate(c, n):
    """scipy's coordinate fold for mode="mirror" (a coordinate outside [0, n - 1] is reflected back into it)"""
    c = np.asarray(c, dtype=np.float64).copy()
    if n <= 1:
        return np.zeros_like(c)
    p = 2.0 * (n - 1)
    lo = c < 0
    v = p * np.trunc(-c[lo] / p) + c[lo]
    c[lo] = np.where(v <= 1 - n, v + p, -v)
    hi = c > n - 1
    v = c[hi] - p * np.trunc(c[hi] / p)
    c[hi] = np.where(v >= n, p - v, v)
    return c


def gaussian_weights(sigma):
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum(), radius


def gaussian_axis0(x, sigma):
    """ndimage.gaussian_filter1d(x, sigma, axis=0, mode="mirror")"""
    if sigma <= 0:
        return x
    w, radius = gaussian_weights(sigma)
    n = x.shape[0]
    rows = np.arange(n)
    out = x * w[radius]
    for k in range(1, radius + 1):
        out = out + (x[mirror_index(rows - k, n)] + x[mirror_index(rows + k, n)]) * w[radius - k]
    return out


def prefilter_axis0(x):
    """ndimage.spline_filter1d(x, order=3, axis=0, mode="mirror"): gain 6, causal and anticausal pass with pole sqrt(3) - 2; the causal
    start value is the sum over the mirrored signal, z^k x[-k], cut after START_TERMS terms"""
    n = x.shape[0]
    z = POLE
    s = 6.0 * x
    c = np.empty_like(s)
    start = np.zeros_like(s[0])
    for k in range(START_TERMS - 1, -1, -1):        # Horner, far terms first
        start = s[int(mirror_index(-k, n))] + z * start
    c[0] = start
    for i in range(1, n):
        c[i] = s[i] + z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * (z / (z * z - 1.0))
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def spline_weights(t, order):
    """the B-spline weights of the nodes floor(c) - order // 2 ... at the fractional part t (scipy's forms)"""
    if order == 1:
        return [1.0 - t, t]
    u = 1.0 - t
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w0 = u * u * u / 6.0
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]


def zoom_axis0(x, out_n, order):
    """one axis of ndimage.zoom(order, mode="mirror", grid_mode=True, prefilter=False) on spline coefficients x"""
    n = x.shape[0]
    c = mirror_coordinate((np.arange(out_n, dtype=np.float64) + 0.5) * (float(n) / float(out_n)) - 0.5, n)
    f = np.floor(c)
    w = spline_weights(c - f, order)
    start = f.astype(np.int64) - order // 2
    out = 0.0
    for k in range(order + 1):
        out = out + x[mirror_index(start + k, n)] * w[k].reshape((-1,) + (1,) * (x.ndim - 1))
    return out


def rescale64(image, scale, order=1, anti_aliasing=True, clip=True, as_int=False):
    """the float64 result before the final rounding"""
    if order not in (1, 3):
        raise ValueError("order must be 1 or 3")
    x = np.asarray(image)
    if x.ndim != 2 or min(x.shape) < 2:
        raise ValueError("image must be (H, W) with H, W >= 2")
    out_h, out_w = output_shape(x.shape, scale)
    if out_h < 1 or out_w < 1:
        raise ValueError("empty output")
    x = (x.astype(np.int32) if as_int else x).astype(np.float64)
    lo, hi = x.min(), x.max()
    if anti_aliasing:
        x = gaussian_axis0(x, max(0.0, (x.shape[0] / out_h - 1.0) / 2.0))
        x = gaussian_axis0(x.T, max(0.0, (x.shape[1] / out_w - 1.0) / 2.0)).T
    if order == 3:
        x = prefilter_axis0(x)
        x = prefilter_axis0(x.T).T
    x = zoom_axis0(x, out_h, order)
    x = zoom_axis0(x.T, out_w, order).T
    return np.clip(x, lo, hi) if clip else x


def rescale(image, scale, order=1, anti_aliasing=True, clip=True, as_int=False):
    return rescale64(image, scale, order, anti_aliasing, clip, as_int).astype(np.float32)


def cubic_bedmap(X_tile):
    """deepbedmap.py:323-332: the interior of the (1, 1, h, w) BEDMAP2 tile as int32, x4, order 3 -> (1, 1, 4 (h - 2), 4 (w - 2))"""
    return rescale(np.asarray(X_tile)[0, 0, 1:-1, 1:-1], 4, order=3, as_int=True)[None, None]


def standard_deviation_2d64(grid, window_length):
    """float64 roughness; sums of the values shifted by one valid value of the window (the centre node, or else the window's first
    valid node in row-major order), so that nothing cancels and a constant window gives exactly 0"""
    if window_length % 2 != 1 or not 1 <= window_length <= 63:
        raise ValueError("window_length must be odd, 1..63")
    g = np.asarray(grid, dtype=np.float64)
    H, W = g.shape
    h = window_length // 2
    pad = np.full((H + 2 * h, W + 2 * h), np.nan)
    pad[h:h + H, h:h + W] = g
    views = [pad[dr:dr + H, dc:dc + W] for dr in range(window_length) for dc in range(window_length)]
    shift = g.copy()
    for v in views:
        shift = np.where(np.isnan(shift), v, shift)
    n = np.zeros((H, W))
    s1 = np.zeros((H, W))
    s2 = np.zeros((H, W))
    for v in views:
        ok = ~np.isnan(v)
        d = np.where(ok, v - shift, 0.0)
        n += ok
        s1 += d
        s2 += d * d
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s1 / n
        var = np.maximum(s2 / n - m * m, 0.0)
        return np.where(n > 0, np.sqrt(var), np.nan)


def standard_deviation_2d(grid, window_length):
    return standard_deviation_2d64(grid, window_length).astype(np.float32)
