"""An independent restatement of the overview definition ("Overviews"): one Python loop per pixel, np.float32 scalars,
no code shared with `geotiff.overview_pyramid`.  Slow on purpose; the tests use it on small planes, once per module.

Level k + 1 from level k alone: H' = ceil(H / 2), W' = ceil(W / 2); pixel (r, c) covers rows 2r, 2r + 1 and columns 2c, 2c + 1 as far
as they exist; a sample is valid unless it is NaN or equals float32(nodataval) (float32 files) / equals int(nodataval) (int16 files);
s = (a00 + a01) + (a10 + a11) in float32 with +0.0 for samples that are invalid or do not exist; m = s / float32(n); n == 0: nodata;
int16 files: rint(m), ties to even, and the next level is made from the rounded samples."""
import numpy as np

POS_ZERO = np.float32(0.0)


def _valid(v, integer, nodataval):
    if integer:
        return int(v) != int(nodataval)
    return not (np.isnan(v) or v == np.float32(nodataval))


def halve(level, nodataval):
    """(the next level, counts[n] = the number of windows with n valid samples, n = 0..4)"""
    integer = level.dtype.kind == "i"
    H, W = level.shape
    out = np.empty(((H + 1) // 2, (W + 1) // 2), dtype=level.dtype)
    counts = [0] * 5
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(out.shape[0]):
            for c in range(out.shape[1]):
                term = []
                n = 0
                for rr in (2 * r, 2 * r + 1):
                    for cc in (2 * c, 2 * c + 1):
                        if rr < H and cc < W and _valid(level[rr, cc], integer, nodataval):
                            term.append(np.float32(level[rr, cc]))
                            n += 1
                        else:
                            term.append(POS_ZERO)
                counts[n] += 1
                if n == 0:
                    out[r, c] = int(nodataval) if integer else np.float32(nodataval)
                    continue
                s = np.float32(np.float32(term[0] + term[1]) + np.float32(term[2] + term[3]))
                m = np.float32(s / np.float32(n))
                out[r, c] = int(np.rint(m)) if integer else m
    return out, counts


def pyramid(band, levels, nodataval):
    """(the list of the levels 1 .. levels, the summed window counts per n)"""
    out, total, level = [], [0] * 5, np.asarray(band)
    for _ in range(levels):
        level, counts = halve(level, nodataval)
        out.append(level)
        total = [a + b for a, b in zip(total, counts)]
    return out, total


def max_levels(H, W):
    n = 0
    while H > 1 or W > 1:
        H, W, n = (H + 1) // 2, (W + 1) // 2, n + 1
    return n


def branch_plane(H, W, dtype, nodataval, seed=0):
    """A plane of `dtype` built to reach every branch of the definition at whatever shape it has: noise, blocks and isolated samples
    of nodata (windows with 0 .. 4 valid samples), NaN and -0.0 (float32), +-32767, and values whose means end in .5 after / 2 and
    / 4 in both signs and in a third after / 3 (int16: the ties of rint)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    a = rng.integers(-3000, 3000, (H, W)).astype(np.float32)
    if np.dtype(dtype).kind == "f":
        a += rng.random((H, W), dtype=np.float32)
    flat = a.reshape(-1)
    # 2 x 2 patterns laid over the plane's windows, cycled: [a00, a01, a10, a11], None = nodata
    nd = None
    patterns = [[1, 2, nd, nd], [-1, -2, nd, nd], [1, 1, 1, 2], [-1, -1, -1, -2], [1, 1, 1, 3], [-1, -1, -1, -3], [3, 4, nd, nd],
                [-3, -4, nd, nd], [1, 1, 2, nd], [-1, -1, -2, nd], [nd, nd, nd, nd], [nd, 7, nd, nd], [32767, 32767, 32767, 32767],
                [-32767, -32767, -32767, -32767], [32767, nd, 32767, 32766], [5, nd, nd, 8], [2, 3, 2, 3], [-2, -3, -2, -3]]
    k = 0
    for r in range(0, H, 2):
        for c in range(0, W, 2):
            if (r // 2 + c // 2) % 2 == 0:
                p = patterns[k % len(patterns)]
                k += 1
                for i, (rr, cc) in enumerate(((r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1))):
                    if rr < H and cc < W:
                        a[rr, cc] = nodataval if p[i] is None else p[i]
    if H >= 8 and W >= 8:   # an 8 x 8 block of nodata: empty windows two levels down
        a[:8, :8] = nodataval
    if np.dtype(dtype).kind == "f" and flat.size >= 6:
        flat[flat.size // 2] = np.nan
        flat[flat.size // 3] = -0.0
        if H >= 4 and W >= 8:   # a window of -0.0 alone, one of -0.0 beside nodata, one of NaN alone
            r, c = 2 * ((H - 1) // 4), 2 * ((W - 1) // 4)
            a[r:r + 2, c:c + 2] = -0.0
            a[r:r + 2, c + 2:c + 4] = np.float32([[-0.0, nodataval], [nodataval, nodataval]])
            a[H - 2:, :2] = np.nan
    with np.errstate(invalid="ignore"):
        return a.astype(dtype)
