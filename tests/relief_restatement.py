"""Independent NumPy-only restatements of DESIGN.md 6n (colour relief, hillshade, PNG from HBM); no code shared with
`deepbedmap_amd.relief`.  Scalar float64 arithmetic, one Python loop per pixel where a rule is per pixel: slow on purpose, the tests
use them on small planes and compute every reference once per module.

Table: edges E_0 < ... < E_n, slice i with colours c0_i, c1_i, and B / F / N.
make_cpt: E_i = lo + (e_i - e_0) / (e_n - e_0) * (hi - lo), ends exact; hinge: below the master's hinge onto [lo, h], above onto [h, hi];
discrete: band j = [lo + j inc, lo + (j + 1) inc), its colour the continuous table at E_j + (E_{j+1} - E_j) / 2, floor(u + 0.5).
Pixel: NaN -> N (alpha 0); v < E_0 -> B; v > E_n -> F; else i = the largest index <= n - 1 with E_i <= v, t = (v - E_i) / (E_{i+1} - E_i),
u = c0 + (c1 - c0) * t; shaded: I = k atan((g - mean) / sigma) where g is defined else 0, I >= 0: u + (255 - u) I, I < 0: u + u I; byte =
floor(u' + 0.5) clamped.  g = -(dx sin_a + (dy aspect) cos_a), central differences halved, one-sided ones not, defined where the four
samples read are finite and H, W >= 2.
PNG: filters 0 / 1 / 2 from the raw image, bands of rows as segments of one zlib stream, Adler-32s joined."""
import bisect
import functools
import math
import os
import struct
import zlib

import numpy as np

ADLER = 65521


# ---- tables ----
def parse_cpt(path):
    """(edges, colours (n, 2, 3), B, F, N, hinge) of a GMT >= 5 RGB table, as plain lists."""
    edges, colours, hinge = [], [], None
    bfn = {"B": [0, 0, 0], "F": [255, 255, 255], "N": [128, 128, 128]}
    for line in open(path):
        line = line.strip()
        if line.startswith("#"):
            if "HINGE" in line and "=" in line:
                hinge = float(line.split("=")[1])
            continue
        if not line:
            continue
        tok = line.split()
        if tok[0] in bfn:
            bfn[tok[0]] = [int(x) for x in tok[1].split("/")]
            continue
        if not edges:
            edges.append(float(tok[0]))
        assert float(tok[0]) == edges[-1]
        edges.append(float(tok[2]))
        colours.append([[int(x) for x in tok[1].split("/")], [int(x) for x in tok[3].split("/")]])
    return edges, colours, bfn["B"], bfn["F"], bfn["N"], hinge


def stretch(master_edges, lo, hi, hinge=None, master_hinge=0.0):
    e, n = [float(x) for x in master_edges], len(master_edges) - 1
    out = []
    for i, x in enumerate(e):
        if i == 0:
            out.append(float(lo))
        elif i == n:
            out.append(float(hi))
        elif hinge is None:
            out.append(lo + (x - e[0]) / (e[n] - e[0]) * (hi - lo))
        elif x == master_hinge:
            out.append(float(hinge))
        elif x < master_hinge:
            out.append(lo + (x - e[0]) / (master_hinge - e[0]) * (hinge - lo))
        else:
            out.append(hinge + (x - master_hinge) / (e[n] - master_hinge) * (hi - hinge))
    return out


def colour_u(edges, colours, B, F, v):
    """The three float64 channel values before rounding of the finite-or-infinite value v."""
    n = len(edges) - 1
    if v < edges[0]:
        return [float(x) for x in B]
    if v > edges[n]:
        return [float(x) for x in F]
    i = min(max(bisect.bisect_right(edges, v) - 1, 0), n - 1)   # the largest index <= n - 1 with E_i <= v
    t = (v - edges[i]) / (edges[i + 1] - edges[i])
    return [float(colours[i][0][ch]) + (float(colours[i][1][ch]) - float(colours[i][0][ch])) * t for ch in range(3)]


def discrete(edges, colours, B, F, lo, hi, inc):
    nb = int(round((hi - lo) / inc))
    D = [lo + j * inc for j in range(nb + 1)]
    D[0], D[nb] = float(lo), float(hi)
    cols = []
    for j in range(nb):
        u = colour_u(edges, colours, B, F, D[j] + (D[j + 1] - D[j]) * 0.5)
        c = [int(math.floor(x + 0.5)) for x in u]
        cols.append([c, c])
    return D, cols


# ---- gradient, statistics, shading ----
def gradient(z, sin_a, cos_a, aspect):
    """(g float64 (H, W), defined bool (H, W)) of the float32 plane z."""
    H, W = z.shape
    g = np.zeros((H, W))
    ok = np.zeros((H, W), dtype=bool)
    if H < 2 or W < 2:
        return g, ok
    for r in range(H):
        ru, rd = max(r - 1, 0), min(r + 1, H - 1)
        sy = 0.5 if rd - ru == 2 else 1.0
        for c in range(W):
            cl, cr = max(c - 1, 0), min(c + 1, W - 1)
            sx = 0.5 if cr - cl == 2 else 1.0
            zl, zr, zu, zd = float(z[r, cl]), float(z[r, cr]), float(z[ru, c]), float(z[rd, c])
            if not all(math.isfinite(x) for x in (zl, zr, zu, zd)):
                continue
            dx = (zr - zl) * sx
            dy = (zu - zd) * sy
            g[r, c] = -(dx * sin_a + (dy * aspect) * cos_a)
            ok[r, c] = True
    return g, ok


def stats(g, ok):
    """(n, mean, sigma) by math.fsum: the exactly rounded sums, the reference the device's fixed-order sums are measured against."""
    values = [float(x) for x in g[ok]]
    n = len(values)
    if n == 0:
        return 0, 0.0, 0.0
    mean = math.fsum(values) / n
    if n < 2:
        return n, mean, 0.0
    return n, mean, math.sqrt(math.fsum((x - mean) * (x - mean) for x in values) / (n - 1))


def relief(z, edges, colours, B, F, N, channels, shade=None, g=None, ok=None):
    """(image uint8 (H, W, channels), pre float64 (H, W, 3): the values before floor(. + 0.5), NaN at N pixels).
    shade = (k, mean, sigma) or None."""
    H, W = z.shape
    img = np.zeros((H, W, channels), dtype=np.uint8)
    pre = np.full((H, W, 3), np.nan)
    for r in range(H):
        for c in range(W):
            if np.isnan(z[r, c]):
                img[r, c, :3] = N
                continue
            u = colour_u(edges, colours, B, F, float(z[r, c]))
            I = 0.0
            if shade is not None and ok[r, c]:
                I = shade[0] * math.atan((g[r, c] - shade[1]) / shade[2])
            for ch in range(3):
                w = u[ch] + ((255.0 - u[ch]) * I if I >= 0.0 else u[ch] * I)
                pre[r, c, ch] = w
                img[r, c, ch] = int(min(255.0, max(0.0, math.floor(w + 0.5))))
            if channels == 4:
                img[r, c, 3] = 255
    return img, pre


def near_tie(pre):
    """True where a byte may legitimately differ between two correct atan implementations: its pre-rounding value lies within 1e-9 of
    some k + 0.5."""
    with np.errstate(invalid="ignore"):
        frac = pre - np.floor(pre)
        return np.abs(frac - 0.5) <= 1e-9


# ---- PNG ----
def filtered_scanlines(image, filter):
    """The bytes a PNG's zlib stream holds for the uint8 image (H, W, channels): per row the filter byte and the filtered row."""
    H, W, ch = image.shape
    raw = image.reshape(H, W * ch).astype(np.int64)
    out = np.zeros((H, W * ch + 1), dtype=np.uint8)
    out[:, 0] = filter
    for r in range(H):
        for x in range(W * ch):
            if filter == 1:
                prior = raw[r, x - ch] if x >= ch else 0
            elif filter == 2:
                prior = raw[r - 1, x] if r > 0 else 0
            else:
                prior = 0
            out[r, x + 1] = (raw[r, x] - prior) % 256
    return out


def adler32_combine(a1, a2, len2):
    """zlib's adler32_combine, restated from its definition: both halves are sums modulo 65521."""
    s1, s2 = a1 & 0xFFFF, a1 >> 16
    t1, t2 = a2 & 0xFFFF, a2 >> 16
    return (((s2 + t2 + len2 * (s1 - 1)) % ADLER) << 16) | ((s1 + t1 - 1) % ADLER)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def stitched_png(image, filter, band_rows, idat_bytes=1 << 20):
    """A PNG whose zlib stream is stitched from bands deflated by zlib itself (raw deflate, Z_SYNC_FLUSH between bands, Z_FINISH at
    the end): proves the container and the stitching only -- the package's bytes come from its own encoder."""
    H, W, ch = image.shape
    lines = filtered_scanlines(image, filter)
    stream, adler = b"\x78\x01", 1
    for r0 in range(0, H, band_rows):
        band = lines[r0:r0 + band_rows].tobytes()
        enc = zlib.compressobj(6, zlib.DEFLATED, -15)
        stream += enc.compress(band) + enc.flush(zlib.Z_FINISH if r0 + band_rows >= H else zlib.Z_SYNC_FLUSH)
        adler = adler32_combine(adler, zlib.adler32(band), len(band))
    stream += struct.pack(">I", adler)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0))
    for at in range(0, len(stream), idat_bytes):
        out += chunk(b"IDAT", stream[at:at + idat_bytes])
    return out + chunk(b"IEND", b"")


# ---- inputs ----
def sample_plane(H, W, lo=-4500.0, hi=4500.0, edge=None, seed=0):
    """Smooth relief plus noise spanning beyond [lo, hi], with a NaN block, +inf, -inf, the exact values lo, hi, 0 and `edge`, and
    values below lo and above hi -- each only where the plane has room."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    z = (0.45 * (hi - lo) * np.sin(x / 7.0 + 0.3) * np.cos(y / 5.0) + 0.5 * (hi + lo) + rng.standard_normal((H, W)) * 0.02 * (hi - lo))
    z = z.astype(np.float32)
    flat = z.reshape(-1)
    specials = [lo, hi, 0.0, hi + 0.25 * (hi - lo), lo - 0.25 * (hi - lo), np.inf, -np.inf] + ([edge] if edge is not None else [])
    if flat.size >= 4 * len(specials):
        for i, v in enumerate(specials):
            flat[(i * 37 + 11) % flat.size] = v
    elif flat.size > 1:
        for i, v in enumerate(specials[:flat.size - 1]):
            flat[i + 1] = v
    if H >= 12 and W >= 12:
        z[5:9, 6:11] = np.nan
    return z


# ---- the cases the host and the GPU tests share ----
GOLDEN_CPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oleron.cpt")
SHAPES = [(1, 1), (1, 7), (7, 1), (37, 29), (150, 210)]
WIDE_N = 2048


def wide_master():
    """(edges, colours) of a 2048-slice master built in code: edges 0 .. 2048, colours that change with every slice."""
    def colour(k):
        return [(7 * k) % 256, (13 * k + 5) % 256, (k // 8) % 256]
    return [float(k) for k in range(WIDE_N + 1)], [[colour(k), colour(k + 1)] for k in range(WIDE_N)]


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (edges, colours, B, F, N, lo, hi, a float32-exact interior value worth sampling) by the restatement alone."""
    e, c, B, F, N, h = parse_cpt(GOLDEN_CPT)
    out = {}
    cont = stretch(e, -4500.0, 4500.0)
    out["oleron"] = (cont, c, B, F, N, -4500.0, 4500.0, float(np.float32(cont[100])))
    out["hinge"] = (stretch(e, -2000.0, 4500.0, hinge=0.0, master_hinge=h), c, B, F, N, -2000.0, 4500.0, 0.0)
    D, cols = discrete(stretch(e, -2800.0, 2800.0), c, B, F, -2800.0, 2800.0, 200.0)
    out["bands"] = (D, cols, cols[0][0], cols[-1][1], N, -2800.0, 2800.0, 600.0)
    out["one"] = ([-4500.0, 4500.0], [[[0, 0, 0], [255, 255, 255]]], [0, 0, 0], [255, 255, 255], [128, 128, 128], -4500.0, 4500.0, None)
    we, wc = wide_master()
    out["wide"] = (stretch(we, -4500.0, 4500.0), wc, [1, 2, 3], [250, 251, 252], [9, 8, 7], -4500.0, 4500.0, -2250.0)
    return out


@functools.lru_cache(maxsize=None)
def plane_of(name, shape):
    t = tables()[name]
    return sample_plane(shape[0], shape[1], t[5], t[6], t[7])


SHADING = (-45.0, 1.0)   # the reference's "+d"


def shading_constants():
    a = math.radians(SHADING[0])
    return math.sin(a), math.cos(a), SHADING[1] * (2.0 / math.pi)


@functools.lru_cache(maxsize=None)
def gradient_of(name, shape):
    sin_a, cos_a, _ = shading_constants()
    return gradient(plane_of(name, shape), sin_a, cos_a, 1.0)


@functools.lru_cache(maxsize=None)
def reference(name, shape, shade=None):
    """(image (H, W, 4), pre) of the case; shade = None or (mean, sigma): the statistics the shading is normalised by."""
    t = tables()[name]
    if shade is None:
        return relief(plane_of(name, shape), t[0], t[1], t[2], t[3], t[4], 4)
    g, ok = gradient_of(name, shape)
    return relief(plane_of(name, shape), t[0], t[1], t[2], t[3], t[4], 4, (shading_constants()[2], shade[0], shade[1]), g, ok)
