"""Rendering the DEM where it lies: colour relief, hillshade and a PNG written from HBM (reference deepbedmap.py:758-775, "Show *the*
DeepBedMap": `gmt.makecpt(cmap="oleron", series=[-4500, 4500])`, `fig.grdimage(..., cmap=True, Q=True)`, `fig.savefig(...)`;
paper_figures.py:81-131, :521-531 plain colour relief, :692-699, :1193-1200 with `shading="+d"`).

The reference hands the GeoTIFF to GMT.  Here the canvas `predict_tiled_resident` left in HBM -- or a level of its overview pyramid --
is coloured by dbm_grid_relief, and the image is filtered and deflated by dbm_png_encode, one wavefront per band of rows; only the
compressed bytes cross PCIe.  Host side: GMT colour tables (`read_cpt`, `make_cpt`), the PNG container (`save_png`, the host writer
of the same bytes; `write_png_resident`; `read_png`), the NumPy statement of the pixel rule (`relief_image_host`) and the public calls
(`relief_image`, `render_dem`).

The rules are this project's own and are stated in DESIGN.md 6n; GMT's pixels are NOT claimed: its HSV illumination, its handling of
hinges from version to version and its dpi resampling are not restated.  The `grdview` 3-D view is perspective.py; axes, text and histograms stay
out of scope.  No CPU fallback: the device calls raise DbmError without a GPU; the host calls (`relief_image_host`, `save_png`, `read_png`,
the colour tables) need none.
"""
import dataclasses
import math
import os
import struct
import zlib

import numpy as np

from . import _lib
from .block_writes import blocks_per_call, deflate_slot, encoded_batches, write_options
from .resident import DeviceArray, GridGeometry, devptr, plane_shape, to_device

MAX_SLICES = 2048                # edges and colours live in LDS (relief.hip)
BAND_BYTES = 128 << 10           # the size `default_band_rows` aims at: DESIGN.md 6n, "Bands"
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPES = {1: 0, 3: 2, 4: 6}   # channels -> PNG colour type (8 bits per sample)
ADLER_MOD = 65521


# ---- colour tables ----
@dataclasses.dataclass(frozen=True, eq=False)
class ColorTable:
    """n slices: `edges` (float64, n + 1, strictly ascending) and `colors` (uint8, 6 n + 9: per slice r, g, b at its lower edge and
    at its upper edge, then the background B (below the table), the foreground F (above it) and the NaN colour N).  `hinge`: the
    master's `# HINGE` value, or None.  The arrays are read-only."""
    edges: np.ndarray
    colors: np.ndarray
    hinge: float = None

    def __post_init__(self):
        edges = np.array(self.edges, dtype=np.float64).ravel()
        colors = np.array(self.colors, dtype=np.uint8).ravel()
        n = edges.size - 1
        if n < 1 or colors.size != 6 * n + 9:
            raise ValueError(f"ColorTable: {edges.size} edges and {colors.size} colour bytes do not make a table (n + 1 and 6 n + 9)")
        if n > MAX_SLICES:
            raise ValueError(f"ColorTable: {n} slices: at most {MAX_SLICES}")
        if not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
            raise ValueError("ColorTable: the edges must be finite and strictly ascending")
        edges.setflags(write=False)
        colors.setflags(write=False)
        object.__setattr__(self, "edges", edges)
        object.__setattr__(self, "colors", colors)

    @property
    def n(self):
        return self.edges.size - 1

    @property
    def slices(self):
        """(n, 2, 3): the colours at the lower and the upper edge of every slice."""
        return self.colors[:6 * self.n].reshape(self.n, 2, 3)

    @property
    def background(self):
        return self.colors[6 * self.n:6 * self.n + 3]

    @property
    def foreground(self):
        return self.colors[6 * self.n + 3:6 * self.n + 6]

    @property
    def nan(self):
        return self.colors[6 * self.n + 6:]


def _table(edges, slices, b, f, n, hinge=None):
    return ColorTable(edges, np.concatenate([np.asarray(slices, dtype=np.uint8).ravel(), np.asarray(b, dtype=np.uint8),
                                             np.asarray(f, dtype=np.uint8), np.asarray(n, dtype=np.uint8)]), hinge)


def grey_cpt(lo=0.0, hi=1.0):
    """The one table the package builds itself: black at lo to white at hi, B black, F white, N 128 grey."""
    return _table([float(lo), float(hi)], [[[0, 0, 0], [255, 255, 255]]], (0, 0, 0), (255, 255, 255), (128, 128, 128))


def _triplet(text, where):
    parts = text.split("/")
    try:
        values = [float(p) for p in parts]
    except ValueError:
        values = None
    if values is None or len(values) != 3 or not all(0 <= v <= 255 for v in values):
        raise ValueError(f"{where}: colour {text!r}: only r/g/b triplets of 0..255 are read (no names, no grey levels, no other model)")
    return [int(math.floor(v + 0.5)) for v in values]


def read_cpt(path):
    """A GMT >= 5 colour table: `#` comments (`# COLOR_MODEL = RGB` is checked, `# HINGE = v` remembered), slice lines
    `z0 r/g/b z1 r/g/b` (a trailing annotation flag L, U, B or a `;label` is ignored) and the optional lines `B`, `F`, `N r/g/b`;
    GMT's defaults stand in for absent ones: black, white, 128 grey.  Refused by a ValueError that names the line: another colour
    model, colour names, gaps or overlaps between slices, a slice whose z does not ascend, more than 2048 slices."""
    path = os.fspath(path)
    edges, slices, hinge = [], [], None
    special = {"B": (0, 0, 0), "F": (255, 255, 255), "N": (128, 128, 128)}
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            where = f"{path}:{number}"
            text = line.strip()
            if not text:
                continue
            if text.startswith("#"):
                key, eq, value = text[1:].partition("=")
                key, value = key.strip().upper(), value.strip()
                if eq and key == "COLOR_MODEL" and value.upper().lstrip("+") != "RGB":
                    raise ValueError(f"{where}: COLOR_MODEL = {value}: only RGB tables are read")
                if eq and key == "HINGE":
                    try:
                        hinge = float(value)
                    except ValueError:
                        raise ValueError(f"{where}: HINGE = {value!r} is not a number") from None
                continue
            tokens = text.split()
            if tokens[0] in special:
                if len(tokens) != 2:
                    raise ValueError(f"{where}: {tokens[0]} takes one r/g/b triplet")
                special[tokens[0]] = _triplet(tokens[1], where)
                continue
            while len(tokens) > 4 and (tokens[-1] in ("L", "U", "B") or tokens[-1].startswith(";")):
                tokens.pop()
            if len(tokens) != 4:
                raise ValueError(f"{where}: a slice is `z0 r/g/b z1 r/g/b`; got {text!r}")
            try:
                z0, z1 = float(tokens[0]), float(tokens[2])
            except ValueError:
                raise ValueError(f"{where}: a slice is `z0 r/g/b z1 r/g/b`; got {text!r}") from None
            if not (np.isfinite(z0) and np.isfinite(z1) and z1 > z0):
                raise ValueError(f"{where}: the slice's z must ascend: {tokens[0]} .. {tokens[2]}")
            if edges and z0 != edges[-1]:
                raise ValueError(f"{where}: the slice starts at {tokens[0]}, the one before ends at {edges[-1]!r}: a gap or an overlap")
            if not edges:
                edges.append(z0)
            edges.append(z1)
            slices.append([_triplet(tokens[1], where), _triplet(tokens[3], where)])
            if len(slices) > MAX_SLICES:
                raise ValueError(f"{where}: more than {MAX_SLICES} slices")
    if not slices:
        raise ValueError(f"{path}: no slices")
    return _table(edges, slices, special["B"], special["F"], special["N"], hinge)


def colour_values(table, v):
    """The unshaded colour rule of DESIGN.md 6n for the float64 values v (no NaN): (u, kind) with u (..., 3) float64 before rounding
    and kind 0 inside the table, 1 below it (B), 2 above it (F).  Every operation is one IEEE float64 operation."""
    v = np.asarray(v, dtype=np.float64)
    E, n = table.edges, table.n
    sl = table.slices.astype(np.float64)
    below, above = v < E[0], v > E[n]
    i = np.clip(np.searchsorted(E, v, side="right") - 1, 0, n - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v - E[i]) / (E[i + 1] - E[i])
        u = sl[i, 0] + (sl[i, 1] - sl[i, 0]) * t[..., None]
    u = np.where(below[..., None], table.background.astype(np.float64), u)
    u = np.where(above[..., None], table.foreground.astype(np.float64), u)
    return u, np.where(below, 1, np.where(above, 2, 0))


def make_cpt(master, series, hinge=None, overrule_bg=False):
    """This project's `makecpt`: the master table stretched onto `series`.  With e_0 .. e_n the master's edges:
    series = (lo, hi), continuous: E_i = lo + (e_i - e_0) / (e_n - e_0) * (hi - lo) in float64 as written, E_0 = lo and E_n = hi exactly.
    hinge = h: the master's hinge (its `# HINGE` value, else its edge equal to 0; it must be an inner edge) goes to h; master edges
    below it map linearly onto [lo, h], those above onto [h, hi]; lo < h < hi.
    series = (lo, hi, inc), discrete: (hi - lo) / inc must be an integer within 1e-9 relative; band j is [lo + j inc, lo + (j + 1) inc)
    (the last edge is hi exactly) and has ONE colour: the stretched continuous table at the band's centre E_j + (E_{j+1} - E_j) / 2,
    each channel floor(u + 0.5).
    overrule_bg (GMT's D="o"): B and F become the table's first and last colours; else B, F and N are the master's.
    At most 2048 slices.  Every refusal is a ValueError."""
    if not isinstance(master, ColorTable):
        raise ValueError(f"make_cpt: master must be a ColorTable (read_cpt, grey_cpt), not {type(master).__name__}")
    try:
        values = [float(s) for s in series]
    except (TypeError, ValueError):
        values = []
    if len(values) not in (2, 3) or not all(np.isfinite(values)):
        raise ValueError(f"make_cpt: series {series!r}: (lo, hi) or (lo, hi, inc), finite")
    lo, hi = values[0], values[1]
    if not lo < hi:
        raise ValueError(f"make_cpt: series {series!r}: lo must be below hi")
    e = master.edges
    n = master.n
    if hinge is None:
        E = lo + (e - e[0]) / (e[n] - e[0]) * (hi - lo)
    else:
        h = float(hinge)
        if not lo < h < hi:
            raise ValueError(f"make_cpt: hinge {hinge!r} must lie strictly inside the series {lo} .. {hi}")
        hm = master.hinge if master.hinge is not None else 0.0
        at = np.flatnonzero(e == hm)
        if at.size != 1 or at[0] in (0, n):
            raise ValueError(f"make_cpt: the master has no inner edge at its hinge {hm}")
        m = int(at[0])
        E = np.where(e < hm, lo + (e - e[0]) / (hm - e[0]) * (h - lo), h + (e - hm) / (e[n] - hm) * (hi - h))
        E[m] = h
    E[0], E[n] = lo, hi
    if not np.all(np.diff(E) > 0):
        raise ValueError(f"make_cpt: series {series!r}: the stretched edges do not ascend strictly in float64")
    table = _table(E, master.slices, master.background, master.foreground, master.nan, None if hinge is None else float(hinge))
    if len(values) == 3:
        inc = values[2]
        q = (hi - lo) / inc if inc > 0 else 0.0
        nb = int(round(q))
        if inc <= 0 or nb < 1 or abs(q - nb) > 1e-9 * abs(q):
            raise ValueError(f"make_cpt: series {series!r}: (hi - lo) / inc must be a positive integer (within 1e-9 relative)")
        if nb > MAX_SLICES:
            raise ValueError(f"make_cpt: series {series!r} makes {nb} bands: at most {MAX_SLICES} slices")
        D = lo + np.arange(nb + 1, dtype=np.float64) * inc
        D[0], D[nb] = lo, hi
        if not np.all(np.diff(D) > 0):
            raise ValueError(f"make_cpt: series {series!r}: the band edges do not ascend strictly in float64")
        centre = D[:-1] + (D[1:] - D[:-1]) * 0.5
        u, _ = colour_values(table, centre)
        c = np.floor(u + 0.5).astype(np.uint8)
        table = _table(D, np.stack([c, c], axis=1), master.background, master.foreground, master.nan, table.hinge)
    if overrule_bg:
        table = _table(table.edges, table.slices, table.slices[0, 0], table.slices[-1, 1], table.nan, table.hinge)
    return table


# ---- the pixel rule on the host ----
def shading_parameters(shading):
    """None, or (sin_a, cos_a, k) of `shading`: "+d" (the reference's default: azimuth -45 degrees, amplitude 1) or (azimuth in
    degrees clockwise from north, amplitude in [0, 1]); k = amplitude * (2 / pi)."""
    if shading is None:
        return None
    if isinstance(shading, str):
        if shading != "+d":
            raise ValueError(f"shading {shading!r}: None, \"+d\" or (azimuth, amplitude)")
        shading = (-45.0, 1.0)
    try:
        azimuth, amplitude = (float(s) for s in shading)
    except (TypeError, ValueError):
        raise ValueError(f"shading {shading!r}: None, \"+d\" or (azimuth, amplitude)") from None
    if not np.isfinite(azimuth) or not 0.0 <= amplitude <= 1.0:
        raise ValueError(f"shading {shading!r}: the azimuth must be finite and the amplitude lie in [0, 1]")
    a = math.radians(azimuth)
    return math.sin(a), math.cos(a), amplitude * (2.0 / math.pi)


def gradient_host(z, sin_a, cos_a, aspect):
    """(g, defined) of the float32 plane z: DESIGN.md 6n's directional gradient in float64, rows north-up, index units."""
    z = np.asarray(z, dtype=np.float32)
    H, W = z.shape
    g = np.zeros((H, W), dtype=np.float64)
    if H < 2 or W < 2:
        return g, np.zeros((H, W), dtype=bool)
    d = z.astype(np.float64)
    cols, rows = np.arange(W), np.arange(H)
    cl, cr = np.maximum(cols - 1, 0), np.minimum(cols + 1, W - 1)
    ru, rd = np.maximum(rows - 1, 0), np.minimum(rows + 1, H - 1)
    zl, zr, zu, zd = d[:, cl], d[:, cr], d[ru, :], d[rd, :]
    defined = np.isfinite(zl) & np.isfinite(zr) & np.isfinite(zu) & np.isfinite(zd)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (zr - zl) * np.where(cr - cl == 2, 0.5, 1.0)[None, :]
        dy = (zu - zd) * np.where(rd - ru == 2, 0.5, 1.0)[:, None]
        g = -(dx * sin_a + (dy * aspect) * cos_a)
    return np.where(defined, g, 0.0), defined


def shade_stats_host(g, defined):
    """(n, mean, sigma) of the defined g: mean = sum g / n, sigma = sqrt(sum (g - mean)^2 / (n - 1)); NumPy's summation order."""
    values = g[defined]
    n = int(values.size)
    mean = float(values.sum() / n) if n else 0.0
    sigma = float(np.sqrt(((values - mean) ** 2).sum() / (n - 1))) if n > 1 else 0.0
    return n, mean, sigma


def relief_image_host(array, cpt, shading=None, aspect=1.0, channels=4, stats=None):
    """The NumPy statement of dbm_grid_relief: the float32 (H, W) `array` coloured by the ColorTable `cpt` as a uint8
    (H, W, channels) image, channels 3 or 4 (alpha 0 at NaN, else 255).  shading: `shading_parameters`; stats = (n, mean, sigma) of
    the gradient (default: `shade_stats_host` of this array); n < 2 or sigma == 0 render with intensity 0."""
    z = np.asarray(array, dtype=np.float32)
    if z.ndim != 2 or z.size == 0:
        raise ValueError(f"relief_image_host: array must be (H, W) and not empty; got {z.shape}")
    _check_render("relief_image_host", cpt, channels, aspect)
    params = shading_parameters(shading)
    nan = np.isnan(z)
    u, _ = colour_values(cpt, np.where(nan, 0.0, z.astype(np.float64)))
    if params is not None:
        sin_a, cos_a, k = params
        g, defined = gradient_host(z, sin_a, cos_a, float(aspect))
        n, mean, sigma = shade_stats_host(g, defined) if stats is None else stats
        if n >= 2 and sigma > 0 and np.isfinite(mean) and np.isfinite(sigma):
            intensity = np.where(defined, k * np.arctan((g - mean) / sigma), 0.0)[..., None]
            u = u + np.where(intensity >= 0, (255.0 - u) * intensity, u * intensity)
    rgb = np.clip(np.floor(u + 0.5), 0, 255).astype(np.uint8)
    rgb = np.where(nan[..., None], cpt.nan, rgb)
    if channels == 3:
        return np.ascontiguousarray(rgb)
    alpha = np.where(nan, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, alpha[..., None]], axis=2))


def _check_render(who, cpt, channels, aspect):
    if not isinstance(cpt, ColorTable):
        raise ValueError(f"{who}: cpt must be a ColorTable (read_cpt, make_cpt, grey_cpt), not {type(cpt).__name__}")
    if channels not in (3, 4):
        raise ValueError(f"{who}: channels {channels!r}: 3 (RGB) or 4 (RGBA)")
    if not np.isfinite(float(aspect)):
        raise ValueError(f"{who}: aspect {aspect!r} must be finite")


# ---- the pixel rule on the device ----
def shade_stats(plane, sin_a, cos_a, aspect=1.0):
    """(n, mean, sigma) of the gradient of the resident float32 plane (dbm_grid_shade_stats: two passes in float64, a fixed order)."""
    H, W = plane_shape(plane)
    out = np.zeros(3, dtype=np.float64)
    plane.ctx.call("dbm_grid_shade_stats", devptr(plane), H, W, float(sin_a), float(cos_a), float(aspect), devptr(out))
    return int(out[0]), float(out[1]), float(out[2])


def relief_image(grid, cpt, shading=None, aspect=1.0, channels=4, ctx=None, stats=None):
    """Colour relief of a plane on the GPU (dbm_grid_relief; the rule: DESIGN.md 6n, `relief_image_host` is its NumPy statement).
    grid: a float32 DeviceArray (H, W) or (1, H, W), a Raster, or a NumPy array that is uploaded.  cpt: a ColorTable.  shading: None,
    "+d" (azimuth -45 degrees, amplitude 1) or (azimuth, amplitude): the intensity k atan((g - mean) / sigma) of the gradient along
    the azimuth, mean and sigma from dbm_grid_shade_stats (or `stats` = (n, mean, sigma)); aspect scales dy.  Returns the resident
    uint8 DeviceArray (H, W, channels), channels 3 or 4.  The call only enqueues unless it computes the statistics."""
    from .tiling import Raster

    _check_render("relief_image", cpt, channels, aspect)
    params = shading_parameters(shading)
    if isinstance(grid, Raster):
        grid = grid.device()
    if isinstance(grid, DeviceArray):
        if grid.dtype != np.float32:
            raise ValueError(f"relief_image: grid holds {grid.dtype.name}: float32 planes are rendered")
        plane = grid
    else:
        host = np.asarray(grid, dtype=np.float32)
        plane = to_device(host.reshape(plane_shape(host)), ctx)
    H, W = plane_shape(plane)
    if H < 1 or W < 1:
        raise ValueError(f"relief_image: empty grid ({H} x {W})")
    shade, sin_a, cos_a, k, mean, sigma = 0, 0.0, 1.0, 0.0, 0.0, 1.0
    if params is not None:
        sin_a, cos_a, k = params
        n, mean, sigma = shade_stats(plane, sin_a, cos_a, aspect) if stats is None else stats
        shade = int(n >= 2 and sigma > 0 and np.isfinite(mean) and np.isfinite(sigma))
        if not shade:
            mean, sigma = 0.0, 1.0
    out = DeviceArray((H, W, channels), plane.ctx, dtype=np.uint8)
    plane.ctx.call("dbm_grid_relief", devptr(plane), H, W, devptr(cpt.edges), devptr(cpt.colors), cpt.n, channels, shade, sin_a, cos_a,
                   float(aspect), float(mean), float(sigma), k, devptr(out))
    return out.written()


# ---- PNG ----
def adler32_combine(adler1, adler2, len2):
    """The Adler-32 of A + B from adler32(A), adler32(B) and len(B).  With (a, b) the two halves (a = 1 + sum of bytes, b = sum of the
    running a's, both mod 65521): a = a1 + a2 - 1, b = b1 + b2 + len2 (a1 - 1)."""
    a1, b1 = adler1 & 0xFFFF, (adler1 >> 16) & 0xFFFF
    a2, b2 = adler2 & 0xFFFF, (adler2 >> 16) & 0xFFFF
    a = (a1 + a2 - 1) % ADLER_MOD
    b = (b1 + b2 + (len2 % ADLER_MOD) * (a1 - 1)) % ADLER_MOD
    return (b << 16) | a


def default_band_rows(W, channels):
    """Rows per band: as many as fit 128 KiB of filtered scanlines, at least one ("Bands": every band is deflated by one
    wavefront and starts without a window -- enough bands to fill the device against matches lost at every cut)."""
    return max(1, BAND_BYTES // (int(W) * int(channels) + 1))


def _image_shape(who, shape, dtype):
    shape = tuple(int(s) for s in shape)
    if np.dtype(dtype) != np.uint8:
        raise ValueError(f"{who}: image holds {np.dtype(dtype).name}: uint8 images are written")
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or shape[2] not in COLOUR_TYPES or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: image must be (H, W) or (H, W, 1 | 3 | 4) and not empty; got {shape}")
    if shape[0] * shape[1] >= 1 << 31:
        raise ValueError(f"{who}: H W must stay below 2^31 pixels")
    return shape


def _png_arguments(who, shape, dtype, filter, band_rows, idat_bytes):
    H, W, channels = _image_shape(who, shape, dtype)
    if filter not in (0, 1, 2):
        raise ValueError(f"{who}: filter {filter!r}: 0 (None), 1 (Sub) or 2 (Up)")
    if band_rows is None:
        band_rows = default_band_rows(W, channels)
    if not isinstance(band_rows, (int, np.integer)) or band_rows < 1:
        raise ValueError(f"{who}: band_rows {band_rows!r}: a number of rows, at least 1")
    band_rows = min(int(band_rows), H)
    if band_rows * (W * channels + 1) >= 1 << 31:
        raise ValueError(f"{who}: bands of {band_rows} rows hold 2^31 bytes or more")
    if not isinstance(idat_bytes, (int, np.integer)) or not 1 <= idat_bytes < 1 << 31:
        raise ValueError(f"{who}: idat_bytes {idat_bytes!r}: 1 .. 2^31 - 1")
    return H, W, channels, band_rows, int(idat_bytes)


def _chunk(f, kind, data):
    f.write(struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF))


def _write_container(path, H, W, channels, idat_bytes, segments):
    """The PNG file: signature, IHDR (8 bits, colour type 0 / 2 / 6, no interlace), the zlib stream 78 01 + the segments + the
    Adler-32 joined from theirs cut into IDAT chunks of idat_bytes (the last one shorter), IEND.  segments yields (bytes, adler,
    length of the band) in band order.  Shared by the host and the device writer."""
    with open(path, "wb") as f:
        f.write(PNG_SIGNATURE)
        _chunk(f, b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPES[channels], 0, 0, 0))
        pending = bytearray(b"\x78\x01")
        adler = 1
        for data, band_adler, band_len in segments:
            pending += data
            adler = adler32_combine(adler, int(band_adler), int(band_len))
            while len(pending) >= idat_bytes:
                _chunk(f, b"IDAT", bytes(pending[:idat_bytes]))
                del pending[:idat_bytes]
        pending += struct.pack(">I", adler)
        while pending:
            _chunk(f, b"IDAT", bytes(pending[:idat_bytes]))
            del pending[:idat_bytes]
        _chunk(f, b"IEND", b"")
    return path


def _segments(H, W, channels, band_rows, per_batch, encode):
    """(bytes, adler, length of the band) of all bands, `per_batch` bands per call of encode(first, n, out, sizes, adlers)."""
    row = W * channels + 1
    batches = encoded_batches(-(-H // band_rows), per_batch, deflate_slot(band_rows * row), encode, extras=(np.uint32,))
    return ((data, adler, min(band_rows, H - k * band_rows) * row) for k, (data, adler) in enumerate(batches))


def write_world_file(path, geometry):
    """The six-line world file next to the image `path` (its extension replaced by .pgw): pixel size x, two zero rotations, pixel
    size y (negative: north-up), then x and y of the CENTRE of the upper-left pixel -- a GridGeometry's node (0, 0)."""
    if not isinstance(geometry, GridGeometry):
        raise ValueError(f"world_file must be a GridGeometry, not {type(geometry).__name__}")
    world = os.path.splitext(os.fspath(path))[0] + ".pgw"
    with open(world, "w") as f:
        f.write("".join(f"{v!r}\n" for v in (float(geometry.dx), 0.0, 0.0, float(geometry.dy), float(geometry.x0), float(geometry.y0))))
    return world


def save_png(path, image, filter=1, band_rows=None, idat_bytes=1 << 20, world_file=None, nthreads=None):
    """Writes the uint8 NumPy `image` (H, W) or (H, W, 1 | 3 | 4) as the PNG `path` and returns the path: the host writer.  The image
    is cut into bands of band_rows rows (default `default_band_rows`); every band is filtered (filter 0 None, 1 Sub, 2 Up) and deflated
    with the fixed Huffman code by dbm_png_encode_host on `nthreads` host threads -- the device encoder's own loop run with one lane --
    and the bands are stitched into one zlib stream.  `write_png_resident` writes the same file, byte for byte, from an
    image in HBM.  world_file: a GridGeometry whose .pgw is written next to the file."""
    who = "save_png"
    if not isinstance(image, np.ndarray):
        raise ValueError(f"{who}: image must be a uint8 NumPy array, not {type(image).__name__} (a DeviceArray is written by write_png_resident)")
    H, W, channels, band_rows, idat_bytes = _png_arguments(who, image.shape, image.dtype, filter, band_rows, idat_bytes)
    if world_file is not None and not isinstance(world_file, GridGeometry):
        raise ValueError(f"{who}: world_file must be a GridGeometry, not {type(world_file).__name__}")
    image = np.ascontiguousarray(image)
    threads = int(nthreads) if nthreads else min(16, os.cpu_count() or 1)
    band_bytes = band_rows * (W * channels + 1)
    per_batch = blocks_per_call(256 << 20, band_bytes, 0, 1, -(-H // band_rows))
    lib = _lib.lib()

    def encode(first, n, out, sizes, adlers):
        _lib.check(lib.dbm_png_encode_host(devptr(image), H, W, channels, filter, band_rows, first, n, devptr(out), out.size, devptr(sizes),
                                           devptr(adlers), threads))

    _write_container(os.fspath(path), H, W, channels, idat_bytes, _segments(H, W, channels, band_rows, per_batch, encode))
    if world_file is not None:
        write_world_file(path, world_file)
    return path


def write_png_resident(path, image, filter=1, band_rows=None, idat_bytes=1 << 20, world_file=None, workspace_limit=None):
    """Writes the resident uint8 DeviceArray `image` (H, W) or (H, W, 1 | 3 | 4) as the PNG `path` and returns the path.  Filtering and
    deflate (one wavefront per band of band_rows rows) run on the GPU (dbm_png_encode); only the compressed segments cross PCIe.  The
    file is byte for byte the one `save_png` writes from the downloaded image with the same arguments.
    workspace_limit: bytes of raw blocks plus their stream slots per batch (block_writes: default 1 GiB; one block always goes)."""
    who = "write_png_resident"
    if not isinstance(image, DeviceArray):
        raise ValueError(f"{who}: image must be a uint8 DeviceArray, not {type(image).__name__} (a NumPy array is written by save_png)")
    H, W, channels, band_rows, idat_bytes = _png_arguments(who, image.shape, image.dtype, filter, band_rows, idat_bytes)
    if world_file is not None and not isinstance(world_file, GridGeometry):
        raise ValueError(f"{who}: world_file must be a GridGeometry, not {type(world_file).__name__}")
    workspace_limit = write_options(workspace_limit, who)
    ctx = image.ctx
    band_bytes = band_rows * (W * channels + 1)
    groups = -(-band_bytes // 16384)                                   # workgroups per band of the filter kernel
    per_batch = blocks_per_call(workspace_limit, band_bytes, deflate_slot(band_bytes), groups, -(-H // band_rows))

    def encode(first, n, out, sizes, adlers):
        ctx.call("dbm_png_encode", devptr(image), H, W, channels, filter, band_rows, first, n, devptr(out), out.size, devptr(sizes),
                 devptr(adlers))

    _write_container(os.fspath(path), H, W, channels, idat_bytes, _segments(H, W, channels, band_rows, per_batch, encode))
    if world_file is not None:
        write_world_file(path, world_file)
    return path


def read_png(path):
    """A minimal reader of exactly the files the two writers make: 8 bits, colour type 0 / 2 / 6, no interlace, filter types 0..2;
    every chunk's CRC-32 is checked, the IDAT data goes through zlib.  Returns the uint8 image, (H, W) for grey, else (H, W, 3 | 4)."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:8] != PNG_SIGNATURE:
        raise ValueError(f"{path}: not a PNG file")
    at, header, data, ended = 8, None, [], False
    while at < len(blob) and not ended:
        if at + 12 > len(blob):
            raise ValueError(f"{path}: truncated chunk at {at}")
        (size,), kind = struct.unpack(">I", blob[at:at + 4]), blob[at + 4:at + 8]
        body = blob[at + 8:at + 8 + size]
        if len(body) != size or at + 12 + size > len(blob):
            raise ValueError(f"{path}: truncated chunk {kind!r} at {at}")
        if struct.unpack(">I", blob[at + 8 + size:at + 12 + size])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"{path}: chunk {kind!r} at {at}: CRC-32 mismatch")
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            data.append(body)
        elif kind == b"IEND":
            ended = True
        at += 12 + size
    if header is None or not ended:
        raise ValueError(f"{path}: IHDR or IEND is missing")
    W, H, depth, colour, compression, filter_method, interlace = header
    channels = {v: k for k, v in COLOUR_TYPES.items()}.get(colour)
    if depth != 8 or channels is None or compression != 0 or filter_method != 0 or interlace != 0:
        raise ValueError(f"{path}: only 8-bit grey, RGB and RGBA images without interlace are read")
    row = W * channels
    raw = np.frombuffer(zlib.decompress(b"".join(data)), dtype=np.uint8)
    if raw.size != H * (row + 1):
        raise ValueError(f"{path}: {raw.size} bytes of scanlines for {H} x {row + 1}")
    lines = raw.reshape(H, row + 1)
    types, image = lines[:, 0], lines[:, 1:].copy()
    if np.any(types > 2):
        raise ValueError(f"{path}: filter types above 2 (Up) are not read")
    for r in range(H):
        if types[r] == 1:   # Sub: a running sum per channel along the row
            image[r] = np.cumsum(image[r].reshape(W, channels), axis=0, dtype=np.uint8).reshape(row)
        elif types[r] == 2 and r > 0:
            image[r] += image[r - 1]
    return image.reshape(H, W) if channels == 1 else image.reshape(H, W, channels)


# ---- the product ----
def reduced_geometry(geometry, k):
    """The geometry of level k of the 2 x 2 pyramid of a grid: pixels 2^k times as large, node (0, 0) at the centre of the first
    2^k x 2^k block of nodes."""
    f = 1 << int(k)
    return dataclasses.replace(geometry, x0=geometry.x0 + (f - 1) / 2 * geometry.dx, y0=geometry.y0 + (f - 1) / 2 * geometry.dy,
                               dx=geometry.dx * f, dy=geometry.dy * f)


def prepared_plane(who, grid, nodata=None, reduce=0, max_size=4096, ctx=None):
    """What `render_dem` and `plot_3d_view` do to a grid before they colour it: (the resident float32 plane, its GridGeometry or None).
    grid: a float32 DeviceArray, a Raster (its nodata and geometry are used) or a NumPy array that is uploaded.  nodata: samples that
    match this finite value by the Raster rule become NaN, in a copy.  reduce = k: level k of `build_overviews` (float32, NaN as nodata)
    and its `reduced_geometry`; "auto": the smallest k with max(H_k, W_k) <= max_size.  `who` opens the messages."""
    import ctypes as C

    from .geotiff import build_overviews
    from .tiling import Raster

    geometry = None
    if isinstance(grid, Raster):
        geometry = grid.geometry
        if nodata is None:
            nodata = grid.nodata
        grid = grid.device()
    if isinstance(grid, DeviceArray):
        if grid.dtype != np.float32:
            raise ValueError(f"{who}: grid holds {grid.dtype.name}: float32 planes are rendered")
        plane = grid
    else:
        host = np.asarray(grid, dtype=np.float32)
        plane = to_device(host.reshape(plane_shape(host)), ctx)
    H, W = plane_shape(plane)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: empty grid ({H} x {W})")
    if nodata is not None:
        nodata = float(nodata)
        if np.isinf(nodata):
            raise ValueError(f"{who}: nodata must be finite, NaN or None")
    if reduce == "auto":
        if not isinstance(max_size, (int, np.integer)) or max_size < 1:
            raise ValueError(f"{who}: max_size {max_size!r}: a number of pixels, at least 1")
        k = 0
        while max(-(-H >> k), -(-W >> k)) > max_size:
            k += 1
    elif isinstance(reduce, (int, np.integer)) and not isinstance(reduce, bool) and reduce >= 0:
        k = int(reduce)
    else:
        raise ValueError(f"{who}: reduce {reduce!r}: a level k >= 0 or \"auto\"")
    c = plane.ctx
    if nodata is not None and not np.isnan(nodata):
        masked = DeviceArray((H, W), c)
        window = np.array([[0, 0, 1, 1]], dtype=np.int64)
        c.call("dbm_grid_tile", devptr(plane), H, W, np.array([0.0, 0.0, 1.0, 1.0]).ctypes.data_as(C.POINTER(C.c_double)), devptr(window), 1,
               0, 1.0, H, W, C.byref(C.c_double(nodata)), C.byref(C.c_float(float("nan"))), 0, devptr(masked), H * W, None)
        plane = masked.written()
    if k > 0:
        plane = build_overviews(plane, k, np.float32, float("nan"))[-1]
        if geometry is not None:
            geometry = reduced_geometry(geometry, k)
    return plane, geometry


def render_dem(grid, path, cpt, shading=None, reduce=0, max_size=4096, nodata=None, filter=1, world_file=True, ctx=None, aspect=1.0,
               channels=4, band_rows=None):
    """The reference's last step (deepbedmap.py:758-775) without GMT and without downloading the plane: `grid` -- a float32 DeviceArray,
    a Raster (its nodata and geometry are used) or a NumPy array that is uploaded -- coloured by `cpt` (with `shading`) and written as
    the PNG `path`.
    nodata: samples that match this finite value by the Raster rule (|v - nodata| <= 1e-8 + 1e-5 |nodata|, dbm_grid_tile) become NaN
    first, in a copy; NaN samples take the table's NaN colour and alpha 0.
    reduce = k: level k of `build_overviews` (float32, NaN as nodata: the nodata-aware 2 x 2 mean) is rendered instead of the plane;
    "auto": the smallest k with max(H_k, W_k) <= max_size.
    world_file: with a Raster, the .pgw of the rendered level is written next to the file.
    Returns (path, the GridGeometry of the image or None)."""
    who = "render_dem"
    _check_render(who, cpt, channels, aspect)
    shading_parameters(shading)
    plane, geometry = prepared_plane(who, grid, nodata, reduce, max_size, ctx)
    image = relief_image(plane, cpt, shading=shading, aspect=aspect, channels=channels)
    write_png_resident(path, image, filter=filter, band_rows=band_rows, world_file=geometry if world_file else None)
    return path, geometry
