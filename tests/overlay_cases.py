"""The scenes the overlay tests draw (tests/test_overlay_host.py on the host, tests/test_gpu_overlay.py on the GPU): geometries, shapes,
a zoo of primitives per geometry and primitive tables of an exact length.  Not collected by pytest (no test_ prefix).  A layer is the
tuple of tests/overlay_restatement.py: (kind, table, size, rgba); `layers_of` makes the package's Layer objects of them."""
import numpy as np

T, K = 16, 256                                              # DBM_OVERLAY_TILE, DBM_OVERLAY_CHUNK (the tests assert that they are)
PX = 250.0
GEOM = (-1_600_000.0, -200_000.0, PX, -PX)                  # continental coordinates, north-up
GEOM_SOUTH_UP = (-1_600_000.0, -230_000.0, PX, PX)          # dy > 0
GEOM_EAST_FIRST = (-1_570_000.0, -200_000.0, -PX, -PX)      # dx < 0
GEOMETRIES = {"north_up": GEOM, "dy_positive": GEOM_SOUTH_UP, "dx_negative": GEOM_EAST_FIRST}
SHAPES = [(1, 1), (1, T + 1), (T - 1, T), (T, T), (T + 1, 2 * T + 1), (33, 47), (97, 131)]
COUNTS = [0, 1, K - 1, K, K + 1, 2 * K + 3]
SIZES = [0.0, 1.0, 2.5, 40.0]
ORANGE, BLUE = (238, 154, 0, 255), (20, 40, 230, 128)


def xy(geom, c, r):
    """Map coordinates of the (possibly fractional) pixel position (c, r)."""
    return geom[0] + c * geom[2], geom[1] + r * geom[3]


def segment(geom, ca, ra, cb, rb):
    return [*xy(geom, ca, ra), *xy(geom, cb, rb)]


def zoo_segments(geom, shape, size):
    """Horizontal, vertical and diagonal segments through pixel centres; one that enters and leaves the image; one entirely outside
    but within the pen's radius of the first row; one that ends exactly on a tile corner; a dot (length zero) on a centre."""
    H, W = shape
    n = max(min(H, W) - 1, 1)
    return np.array([
        segment(geom, 1, H // 2, max(W - 2, 1), H // 2),
        segment(geom, W // 3, 0, W // 3, H - 1),
        segment(geom, 0, 0, n, n),
        segment(geom, -5.3, 0.3 * H, W + 4.7, 0.8 * H),
        segment(geom, 2, -0.45 * size - 0.3, max(W - 3, 3), -0.45 * size - 0.3),
        segment(geom, 3.25, 2.75, T - 0.5, T - 0.5),
        segment(geom, W // 2, H // 3, W // 2, H // 3),
    ])


def zoo_discs(geom, shape, size):
    """Discs centred on pixel centres, on pixel corners (one of them a tile corner) and half a radius outside the image."""
    H, W = shape
    return np.array([
        xy(geom, W // 2, H // 2), xy(geom, 0, 0), xy(geom, W - 1, H - 1),
        xy(geom, W // 3 + 0.5, H // 4 + 0.5), xy(geom, T - 0.5, T - 0.5),
        xy(geom, -0.5 - size / 4, H / 2), xy(geom, W / 2, H - 0.5 + size / 4),
    ])


def zoo(geom, shape, size, kind):
    return zoo_segments(geom, shape, size) if kind == "segments" else zoo_discs(geom, shape, size)


def far_away(geom, k, kind):
    """A primitive a few thousand kilometres away: culling must drop it."""
    x, y = geom[0] + 3.0e6 + 1000.0 * k, geom[1] - 2.5e6 - 700.0 * k
    return [x, y, x + 300.0, y + 100.0] if kind == "segments" else [x, y]


def padded(geom, shape, count, size, kind):
    """Exactly `count` primitives: the zoo first, then dots inside the image and far-away primitives in turn."""
    width = 4 if kind == "segments" else 2
    if count == 0:
        return np.zeros((0, width))
    if count == 1:
        if kind == "segments":
            return np.array([segment(geom, -2.5, 0.3 * shape[0], shape[1] + 1.25, 0.8 * shape[0])])
        return np.array([xy(geom, shape[1] // 2, shape[0] // 2)])
    rows = [list(r) for r in zoo(geom, shape, size, kind)]
    assert len(rows) <= count
    k = 0
    while len(rows) < count:
        if k % 2 == 0:
            p = xy(geom, (7 * k) % shape[1] + 0.37, (3 * k) % shape[0] + 0.1)
            rows.append([*p, *p] if kind == "segments" else [*p])
        else:
            rows.append(far_away(geom, k, kind))
        k += 1
    return np.array(rows)


def destination(shape, channels, seed=0, transparent=False):
    """Random bytes; transparent: alpha 0 on a third of the pixels, the nodata pixels of relief_image."""
    r = np.random.default_rng(seed)
    image = r.integers(0, 256, size=(shape[0], shape[1], channels), dtype=np.uint8)
    if transparent and channels == 4:
        image[r.random(shape) < 0.33, 3] = 0
    return image


def two_layers(geom, shape, size, first=ORANGE, second=BLUE):
    return [("segments", zoo_segments(geom, shape, size), size, first), ("discs", zoo_discs(geom, shape, size), size, second)]


def layers_of(dbm, layers):
    return [dbm.Layer.lines(table, size, rgba) if kind == "segments" else dbm.Layer.points(table, size, rgba)
            for kind, table, size, rgba in layers]
