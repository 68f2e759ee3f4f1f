"""GeoTIFF writer for the stitched DEM (reference deepbedmap.py:749-756 -> data_prep.py:779-834).

The reference saves `Y_hat.astype(np.int16)` through rasterio / GDAL: driver GTiff, one band, `dtype=int16`,
`nodata=-2000`, `tiled=True`, `compress=lzw`, `bigtiff=YES`, polar stereographic CRS, the affine transform of
`rasterio.transform.from_bounds(*window_bound, height, width)`.  rasterio / GDAL are not part of this framework: the
container is written here (classic TIFF or BigTIFF, little endian, 256 x 256 tiles as GDAL's default block size, GeoTIFF
tags ModelPixelScale / ModelTiepoint / GeoKeyDirectory with ProjectedCSType = EPSG:3031, GDAL_NODATA), the LZW streams come
from libdbm (dbm_lzw_encode_tiles: TIFF 6.0 LZW, host threads over tiles) and the int16 cast of a device-resident canvas
from the GPU (dbm_f32_to_i16: NumPy's astype semantics, NaN frame -> 0).  `read_geotiff` decodes the file again
(bit-exact round trip; the tests also decode it with Pillow / libtiff).  `write_geotiff_resident` writes the same file from a plane in
HBM without downloading it: cast, tile cutting, predictor 2 and LZW run on the GPU (dbm_tiff_encode), only the streams
cross PCIe; both writers share the tags (`_image_tags`) and the container (`_write_container`).  `overviews=` on either writer puts
reduced-resolution images behind the first one, as `gdaladdo -r average` would: each level is the nodata-aware 2 x 2 mean of the one
before (`overview_pyramid`, the NumPy statement; dbm_grid_overviews builds the levels next to a resident canvas), and `overview=k` on
the readers selects one ("Overviews").

Reading rasters as GDAL and libtiff write them (reference data_prep.py:668, :845-877; deepbedmap.py:164-204, through rasterio): the
second half of this file -- `open_geotiff` (header, geometry, block plan, refusals: host), `read_geotiff_resident` (the blocks decoded on
the GPU by dbm_tiff_decode: LZW, deflate, predictors, float32 conversion, placement; `inflate="host"` inflates on host threads instead).
DESIGN.md 6i.
"""
import ctypes as C
import os
import struct

import numpy as np

from . import _lib, block_reads, block_writes
from .block_reads import BlockPlan
from .resident import DeviceArray, GridGeometry, devptr

TILE = 256  # GDAL's default block size for tiled=True
EPSG_ANTARCTIC_POLAR_STEREOGRAPHIC = 3031  # "+proj=stere +lat_0=-90 +lat_ts=-71 +lon_0=0 ..." (data_prep.py:784)

_TYPES = {1: ("B", 1), 2: ("s", 1), 3: ("H", 2), 4: ("I", 4), 12: ("d", 8), 16: ("Q", 8)}


def canvas_to_int16(canvas):
    """`Y_hat.astype(np.int16)` (deepbedmap.py:752) for a NumPy array or a DeviceArray (converted on the GPU: half the
    bytes cross PCIe).  Returns a NumPy int16 array of the same shape."""
    if isinstance(canvas, DeviceArray):
        ctx = canvas.ctx
        with ctx.scratch(2 * canvas.size + 16) as dst:
            ctx.call("dbm_f32_to_i16", devptr(canvas), devptr(dst), canvas.size)
            return ctx.download(dst, np.int16, canvas.shape)
    with np.errstate(invalid="ignore"):
        return np.asarray(canvas).astype(np.int16)


def lzw_encode_tiles(tiles, nthreads=None):
    """tiles: (ntiles, tile_bytes) uint8 -> list of bytes objects (TIFF 6.0 LZW streams)."""
    tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
    nt, nb = tiles.shape
    stride = nb * 3 // 2 + 64
    out = np.empty((nt, stride), dtype=np.uint8)
    sizes = (C.c_size_t * max(nt, 1))()
    rc = _lib.lib().dbm_lzw_encode_tiles(tiles.ctypes.data_as(C.c_void_p), nb, nt, out.ctypes.data_as(C.c_void_p), stride, sizes,
                                         int(nthreads or min(16, os.cpu_count() or 1)))
    if rc != 0:
        raise _lib.DbmError(f"dbm_lzw_encode_tiles failed ({rc})")
    return [out[i, :sizes[i]].tobytes() for i in range(nt)]


def lzw_decode(stream, nbytes):
    src = np.frombuffer(stream, dtype=np.uint8)
    dst = np.empty(nbytes + 16, dtype=np.uint8)
    got = C.c_size_t()
    rc = _lib.lib().dbm_lzw_decode(src.ctypes.data_as(C.c_void_p), src.size, dst.ctypes.data_as(C.c_void_p), dst.size, C.byref(got))
    if rc != 0 or got.value != nbytes:
        raise _lib.DbmError(f"dbm_lzw_decode failed ({rc}, {got.value} of {nbytes} bytes)")
    return dst[:nbytes]


def inflate(stream, nbytes):
    """One zlib stream decoded by the device decoder's loop run with one lane on the host (dbm_inflate): `nbytes` bytes as uint8, or
    DbmError on everything dbm_tiff_decode reports for compression 8 (a malformed stream, a size other than nbytes)."""
    src = np.frombuffer(stream, dtype=np.uint8)
    dst = np.empty(max(int(nbytes), 1), dtype=np.uint8)
    got = C.c_size_t()
    rc = _lib.lib().dbm_inflate(src.ctypes.data_as(C.c_void_p) if src.size else dst.ctypes.data_as(C.c_void_p), src.size,
                                dst.ctypes.data_as(C.c_void_p), int(nbytes), C.byref(got))
    if rc != 0 or got.value != nbytes:
        raise _lib.DbmError(f"dbm_inflate failed ({rc}, {got.value} of {nbytes} bytes)")
    return dst[:nbytes]


def _tiles_of(band, th, tw):
    """(H, W) -> (ntiles, th, tw), row-major tile order, edge tiles zero padded (TIFF 6.0 section 15)."""
    H, W = band.shape
    ny, nx = (H + th - 1) // th, (W + tw - 1) // tw
    padded = np.zeros((ny * th, nx * tw), dtype=band.dtype)
    padded[:H, :W] = band
    return padded.reshape(ny, th, nx, tw).transpose(0, 2, 1, 3).reshape(ny * nx, th, tw), ny, nx


def _epsg_of(crs):
    """EPSG code of `crs`: an int, "EPSG:3031", or the reference's default PROJ string for Antarctic polar stereographic
    (data_prep.py:784: "+proj=stere +lat_0=-90 +lat_ts=-71 +lon_0=0 ... +datum=WGS84 ..." = EPSG:3031).  Other PROJ strings
    would need a projection database: refused with a clear message."""
    if isinstance(crs, (int, np.integer)):
        return int(crs)
    text = str(crs).strip()
    if text.isdigit():
        return int(text)
    if text.upper().startswith("EPSG:") and text[5:].strip().isdigit():
        return int(text[5:])
    if text.startswith("+"):
        kv = dict((t.lstrip("+").split("=") + [""])[:2] for t in text.split())
        f = lambda k, d=0.0: float(kv.get(k, d) or d)  # noqa: E731
        if (kv.get("proj") == "stere" and f("lat_0") == -90.0 and f("lat_ts") == -71.0 and f("lon_0") == 0.0 and f("k", 1.0) == 1.0
                and f("x_0") == 0.0 and f("y_0") == 0.0 and kv.get("datum", kv.get("ellps", "WGS84")) == "WGS84"
                and kv.get("units", "m") == "m"):
            return EPSG_ANTARCTIC_POLAR_STEREOGRAPHIC
    raise ValueError(f"save_array_to_grid: crs {crs!r} is not an EPSG code, 'EPSG:n' or the Antarctic polar stereographic "
                     "PROJ string of the reference (EPSG:3031)")


_OFFSETS, _COUNTS = object(), object()   # tag values that `_write_container` fills in: where it put the streams, and their sizes


def _predictor_of(predictor, who):
    if isinstance(predictor, (bool, np.bool_)) or predictor not in (1, 2):
        raise ValueError(f"{who}: predictor {predictor!r}: 1 (none) or 2 (horizontal differencing) are written")
    return int(predictor)


def _compression_of(compression, who):
    """TIFF Compression (259) of the `compression` argument: 1 or 5."""
    text = str(compression).lower()
    if text == "lzw":
        return 5
    if text in ("none", "1"):
        return 1
    raise ValueError(f"{who}: unsupported compression {compression!r} (none, lzw)")


def _image_tags(H, W, dt, comp, predictor, tiled, th, tw, window_bound, nodataval, epsg, bigtiff, overview=False):
    """The image directory both writers share: (tag, type, values) with _OFFSETS / _COUNTS where the block tables go.  overview: the
    directory of a reduced-resolution image behind the first one, as GDAL lays it out: NewSubfileType (254) = 1 and no georeference
    tags (window_bound and epsg are not looked at)."""
    sample_format = {"f": 3, "i": 2, "u": 1}[dt.kind]
    nodata = (repr(int(nodataval)) if float(nodataval).is_integer() else repr(float(nodataval))).encode() + b"\0"
    off_t = 16 if bigtiff else 4  # LONG8 / LONG
    tags = [
        (256, 4, [W]), (257, 4, [H]), (258, 3, [8 * dt.itemsize]), (259, 3, [comp]), (262, 3, [1]), (277, 3, [1]),
        (284, 3, [1]), (339, 3, [sample_format]), (42113, 2, [nodata]),
    ]
    if overview:
        tags += [(254, 4, [1])]
    else:
        minx, miny, maxx, maxy = (float(v) for v in window_bound)
        px, py = (maxx - minx) / W, (maxy - miny) / H  # rasterio.transform.from_bounds
        geokeys = [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, epsg]  # projected, PixelIsArea, ProjectedCSType
        tags += [(33550, 12, [px, py, 0.0]), (33922, 12, [0.0, 0.0, 0.0, minx, maxy, 0.0]), (34735, 3, geokeys)]
    if predictor != 1:
        tags += [(317, 3, [predictor])]
    if tiled:
        tags += [(322, 4, [tw]), (323, 4, [th]), (324, off_t, _OFFSETS), (325, off_t, _COUNTS)]
    else:
        tags += [(278, 4, [th]), (273, off_t, _OFFSETS), (279, off_t, _COUNTS)]
    return tags


def _write_container(path, bigtiff, tags, streams, overviews=()):
    """The file both writers share: the header, then the streams (any iterable of bytes-like objects, taken one at a time) at even
    offsets, then the image directory with its tags sorted and the values that do not fit an entry behind it.  overviews: the images
    behind the first one, a list of (tags, streams): the streams of image 0, 1, ... follow one another, then the directories in the
    same order, each at an even offset and chained through its next-IFD offset, the last one 0."""
    images = [(tags, streams)] + list(overviews)
    with open(path, "wb") as f:
        # header, then the pixel data, then the IFDs (offsets known by then)
        f.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 0) if bigtiff else struct.pack("<2sHI", b"II", 42, 0))
        tables = []
        for _, image_streams in images:
            offsets, counts = [], []
            for s in image_streams:
                if f.tell() % 2:
                    f.write(b"\0")
                offsets.append(f.tell())
                counts.append(len(s))
                f.write(s)
            tables.append((offsets, counts))
        if f.tell() % 2:
            f.write(b"\0")

        def payload(typ, vals):
            fmt, _ = _TYPES[typ]
            if typ == 2:
                return vals[0]
            return struct.pack("<%d%s" % (len(vals), fmt), *vals)

        inline = 8 if bigtiff else 4
        first_ifd = ifd_pos = f.tell()
        for k, (image_tags, _) in enumerate(images):
            image_tags = sorted(image_tags, key=lambda t: t[0])
            offsets, counts = tables[k]
            entries, extra = [], b""
            ntags = len(image_tags)
            ifd_size = (8 + 20 * ntags + 8) if bigtiff else (2 + 12 * ntags + 4)
            extra_pos = ifd_pos + ifd_size
            for tag, typ, vals in image_tags:
                if vals is _OFFSETS:
                    vals = offsets
                elif vals is _COUNTS:
                    vals = counts
                data = payload(typ, vals)
                count = len(data) if typ == 2 else len(vals)
                if len(data) <= inline:
                    field = data + b"\0" * (inline - len(data))
                else:
                    if (extra_pos + len(extra)) % 2:
                        extra += b"\0"
                    field = struct.pack("<Q" if bigtiff else "<I", extra_pos + len(extra))
                    extra += data
                entries.append(struct.pack("<HHQ" if bigtiff else "<HHI", tag, typ, count) + field)
            last = k == len(images) - 1
            if not last and (extra_pos + len(extra)) % 2:
                extra += b"\0"
            next_ifd = 0 if last else extra_pos + len(extra)
            f.write(struct.pack("<Q" if bigtiff else "<H", ntags) + b"".join(entries) + struct.pack("<Q" if bigtiff else "<I", next_ifd) + extra)
            ifd_pos = next_ifd
        f.seek(8 if bigtiff else 4)
        f.write(struct.pack("<Q" if bigtiff else "<I", first_ifd))
    return path


def _difference_blocks(blocks):
    """Predictor 2 (libtiff's horizontal differencing) of blocks (n, rows, cols): per block row d[0] = s[0], d[c] = s[c] - s[c - 1] over
    the whole row, padding columns included, wrapping in the sample's own width (floats: on the bit patterns)."""
    u = np.ascontiguousarray(blocks).view(np.dtype("<u%d" % blocks.dtype.itemsize))
    d = u.copy()
    d[..., 1:] = u[..., 1:] - u[..., :-1]
    return d.view(blocks.dtype)


def overview_shapes(H, W, levels, who="overview_shapes", name="levels"):
    """The shapes [(H_1, W_1), ..., (H_levels, W_levels)] of the overviews of an (H, W) image: every level halves the one before,
    H' = ceil(H / 2), W' = ceil(W / 2).  levels: an int >= 0, or "auto": down to the first level whose larger side is at most TILE
    (256; none for an image that small).  A level beyond the first 1 x 1 level, or anything else, raises a ValueError that names the
    argument (`name` of `who`) and the number of levels the image admits."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: an image of {H} x {W} has no overviews")
    shapes, h, w = [], H, W
    while h > 1 or w > 1:
        h, w = -(-h // 2), -(-w // 2)
        shapes.append((h, w))
    if isinstance(levels, str) and levels == "auto":
        n = 0
        while max((H, W) if n == 0 else shapes[n - 1]) > TILE:
            n += 1
        return shapes[:n]
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)) or levels < 0:
        raise ValueError(f"{who}: {name} {levels!r}: an int >= 0 or 'auto' (an image of {H} x {W} admits {len(shapes)} levels)")
    if levels > len(shapes):
        raise ValueError(f"{who}: {name} {levels!r}: an image of {H} x {W} admits {len(shapes)} levels (the last one is 1 x 1)")
    return shapes[:int(levels)]


def _halved(a, nodata):
    """One level of `overview_pyramid`: a float32 (H, W) -> (the means, float32 (ceil(H / 2), ceil(W / 2)); where a window holds no valid
    sample); `nodata` marks invalid samples besides NaN."""
    H, W = a.shape
    h, w = -(-H // 2), -(-W // 2)
    zero = np.float32(0.0)
    x = np.full((2 * h, 2 * w), zero, dtype=np.float32)   # samples that do not exist: +0.0, not counted
    ok = np.zeros((2 * h, 2 * w), dtype=bool)
    ok[:H, :W] = ~(np.isnan(a) | (a == nodata))
    x[:H, :W] = a
    x = np.where(ok, x, zero)
    s = (x[0::2, 0::2] + x[0::2, 1::2]) + (x[1::2, 0::2] + x[1::2, 1::2])
    n = (ok[0::2, 0::2].astype(np.float32) + ok[0::2, 1::2].astype(np.float32)) + (ok[1::2, 0::2].astype(np.float32)
                                                                                  + ok[1::2, 1::2].astype(np.float32))
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s / n
    return m, n == 0


def overview_pyramid(band, levels, nodataval):
    """The overviews of the image `band` (H, W), int16 or float32 as the file holds it: the NumPy statement of the definition in
    DESIGN.md 6j ("Overviews"), float32 throughout, that dbm_grid_overviews computes bit for bit.  Level k + 1 is made from level k
    alone: pixel (r, c) is s / float32(n), s = (a00 + a01) + (a10 + a11) over the samples of rows 2r, 2r + 1 and columns 2c, 2c + 1
    with +0.0 for those that do not exist or are invalid (float32: NaN or equal to float32(nodataval); int16: equal to
    int(nodataval)), n the number of the others; n == 0 gives the nodata value; int16 levels are `np.rint` of that (ties to even)
    and the next level is made from the rounded samples.  Returns the list of the levels 1 .. levels in band's dtype
    (levels: `overview_shapes`)."""
    band = np.asarray(band)
    if band.ndim != 2 or band.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError(f"overview_pyramid: band must be an int16 or float32 (H, W) array, not {band.dtype.name} {band.shape}")
    shapes = overview_shapes(band.shape[0], band.shape[1], levels, "overview_pyramid")
    integer = band.dtype.kind == "i"
    nodata = np.float32(int(nodataval)) if integer else np.float32(nodataval)
    out, a = [], band.astype(np.float32)
    for shape in shapes:
        m, empty = _halved(a, nodata)
        with np.errstate(invalid="ignore"):
            a = np.where(empty, nodata, np.rint(m) + np.float32(0.0) if integer else m).astype(np.float32)   # (+ 0.0: the int16 0 is +0.0)
        assert a.shape == shape
        with np.errstate(invalid="ignore"):
            out.append(a.astype(band.dtype))
    return out


def build_overviews(array, levels, dtype=np.float32, nodataval=-2000):
    """The overviews a writer puts behind `array` with `overviews=levels`, without writing a file (`overview_pyramid`'s
    definition; levels: `overview_shapes`).  A float32 DeviceArray (H, W) or (1, H, W): one dbm_grid_overviews call, the levels
    returned as float32 DeviceArrays (H_k, W_k) that share one allocation -- dtype int16: level 0 is the cast of the plane and the
    samples are the rounded values as floats.  A NumPy array: the levels as NumPy arrays of `dtype`, from the array cast to it."""
    who = "build_overviews"
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError(f"{who}: dtype {dt.name}: int16 (by cast) and float32 have overviews")
    if not isinstance(array, DeviceArray):
        band = np.asarray(array)
        if not (band.ndim == 2 or (band.ndim == 3 and band.shape[0] == 1)):
            raise ValueError(f"{who}: array must be (1, H, W) or (H, W); got {band.shape}")
        band = band.reshape(band.shape[-2:])
        with np.errstate(invalid="ignore"):
            return overview_pyramid(band.astype(dt), levels, nodataval)
    shape = tuple(array.shape)
    if array.dtype != np.float32 or not (len(shape) == 2 or (len(shape) == 3 and shape[0] == 1)) or shape[-2] < 1 or shape[-1] < 1:
        raise ValueError(f"{who}: array must be a float32 DeviceArray of (1, H, W) or (H, W) and not empty; got {array.dtype.name} {shape}")
    shapes = overview_shapes(shape[-2], shape[-1], levels, who)
    if dt == np.int16:
        _finite_nodata(nodataval, who)
    return _device_pyramid(array, shape[-2], shape[-1], 1 if dt == np.int16 else 4, nodataval, shapes)


def _finite_nodata(nodataval, who):
    """int(nodataval) marks the invalid samples of an int16 file: NaN and inf have none (refused before any device work)."""
    try:
        int(nodataval)
    except (ValueError, OverflowError):
        raise ValueError(f"{who}: nodataval {nodataval!r}: the overviews of an int16 file need a finite value") from None


def _device_pyramid(array, H, W, sample_type, nodataval, shapes):
    """dbm_grid_overviews of the resident plane `array` into ONE DeviceArray; returns the levels as views of it."""
    if not shapes:
        return []
    ctx = array.ctx
    pyramid = DeviceArray((sum(h * w for h, w in shapes),), ctx)
    ctx.call("dbm_grid_overviews", devptr(array), H, W, sample_type, C.byref(C.c_double(float(nodataval))), len(shapes), devptr(pyramid))
    pyramid.written()
    levels, at = [], 0
    for h, w in shapes:
        levels.append(DeviceArray((h, w), ctx, ptr=pyramid.ptr + 4 * at, owner=pyramid))
        at += h * w
    return levels


def _host_blocks(band, dt, comp, predictor, tiled, nthreads):
    """One image of `save_array_to_grid`: (th, tw, the list of its blocks' streams)."""
    H, W = band.shape
    th, tw = (TILE, TILE) if tiled else (min(TILE, H), W)
    blocks, ny, nx = _tiles_of(band, th, tw)
    if predictor == 2:
        blocks = _difference_blocks(blocks)
    raw = blocks.reshape(len(blocks), -1).view(np.uint8)
    # strips: the last one holds only the rows that exist (TIFF 6.0: StripByteCounts of H % RowsPerStrip rows, what GDAL
    # writes); tiles are always whole (zero padded)
    last_rows = H - (ny - 1) * th
    short_last = (not tiled) and last_rows < th
    if comp == 5:
        if short_last:
            streams = lzw_encode_tiles(raw[:-1], nthreads) if ny > 1 else []
            streams += lzw_encode_tiles(np.ascontiguousarray(raw[-1:, :last_rows * tw * dt.itemsize]), nthreads)
        else:
            streams = lzw_encode_tiles(raw, nthreads)
    else:
        streams = [r.tobytes() for r in raw]
        if short_last:
            streams[-1] = streams[-1][:last_rows * tw * dt.itemsize]
    return th, tw, streams


def save_array_to_grid(outfilepath, window_bound, array, save_netcdf=False, crs=EPSG_ANTARCTIC_POLAR_STEREOGRAPHIC, dtype=None,
                       nodataval=-2000, tiled=False, compression="none", bigtiff=True, nthreads=None, predictor=1, overviews=0):
    """data_prep.py:779-834 without rasterio: writes `{outfilepath}.tif` and returns its path.

    window_bound = (minx, miny, maxx, maxy); array is CHW with one channel (a NumPy array, or a DeviceArray canvas when
    dtype is int16); compression "none" or "lzw" (rasterio.enums.Compression values); tiled=False writes one strip per
    row block of 256 rows.  predictor=2 (with "lzw"; libtiff's predictors are part of its codecs, so "none" writes the samples
    as they are and no tag): every block row is differenced on the host before it is encoded, and Predictor (317) = 2 is written.
    overviews (int16 and float32 files): the number of reduced-resolution images written behind the first one, or "auto"
    (`overview_shapes`); each halves the one before (`overview_pyramid`: `gdaladdo -r average` in spirit) and is cut, differenced
    and compressed as the first one is.  0: the file is byte for byte what it always was.
    save_netcdf (data_prep.py:826-830; float32 files only): `{outfilepath}.nc` is written next to the .tif from the band as the TIFF
    holds it (`netcdf.save_grid_to_netcdf`, its defaults); the .tif and the return value are what they are without it."""
    assert len(array.shape) == 3 and array.shape[0] == 1  # one band, CHW (data_prep.py:800-801)
    predictor = _predictor_of(predictor, "save_array_to_grid")
    dt = np.dtype(dtype if dtype is not None else getattr(array, "dtype", np.float32))
    if dt == np.int16 and not isinstance(array, np.ndarray):
        band = canvas_to_int16(array)[0]
    else:
        band = np.asarray(array)[0]
        if band.dtype != dt:
            with np.errstate(invalid="ignore"):
                band = band.astype(dt)
    band = np.ascontiguousarray(band.astype(dt.newbyteorder("<"), copy=False))
    H, W = band.shape
    if dt.kind not in "fiu":
        raise ValueError(f"unsupported dtype {dt}")
    if save_netcdf and dt != np.dtype(np.float32):
        raise ValueError(f"save_array_to_grid: dtype {dt.name}: save_netcdf writes float32 files only")
    epsg = _epsg_of(crs)
    comp = _compression_of(compression, "save_array_to_grid")
    if comp == 1:
        predictor = 1
    shapes = overview_shapes(H, W, overviews, "save_array_to_grid", "overviews")
    if shapes and dt not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError(f"save_array_to_grid: overviews of {dt.name} samples: int16 and float32 files have them")
    th, tw, streams = _host_blocks(band, dt, comp, predictor, tiled, nthreads)
    tags = _image_tags(H, W, dt, comp, predictor, tiled, th, tw, window_bound, nodataval, epsg, bigtiff)
    images = []
    for level in overview_pyramid(band, len(shapes), nodataval) if shapes else ():
        h, w = level.shape
        level = np.ascontiguousarray(level.astype(dt.newbyteorder("<"), copy=False))
        lh, lw, level_streams = _host_blocks(level, dt, comp, predictor, tiled, nthreads)
        images.append((_image_tags(h, w, dt, comp, predictor, tiled, lh, lw, None, nodataval, None, bigtiff, overview=True), level_streams))
    written = _write_container(f"{outfilepath}.tif", bigtiff, tags, streams, images)
    if save_netcdf:
        from .netcdf import save_grid_to_netcdf

        save_grid_to_netcdf(f"{outfilepath}.nc", window_bound, band, nthreads=nthreads)
    return written


def write_geotiff_resident(outfilepath, window_bound, array, dtype=None, nodataval=-2000, tiled=True, compression="lzw", predictor=1,
                           bigtiff=True, crs=EPSG_ANTARCTIC_POLAR_STEREOGRAPHIC, workspace_limit=None, overviews=0):
    """The mirror of `read_geotiff_resident`: writes `{outfilepath}.tif` from a plane that lives in HBM and returns its path.  The cast
    to int16 (NumPy's `astype`), the cutting of tiles or strips, predictor 2 and TIFF 6.0 LZW (one wavefront per block) run on the GPU
    (dbm_tiff_encode); only the encoded streams cross PCIe.  The file is byte for byte the one `save_array_to_grid` writes from the
    downloaded plane with the same arguments.

    array: a float32 DeviceArray of shape (1, H, W) or (H, W), or a resident Raster; dtype int16 or float32 (the default);
    compression "lzw" or "none" (the samples as they are: as in save_array_to_grid the predictor then has no effect); predictor 1 or
    2.  workspace_limit: bytes of raw blocks plus their stream slots per batch (block_writes: default 1 GiB; one block always goes).
    overviews: the number of reduced-resolution images behind the first one, or "auto" (`overview_shapes`), as in save_array_to_grid:
    one dbm_grid_overviews call builds them all next to the plane -- float32 planes one behind the other in one allocation of at most
    a third of the plane's size (1/4 + 1/16 + ..., a little more at odd sizes); for int16 the canvas is cast while it is read, never
    copied -- and every level then goes through the same batches as the first image.  Anything else raises a ValueError that names
    the argument, before any device work."""
    who = "write_geotiff_resident"
    array = block_writes.resident_plane_to_write(array, who, "save_array_to_grid")
    if array.dtype != np.float32:
        raise ValueError(f"{who}: array holds {array.dtype.name}: only float32 planes are written")
    shape = tuple(array.shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[0] == 1)) or shape[-2] < 1 or shape[-1] < 1:
        raise ValueError(f"{who}: array must be (1, H, W) or (H, W) and not empty; got {shape}")
    H, W = shape[-2], shape[-1]
    try:
        dt = np.dtype(np.float32 if dtype is None else dtype)
    except TypeError:
        raise ValueError(f"{who}: dtype {dtype!r} is not a sample type") from None
    if dt not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError(f"{who}: dtype {dt.name}: int16 (by cast) and float32 are written")
    predictor = _predictor_of(predictor, who)
    comp = _compression_of(compression, who)
    if comp == 1:
        predictor = 1
    epsg = _epsg_of(crs)
    workspace_limit = block_writes.write_options(workspace_limit, who)
    shapes = overview_shapes(H, W, overviews, who, "overviews")
    if shapes and dt == np.int16:
        _finite_nodata(nodataval, who)
    sample_type = 1 if dt == np.int16 else 4
    ctx = array.ctx

    def plan(h, w):
        """Block shape, number of blocks, a block's worst case in the download, blocks per dbm_tiff_encode call of an (h, w) image."""
        th, tw = (TILE, TILE) if tiled else (min(TILE, h), w)
        block_bytes = th * tw * dt.itemsize
        if block_bytes >= 1 << 31:
            raise ValueError(f"{who}: array: blocks of {th} x {tw} samples hold 2^31 bytes or more")
        nblocks = -(-h // th) * -(-w // tw)
        worst = block_bytes * 3 // 2 + 64 if comp == 5 else block_bytes   # a block's bytes in the download, before rounding up to even
        per_batch = block_writes.blocks_per_call(workspace_limit, block_bytes, worst if comp == 5 else 0, th, nblocks)
        return th, tw, nblocks, worst, per_batch

    def streams(plane, h, w, th, tw, nblocks, worst, per_batch):
        def encode(first, n, out, sizes):
            ctx.call("dbm_tiff_encode", devptr(plane), h, w, sample_type, th, tw, 1 if tiled else 0, predictor, comp, first, n, devptr(out),
                     out.size, devptr(sizes))
        return block_writes.encoded_batches(nblocks, per_batch, worst, encode)

    plans = [plan(h, w) for h, w in [(H, W)] + shapes]   # (every refusal before any device work)
    levels = _device_pyramid(array, H, W, sample_type, nodataval, shapes)
    tags = _image_tags(H, W, dt, comp, predictor, bool(tiled), plans[0][0], plans[0][1], window_bound, nodataval, epsg, bigtiff)
    images = [(_image_tags(h, w, dt, comp, predictor, bool(tiled), p[0], p[1], None, nodataval, None, bigtiff, overview=True),
               streams(level, h, w, *p)) for (h, w), p, level in zip(shapes, plans[1:], levels)]
    return _write_container(f"{outfilepath}.tif", bool(bigtiff), tags, streams(array, H, W, *plans[0]), images)


def read_geotiff(path, overview=0):
    """Decodes a file written by save_array_to_grid or write_geotiff_resident.  Returns (array (1, H, W), info dict with the GeoTIFF
    tags).  Predictor 2 is undone in the package's own files, recognised by the directory its writers always write (ModelPixelScale,
    ModelTiepoint, GeoKeyDirectory and GDAL_NODATA all present).  In any other file the Predictor tag is ignored, as it always was
    (tests/test_geotiff_open_host.py pins that): files of other writers are read by open_geotiff / read_geotiff_resident.
    overview = k > 0: the k-th reduced-resolution image behind the first one (a directory whose NewSubfileType (254) has bit 0 set and
    bit 2, mask, clear) instead; its info holds its own tags, and the first directory's GDAL_NODATA where it has none."""
    with open(path, "rb") as f:
        buf = f.read()
    big = struct.unpack_from("<H", buf, 2)[0] == 43
    assert buf[:2] == b"II" and struct.unpack_from("<H", buf, 2)[0] in (42, 43)

    def directory(ifd):
        n = struct.unpack_from("<Q" if big else "<H", buf, ifd)[0]
        pos = ifd + (8 if big else 2)
        tags = {}
        for _ in range(n):
            tag, typ, count = struct.unpack_from("<HHQ" if big else "<HHI", buf, pos)
            fmt, size = _TYPES[typ]
            fpos = pos + (12 if big else 8)
            if count * size > (8 if big else 4):
                fpos = struct.unpack_from("<Q" if big else "<I", buf, fpos)[0]
            tags[tag] = buf[fpos:fpos + count] if typ == 2 else list(struct.unpack_from("<%d%s" % (count, fmt), buf, fpos))
            pos += 20 if big else 12
        return tags, struct.unpack_from("<Q" if big else "<I", buf, pos)[0]

    tags, nxt = directory(struct.unpack_from("<Q", buf, 8)[0] if big else struct.unpack_from("<I", buf, 4)[0])
    own = all(t in tags for t in (33550, 33922, 34735, 42113))   # the directory of _image_tags
    if _overview_of(overview, "read_geotiff"):
        base, found, seen = tags, 0, set()
        while found < overview:
            if nxt == 0:
                raise ValueError(f"{path}: overview {overview} asked for, the file holds {found}")
            if nxt in seen or nxt + (8 if big else 2) > len(buf):
                raise ValueError(f"{path}: the image directory at offset {nxt} repeats or lies outside the file")
            seen.add(nxt)
            tags, nxt = directory(nxt)
            found += tags.get(254, [0])[0] & 5 == 1
        tags.setdefault(42113, base.get(42113, b""))
    W, H, bits, comp, fmtc = tags[256][0], tags[257][0], tags[258][0], tags[259][0], tags.get(339, [1])[0]
    dt = np.dtype({(16, 2): "<i2", (16, 1): "<u2", (32, 3): "<f4", (32, 2): "<i4", (8, 1): "u1", (64, 3): "<f8"}[(bits, fmtc)])
    if 322 in tags:
        tw, th, offs, cnts = tags[322][0], tags[323][0], tags[324], tags[325]
    else:
        tw, th, offs, cnts = W, tags[278][0], tags[273], tags[279]
    ny, nx = (H + th - 1) // th, (W + tw - 1) // tw
    out = np.zeros((ny * th, nx * tw), dtype=dt)
    predictor = tags.get(317, [1])[0] if own and comp == 5 else 1   # (without effect on uncompressed data)
    assert predictor in (1, 2), predictor
    for i, (o, c) in enumerate(zip(offs, cnts)):
        ty, tx = divmod(i, nx)
        rows = th if 322 in tags else min(th, H - ty * th)  # (the last strip holds only the rows that exist)
        raw = lzw_decode(buf[o:o + c], rows * tw * dt.itemsize) if comp == 5 else np.frombuffer(buf[o:o + c], dtype=np.uint8)
        block = raw.view(dt).reshape(rows, tw)
        if predictor == 2:   # a running sum along the row, wrapping in the sample's own width (floats: on the bit patterns)
            u = np.dtype("<u%d" % dt.itemsize)
            block = np.cumsum(block.view(u), axis=1, dtype=u).view(dt)
        out[ty * th:ty * th + rows, tx * tw:(tx + 1) * tw] = block
    info = {"pixel_scale": tags.get(33550), "tiepoint": tags.get(33922), "geokeys": tags.get(34735),
            "nodata": tags.get(42113, b"").rstrip(b"\0").decode(), "bigtiff": big, "compression": comp, "tile": (th, tw)}
    return out[None, :H, :W], info


# ---- opening GeoTIFFs as GDAL and libtiff write them: header and block plan on the host, blocks decoded on the GPU ----
_FIELD_TYPES = {1: ("B", 1), 2: ("s", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4),
                10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 13: ("I", 4), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}
# (BitsPerSample, SampleFormat) -> (NumPy dtype, dbm_tiff_decode's sample_type)
_SAMPLES = {(8, 1): ("u1", 0), (16, 2): ("<i2", 1), (16, 1): ("<u2", 2), (32, 2): ("<i4", 3), (32, 3): ("<f4", 4), (64, 3): ("<f8", 5)}
_COMPRESSIONS = {1: "none", 5: "lzw", 8: "deflate", 32946: "deflate"}
INFLATE_DEFAULT = "device"    # where read_geotiff_resident inflates deflate blocks (the measurement that decided it)


class GeoTiffFile:
    """One image of a TIFF / BigTIFF file as `open_geotiff` accepts it (one sample per pixel, little endian): the first one, or with
    `base` (the GeoTiffFile of the first one) its overview number `overview` >= 1 -- the same checks, and from the base what the
    directory lacks: GDAL_NODATA, the geokeys and the geometry (the base's outer pixel-edge box divided into this image's pixels).
    overview_count: the overviews behind the first image."""

    def __init__(self, path, bigtiff, tags, base=None, overview=0, overview_count=0):
        self.path, self.bigtiff, self.tags = path, bigtiff, tags
        self.overview, self.overview_count = overview, overview_count

        def one(tag, default=None):
            v = tags.get(tag)
            return default if v is None else v[0]

        self.width, self.height = one(256), one(257)
        if self.width is None or self.height is None or self.width < 1 or self.height < 1:
            raise ValueError(f"{path}: ImageWidth (256) = {self.width}, ImageLength (257) = {self.height}: not an image")
        spp = one(277, 1)
        if spp != 1:
            raise ValueError(f"{path}: SamplesPerPixel (277) = {spp}: only one sample per pixel is read (multi-band files are out of scope)")
        bits, fmt = one(258, 1), one(339, 1)
        if (bits, fmt) not in _SAMPLES:
            raise ValueError(f"{path}: BitsPerSample (258) = {bits} with SampleFormat (339) = {fmt}: the sample types read are uint8, int16, "
                             "uint16, int32, float32 and float64")
        self.dtype, self.sample_type = np.dtype(_SAMPLES[(bits, fmt)][0]), _SAMPLES[(bits, fmt)][1]
        self.compression = one(259, 1)
        if self.compression not in _COMPRESSIONS:
            raise ValueError(f"{path}: Compression (259) = {self.compression}: only 1 (none), 5 (LZW) and 8 / 32946 (deflate) are read")
        if one(266, 1) != 1:
            raise ValueError(f"{path}: FillOrder (266) = {one(266)}: only 1 (most significant bit first) is read")
        self.predictor = one(317, 1)
        if self.predictor not in (1, 2, 3) or (self.predictor == 3 and self.dtype.kind != "f"):
            raise ValueError(f"{path}: Predictor (317) = {self.predictor} with {self.dtype.name} samples: 1, 2, and 3 for floating point "
                             "samples, are read")
        if self.compression == 1:
            self.predictor = 1   # libtiff's predictors are part of its LZW / deflate codecs: on uncompressed data the tag has no effect
        self.tiled = 322 in tags or 323 in tags
        if self.tiled:
            if not (322 in tags and 323 in tags and 324 in tags and 325 in tags):
                raise ValueError(f"{path}: a tiled file needs TileWidth (322), TileLength (323), TileOffsets (324) and TileByteCounts (325)")
            self.block_w, self.block_h, self.offsets, self.counts = one(322), one(323), tags[324], tags[325]
        else:
            if not (273 in tags and 279 in tags):
                raise ValueError(f"{path}: StripOffsets (273) and StripByteCounts (279) are missing")
            self.block_w, self.block_h = self.width, min(one(278, self.height), self.height)
            self.offsets, self.counts = tags[273], tags[279]
        if self.block_w < 1 or self.block_h < 1:
            raise ValueError(f"{path}: blocks of {self.block_h} x {self.block_w}")
        self.blocks_y, self.blocks_x = -(-self.height // self.block_h), -(-self.width // self.block_w)
        n = self.blocks_y * self.blocks_x
        if len(self.offsets) != n or len(self.counts) != n:
            raise ValueError(f"{path}: {len(self.offsets)} block offsets and {len(self.counts)} byte counts for {n} blocks")
        if self.block_h * self.block_w * self.dtype.itemsize >= 1 << 31:
            raise ValueError(f"{path}: blocks of {self.block_h} x {self.block_w} samples hold 2^31 bytes or more")
        self.nodata = tags.get(42113, b"").split(b"\0")[0].decode("ascii", "replace").strip()
        self.pixel_scale, self.tiepoint, self.geokeys = tags.get(33550), tags.get(33922), tags.get(34735)
        self._geometry = self._parse_geometry()
        if base is not None:
            if 42113 not in tags:
                self.nodata = base.nodata
            if self.geokeys is None:
                self.geokeys = base.geokeys
            if isinstance(self._geometry, Exception):
                self._geometry = self._overview_geometry(base)

    def _overview_geometry(self, base):
        """Pixel registration, x0 and y0 centres: the base's outer pixel-edge box is kept and divided into this image's W_k x H_k pixels --
        dx_k = dx W / W_k, x0_k = (x0 - dx / 2) + dx_k / 2, likewise in y, in float64 and in this order.  (The base's error where it
        has no georeference.)"""
        g = base._geometry
        if isinstance(g, Exception):
            return g
        dx, dy = g.dx * base.width / self.width, g.dy * base.height / self.height
        return GridGeometry(x0=(g.x0 - g.dx / 2) + dx / 2, y0=(g.y0 - g.dy / 2) + dy / 2, dx=dx, dy=dy, registration="pixel")

    def _raster_type(self):
        """GTRasterTypeGeoKey (1025): 1 PixelIsArea (the default), 2 PixelIsPoint."""
        k = self.geokeys or []
        for i in range(4, len(k) - 3, 4):
            if k[i] == 1025 and k[i + 1] == 0:
                return k[i + 3]
        return 1

    def _parse_geometry(self):
        """GridGeometry of the whole image, or the ValueError that asking for it raises."""
        point = self._raster_type() == 2
        shift = 0.0 if point else 0.5   # PixelIsPoint: the nodes sit on the tiepoint, not half a pixel in
        m = self.tags.get(34264)
        if self.pixel_scale is not None and self.tiepoint is not None and len(self.pixel_scale) >= 2 and len(self.tiepoint) >= 6:
            px, py = self.pixel_scale[0], self.pixel_scale[1]
            i, j, _, x, y, _ = self.tiepoint[:6]
            x0, y0, dx, dy = x + (shift - i) * px, y - (shift - j) * py, px, -py
        elif m is not None and len(m) == 16:
            if m[1] != 0 or m[4] != 0:
                return ValueError(f"{self.path}: ModelTransformation (34264) = {list(m[:8])}...: rotated or sheared rasters are not read")
            x0, y0, dx, dy = m[3] + shift * m[0], m[7] + shift * m[5], m[0], m[5]
        else:
            return ValueError(f"{self.path}: no georeference: ModelPixelScale (33550) with ModelTiepoint (33922), or ModelTransformation "
                              "(34264), is missing")
        try:
            return GridGeometry(x0=x0, y0=y0, dx=dx, dy=dy, registration="pixel")
        except ValueError as e:
            return ValueError(f"{self.path}: ModelPixelScale (33550) = {self.pixel_scale}, ModelTiepoint (33922) = {self.tiepoint}: {e}")

    @property
    def geometry(self):
        if isinstance(self._geometry, Exception):
            raise self._geometry
        return self._geometry

    @property
    def shape(self):
        return self.height, self.width

    def window(self, window_bound=None):
        """(row0, col0, H, W): `block_reads.pixel_window` of this image.  None: the whole image."""
        return block_reads.pixel_window(lambda: self.geometry, self.height, self.width, window_bound, self.path, "the raster")

    def plan(self, window_bound=None):
        """The blocks a read of `window_bound` (None: everything) needs: a BlockPlan."""
        row0, col0, H, W = self.window(window_bound)
        ty = np.arange(row0 // self.block_h, (row0 + H - 1) // self.block_h + 1, dtype=np.int64)
        tx = np.arange(col0 // self.block_w, (col0 + W - 1) // self.block_w + 1, dtype=np.int64)
        ty, tx = (a.ravel() for a in np.meshgrid(ty, tx, indexing="ij"))
        index = ty * self.blocks_x + tx
        blocks = np.empty((index.size, 6), dtype=np.int64)
        blocks[:, BlockPlan.OFFSET] = np.asarray(self.offsets, dtype=np.uint64)[index].astype(np.int64)
        blocks[:, BlockPlan.BYTES] = np.asarray(self.counts, dtype=np.uint64)[index].astype(np.int64)
        blocks[:, BlockPlan.ROWS] = self.block_h if self.tiled else np.minimum(self.block_h, self.height - ty * self.block_h)
        blocks[:, BlockPlan.OUT_ROW] = ty * self.block_h - row0
        blocks[:, BlockPlan.OUT_COL] = tx * self.block_w - col0
        blocks[:, BlockPlan.INDEX] = index
        size = os.path.getsize(self.path)
        for b in blocks:
            tagname = "TileByteCounts (325)" if self.tiled else "StripByteCounts (279)"
            if b[BlockPlan.BYTES] < 1:
                raise ValueError(f"{self.path}: {tagname}[{b[BlockPlan.INDEX]}] = {b[BlockPlan.BYTES]}: sparse (absent) blocks are not read")
            if b[BlockPlan.OFFSET] < 0 or b[BlockPlan.OFFSET] + b[BlockPlan.BYTES] > size:
                raise ValueError(f"{self.path}: block {b[BlockPlan.INDEX]} (offset {b[BlockPlan.OFFSET]}, {b[BlockPlan.BYTES]} bytes) lies "
                                 f"outside the file ({size} bytes)")
        return BlockPlan((row0, col0, H, W), blocks, (self.block_h, self.block_w))


def _read_tags(f, path):
    head = f.read(16)
    if head[:2] == b"MM":
        raise ValueError(f"{path}: byte order 'MM': big-endian TIFFs are not read")
    if len(head) < 8 or head[:2] != b"II":
        raise ValueError(f"{path}: byte order {head[:2]!r}: not a TIFF file")
    magic = struct.unpack_from("<H", head, 2)[0]
    if magic not in (42, 43):
        raise ValueError(f"{path}: TIFF version {magic}: neither classic TIFF (42) nor BigTIFF (43)")
    big = magic == 43
    if big and struct.unpack_from("<HH", head, 4) != (8, 0):
        raise ValueError(f"{path}: BigTIFF offset size {struct.unpack_from('<HH', head, 4)}: must be (8, 0)")
    ifd = struct.unpack_from("<Q", head, 8)[0] if big else struct.unpack_from("<I", head, 4)[0]
    size = os.fstat(f.fileno()).st_size

    def at(pos, n, what):
        if pos < 0 or pos + n > size:
            raise ValueError(f"{path}: {what} at offset {pos} ({n} bytes) lies outside the file ({size} bytes)")
        f.seek(pos)
        return f.read(n)

    cnt_fmt, cnt_size, entry_size, inline = ("<Q", 8, 20, 8) if big else ("<H", 2, 12, 4)
    directories, seen = [], set()
    while ifd != 0 or not directories:
        name = "the first IFD" if not directories else f"IFD {len(directories)}"
        if ifd in seen:
            raise ValueError(f"{path}: {name} at offset {ifd}: the chain of image directories comes back to this offset")
        seen.add(ifd)
        tags, ifd = _read_directory(at, ifd, name, big, cnt_fmt, cnt_size, entry_size, inline)
        directories.append(tags)
    return big, directories


def _read_directory(at, ifd, name, big, cnt_fmt, cnt_size, entry_size, inline):
    """The tags of the image directory at offset `ifd`, and the offset of the next one (0: none)."""
    n = struct.unpack(cnt_fmt, at(ifd, cnt_size, name))[0]
    table = at(ifd + cnt_size, n * entry_size + inline, f"{name}'s entries")
    tags = {}
    for k in range(n):
        tag, typ, count = struct.unpack_from("<HHQ" if big else "<HHI", table, k * entry_size)
        if typ not in _FIELD_TYPES:
            continue   # (a field type of a later TIFF revision: the tag is unknown to this reader anyway)
        fmt, esize = _FIELD_TYPES[typ]
        vpos = k * entry_size + (12 if big else 8)
        if count * esize <= inline:
            data = table[vpos:vpos + count * esize]
        else:
            data = at(struct.unpack_from("<Q" if big else "<I", table, vpos)[0], count * esize, f"the values of tag {tag}")
        if typ == 2:
            tags[tag] = data
        elif len(fmt) == 1 and count > 64:
            tags[tag] = np.frombuffer(data, dtype=np.dtype("<" + {"B": "u1", "b": "i1", "H": "u2", "h": "i2", "I": "u4", "i": "i4", "Q": "u8",
                                                                   "q": "i8", "f": "f4", "d": "f8"}[fmt]))
        else:
            tags[tag] = list(struct.unpack("<" + fmt * count, data))
    return tags, struct.unpack_from("<Q" if big else "<I", table, n * entry_size)[0]


def _overview_of(overview, who):
    if isinstance(overview, (bool, np.bool_)) or not isinstance(overview, (int, np.integer)) or overview < 0:
        raise ValueError(f"{who}: overview {overview!r}: an int >= 0 (0: the first image)")
    return int(overview)


def open_geotiff(path, overview=0):
    """Parses the header and the image directories of a TIFF / BigTIFF file as GDAL and libtiff write them: little endian,
    strips or tiles, one sample per pixel of uint8 / int16 / uint16 / int32 / float32 / float64, Compression 1 / 5 (LZW) / 8 or
    32946 (deflate), Predictor 1 / 2 / 3.  Everything else raises ValueError naming the tag and its value -- here, before any
    device work.  Returns the GeoTiffFile of the first image, or of its overview number `overview`: the later directories whose
    NewSubfileType (254) has bit 0 (reduced resolution) set and bit 2 (mask) clear are the overviews 1, 2, ... in file order; masks
    and anything else are skipped.  An overview passes the same checks, may be compressed and cut differently from the first
    image, and takes GDAL_NODATA and the georeference from it where it has none.  More than the file holds: a ValueError that says
    how many it has."""
    path = os.fspath(path)
    overview = _overview_of(overview, "open_geotiff")
    with open(path, "rb") as f:
        big, directories = _read_tags(f, path)
        overviews = [t for t in directories[1:] if (t[254][0] if len(t.get(254, ())) else 0) & 5 == 1]
        if overview > len(overviews):
            raise ValueError(f"{path}: overview {overview} asked for, the file holds {len(overviews)}")
        gf = GeoTiffFile(path, big, directories[0], overview_count=len(overviews))
        if overview:
            gf = GeoTiffFile(path, big, overviews[overview - 1], base=gf, overview=overview, overview_count=len(overviews))
        if gf.compression == 5:
            # old-style LZW (TIFF 5.0 writers: least significant bit first) starts with the bytes 00 01; TIFF 6.0 streams with ClearCode
            for o, c in zip(gf.offsets, gf.counts):
                if c >= 2:
                    f.seek(int(o))
                    first = f.read(2)
                    if len(first) == 2 and first[0] == 0 and first[1] & 1:
                        raise ValueError(f"{path}: Compression (259) = 5 with a stream that starts {first.hex()}: old-style LZW (least "
                                         "significant bit first) is not read")
                    break
    return gf


def _batches(gf, plan, limit, streams=None):
    """`block_reads.batches` of a plan; streams: the streams themselves are uploaded (None: as for LZW, which always is)."""
    return block_reads.batches(plan.blocks[:, BlockPlan.BYTES], plan.decoded_bytes(gf.dtype.itemsize), limit,
                               gf.compression == 5 if streams is None else streams)


def read_geotiff_resident(path, window_bound=None, workspace_limit=None, ctx=None, inflate=INFLATE_DEFAULT, overview=0):
    """Decodes a GeoTIFF (`open_geotiff`'s dialect) into HBM: LZW, deflate, the predictors, the conversion to float32 (NumPy's `astype`)
    and the placement run on the GPU (dbm_tiff_decode), so only the compressed bytes cross PCIe.  inflate="host" inflates deflate
    streams with zlib on host threads and uploads the decoded blocks instead (DESIGN.md 6i has the measurements behind the default);
    files that are not deflate read the same either way.  window_bound = (minx, miny,
    maxx, maxy) reads the pixels whose centres lie in [minx, maxx) x (miny, maxy] and only the blocks that hold them.
    workspace_limit: bytes of block staging per batch (default 1 GiB; at least one block goes through at a time).
    overview = k > 0 reads the file's k-th overview instead of its first image (`open_geotiff`): everything above, window_bound included,
    then applies to that image, whose geometry is the first image's pixel-edge box divided into its own pixels.
    Returns (DeviceArray (H, W), info): read_geotiff's keys plus predictor, dtype, window (row0, col0, H, W) and geometry (the
    window's GridGeometry, None for a file without georeference)."""
    workspace_limit = block_reads.read_options(workspace_limit, inflate, "read_geotiff_resident")
    gf = open_geotiff(path, _overview_of(overview, "read_geotiff_resident"))
    on_device = gf.compression == 5 or (gf.compression != 1 and inflate == "device")   # the streams themselves are uploaded
    if window_bound is None:
        geometry = None if isinstance(gf._geometry, Exception) else gf._geometry
    else:
        geometry = gf.geometry
    plan = gf.plan(window_bound)
    row0, col0, H, W = plan.window
    ctx = ctx or _lib.default_context()
    out = DeviceArray((H, W), ctx)
    mode = 1 if not on_device else 5 if gf.compression == 5 else 8
    with open(gf.path, "rb") as f:
        def read(b):
            f.seek(int(b[BlockPlan.OFFSET]))
            s = f.read(int(b[BlockPlan.BYTES]))
            if len(s) != b[BlockPlan.BYTES]:
                raise _lib.DbmError(f"{gf.path}: block {b[BlockPlan.INDEX]}: the file ends inside its {b[BlockPlan.BYTES]} bytes")
            return s

        for payload, table in block_reads.staged_batches(plan, slice(None), gf.dtype.itemsize, workspace_limit, read, on_device,
                                                         gf.compression != 1, 0, False, gf.path):
            block_reads.decode_call(ctx, gf.path, "dbm_tiff_decode", devptr(payload), payload.size, devptr(table), len(table), mode,
                                    gf.predictor, gf.sample_type, gf.block_w, gf.block_h, devptr(out), H, W)
    out.written()
    info = {"pixel_scale": gf.pixel_scale, "tiepoint": gf.tiepoint, "geokeys": gf.geokeys, "nodata": gf.nodata, "bigtiff": gf.bigtiff,
            "compression": gf.compression, "tile": (gf.block_h, gf.block_w), "predictor": gf.predictor, "dtype": gf.dtype,
            "window": plan.window, "geometry": block_reads.window_geometry(geometry, row0, col0)}
    return out, info
