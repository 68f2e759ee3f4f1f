"""What the block readers share: `read_geotiff_resident` (strips and tiles, dbm_tiff_decode) and `read_netcdf_resident`
(chunks and row bands, dbm_chunk_decode) both turn a window of a file into a plan of blocks, cut the plan into batches within a
workspace limit, stage each batch -- the streams as they are stored, or the decoded blocks in slots -- and hand it to their entry
point with an int64 (n, 8) table.  Nothing here knows a format: the containers, their refusals and the entry points' own arguments
stay in geotiff.py and netcdf.py.
"""
import dataclasses
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .resident import WORKSPACE_DEFAULT   # (block_writes.py takes the same default)


class BlockPlan:
    """What one (windowed) read takes from the file.  `window` = (row0, col0, H, W) in the pixels of the image as it is RETURNED;
    `blocks` = int64, one row per block (strip, tile, chunk, row band) that meets the window: file offset, stored bytes, rows the block
    holds (a last strip is short; tiles and chunks are whole), row and column of the block's pixel (0, 0) in the OUTPUT plane (negative
    where the block starts before the window), block index, row step (+1, or -1 for a file whose rows ascend), filter mask.  A plan of
    six columns (GeoTIFF) has neither: its rows step +1 and it has no filters.  `block_shape`: (block_h, block_w) of every block."""
    OFFSET, BYTES, ROWS, OUT_ROW, OUT_COL, INDEX, STEP, MASK = range(8)

    def __init__(self, window, blocks, block_shape):
        self.window, self.blocks, self.block_shape = tuple(int(v) for v in window), blocks, tuple(int(v) for v in block_shape)

    def __len__(self):
        return len(self.blocks)

    def decoded_bytes(self, itemsize):
        """A whole decoded block's slot in the staging area: its bytes rounded up to 16."""
        return -(-self.block_shape[0] * self.block_shape[1] * itemsize // 16) * 16


def pixel_window(geometry, H, W, window_bound, path, of):
    """(row0, col0, H, W): the pixels of an (H, W) image whose centres lie in [minx, maxx) x (miny, maxy] -- for bounds on pixel edges
    the reference's `rasterio.windows.from_bounds(...).round_offsets()` --, clipped to the image.  None: the whole image.  geometry: a
    callable that returns the image's GridGeometry or raises the caller's refusal; it is asked only for finite bounds."""
    if window_bound is None:
        return 0, 0, H, W
    minx, miny, maxx, maxy = (float(v) for v in window_bound)
    if not all(np.isfinite(v) for v in (minx, miny, maxx, maxy)):
        raise ValueError("window_bound must be finite")
    g = geometry()
    xc = np.arange(W, dtype=np.float64) * g.dx + g.x0    # (node coordinates as everywhere: multiply, then add)
    yc = np.arange(H, dtype=np.float64) * g.dy + g.y0
    cols = np.flatnonzero((xc >= minx) & (xc < maxx))
    rows = np.flatnonzero((yc > miny) & (yc <= maxy))
    if cols.size == 0 or rows.size == 0:
        raise ValueError(f"{path}: window_bound {(minx, miny, maxx, maxy)} holds no pixel centre of {of}")
    return int(rows[0]), int(cols[0]), int(rows[-1] - rows[0] + 1), int(cols[-1] - cols[0] + 1)


def window_geometry(geometry, row0, col0):
    """The GridGeometry of the window that starts at pixel (row0, col0) of an image of `geometry` (None stays None)."""
    if geometry is None:
        return None
    return dataclasses.replace(geometry, x0=col0 * geometry.dx + geometry.x0, y0=row0 * geometry.dy + geometry.y0)


def read_options(workspace_limit, inflate, who):
    """The checked `workspace_limit` (None: WORKSPACE_DEFAULT) of the resident reader `who`; `inflate` is 'device' or 'host'."""
    workspace_limit = int(WORKSPACE_DEFAULT if workspace_limit is None else workspace_limit)
    if workspace_limit < 1:
        raise ValueError("workspace_limit must be positive")
    if inflate not in ("device", "host"):
        raise ValueError(f"{who}: inflate {inflate!r}: 'device' or 'host'")
    return workspace_limit


def batches(stored_bytes, decoded, limit, uploaded):
    """Consecutive runs (start, stop) over blocks of `stored_bytes` whose staging stays within `limit` bytes; never an empty run.  A
    block costs its decoded slot plus its stream where the streams are uploaded and decoded on the device, else plus 16."""
    runs, start, used = [], 0, 0
    for k, stored in enumerate(stored_bytes):
        cost = decoded + (int(stored) if uploaded else 16)
        if k > start and used + cost > limit:
            runs.append((start, k))
            start, used = k, 0
        used += cost
    runs.append((start, len(stored_bytes)))
    return runs


def inflate_on_host(streams, ids, path):
    """zlib over the streams of the blocks `ids` on host threads; a stream that does not inflate raises DbmError naming its block."""
    def one(k):
        try:
            return zlib.decompress(streams[k])
        except zlib.error as e:
            raise _lib.DbmError(f"{path}: block {ids[k]}: malformed deflate stream ({e})") from None
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(one, range(len(streams))))


def stage(streams, want, decoded, uploaded, exact, ids, path):
    """(payload uint8, offsets, sizes) of one batch.  uploaded: the streams back to back.  Else decoded blocks, block k in the
    `decoded`-byte slot k, zero padded: a block shorter than want[k] bytes is refused, a longer one too if `exact`, else cut."""
    if uploaded:
        sizes = np.array([len(s) for s in streams], dtype=np.int64)
        return np.frombuffer(b"".join(streams), dtype=np.uint8), np.cumsum(sizes) - sizes, sizes
    payload = np.zeros(len(streams) * decoded, dtype=np.uint8)
    for k, s in enumerate(streams):
        if len(s) < want[k] or (exact and len(s) != want[k]):
            raise _lib.DbmError(f"{path}: block {ids[k]}: {len(s)} decoded bytes, {want[k]} expected")
        payload[k * decoded:k * decoded + want[k]] = np.frombuffer(s, dtype=np.uint8, count=int(want[k]))
    return payload, np.arange(len(streams), dtype=np.int64) * decoded, np.asarray(want, dtype=np.int64)


def staged_batches(plan, members, itemsize, limit, read, uploaded, deflated, whole_rows, exact, path):
    """The batches of the blocks `members` (indices into plan.blocks) as (payload, table): what an entry point takes as its streams and
    its int64 (n, 8) block table.  read(block row) -> the block's stored bytes.  uploaded: they go up as they are; else `deflated`
    ones are inflated on host threads first.  A decoded block holds whole_rows rows, or, if that is 0, the rows its plan row names."""
    decoded = plan.decoded_bytes(itemsize)
    blocks = plan.blocks[members]
    for start, stop in batches(blocks[:, BlockPlan.BYTES], decoded, limit, uploaded):
        part = blocks[start:stop]
        ids = part[:, BlockPlan.INDEX]
        streams = [read(b) for b in part]
        if deflated and not uploaded:
            streams = inflate_on_host(streams, ids, path)
        rows = np.full(len(part), whole_rows, dtype=np.int64) if whole_rows else part[:, BlockPlan.ROWS]
        want = rows * (plan.block_shape[1] * itemsize)
        table = np.zeros((len(part), 8), dtype=np.int64)
        held = min(part.shape[1], BlockPlan.MASK)   # (the filter mask stays here; a six-column plan leaves the step column 0)
        table[:, BlockPlan.ROWS:held] = part[:, BlockPlan.ROWS:held]
        payload, table[:, 0], table[:, 1] = stage(streams, want, decoded, uploaded, exact, ids, path)
        yield payload, table


def decode_call(ctx, path, name, *args):
    """ctx.call(name, *args); a DbmError comes back with the file's path in front and its code kept."""
    try:
        return ctx.call(name, *args)
    except _lib.DbmError as e:
        err = _lib.DbmError(f"{path}: {e}")
        err.code = e.code
        raise err from None
