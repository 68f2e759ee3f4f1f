"""What the block writers share: `write_geotiff_resident` (strips and tiles, dbm_tiff_encode), `write_netcdf_resident`
(chunks, dbm_chunk_encode) and the PNG writers (bands, dbm_png_encode and dbm_png_encode_host) all check a workspace limit, work out
how many blocks one call of their entry point takes, and walk the packed streams that come back, batch after batch.  Nothing here
knows a format: the containers, the blocks' shapes and worst cases, the refusals and the entry points' own arguments stay in
geotiff.py, netcdf.py and relief.py.
"""
import numpy as np

from .resident import WORKSPACE_DEFAULT, DeviceArray


def deflate_slot(nbytes):
    """The bytes that always hold the stream of `nbytes` input bytes: no input byte costs more than 9 bits."""
    return nbytes + nbytes // 8 + 16


def write_options(workspace_limit, who):
    """The checked `workspace_limit` (None: WORKSPACE_DEFAULT) of the resident writer `who`."""
    if workspace_limit is None:
        return WORKSPACE_DEFAULT
    try:
        limit = int(workspace_limit)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: workspace_limit {workspace_limit!r} is not a number of bytes") from None
    if limit < 1:
        raise ValueError(f"{who}: workspace_limit must be positive")
    return limit


def resident_plane_to_write(array, who, host_writer):
    """The DeviceArray behind `array`, a DeviceArray or a resident Raster; anything else is refused with the host writer's name."""
    from .tiling import Raster

    if isinstance(array, Raster):
        if array._dev is None:
            raise ValueError(f"{who}: array: the Raster is not resident (a NumPy raster is written by {host_writer})")
        array = array._dev
    if not isinstance(array, DeviceArray):
        raise ValueError(f"{who}: array must be a float32 DeviceArray or a resident Raster, not {type(array).__name__} "
                         f"(a NumPy array is written by {host_writer})")
    return array


def blocks_per_call(limit, raw_bytes, slot_bytes, launch_units, nblocks):
    """Blocks per call of an entry point: as many as keep the raw blocks plus their stream slots (slot_bytes = 0: the blocks are not
    encoded) within `limit` bytes and the launch's grid, `launch_units` per block, below 2^31; never more than there are, at least one."""
    return max(1, min(limit // (raw_bytes + slot_bytes), ((1 << 31) - 1) // launch_units, nblocks))


def encoded_batches(nblocks, per_batch, worst, encode, extras=()):
    """The stream of every block in order, `per_batch` blocks per call of encode(first, n, out, sizes, *extra_arrays): the caller's
    closure around its entry point.  worst: the most bytes one block's stream takes; extras: the dtypes of per-block side arrays the
    entry point fills next to `sizes`: with them a block's item is the tuple (stream, *its extras).  The layout of `out` is the one
    of `pack_streams` (api_data.hip), stated here and nowhere else in Python: block k's sizes[k] bytes start at the even offset
    behind block k - 1's, the first at 0.  A stream is a memoryview into the one buffer that every batch reuses: it holds until the
    next item is taken."""
    out = np.empty(per_batch * ((worst + 1) & ~1), dtype=np.uint8)
    sizes = np.zeros(per_batch, dtype=np.uintp)
    side = [np.zeros(per_batch, dtype=dtype) for dtype in extras]
    view = memoryview(out)
    for first in range(0, nblocks, per_batch):
        n = min(per_batch, nblocks - first)
        encode(first, n, out, sizes, *side)
        pos = 0
        for k in range(n):
            size = int(sizes[k])
            yield (view[pos:pos + size], *(int(a[k]) for a in side)) if side else view[pos:pos + size]
            pos += (size + 1) & ~1
