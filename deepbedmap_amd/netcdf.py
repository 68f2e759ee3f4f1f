"""Opening netCDF grids (reference data_prep.py:889-900 and deepbedmap.py:176-191: the ice velocity `netcdf:FILE:VX` / `:VY`;
deepbedmap.py:74-78 and :437: the ground-truth grids, through xarray / rasterio) without h5py, netCDF4 or xarray.  DESIGN.md 6l.

netCDF-4 files are HDF5 containers: `open_netcdf` parses the dialect netCDF-C, GMT and xarray write with the library's low bound
"earliest" -- superblock 0..3, object headers 1 and 2, root group by symbol table or compact links, layout 3 (compact, contiguous,
chunked by a version-1 B-tree), shuffle and deflate -- and the classic formats CDF-1 / CDF-2 (fixed-size variables).  Everything
outside the dialect raises a ValueError that names the structure and the value, before any device work.  Version-2 object header
checksums are NOT verified.  `read_netcdf` is the host reader (zlib, NumPy): the statement of the dialect.  `read_netcdf_resident`
takes only the chunks (or row bands) a window touches and lets dbm_chunk_decode undo the shuffle, put the bytes in order, mask, scale
and place them (nc_chunks.hip); deflated chunks are inflated on the GPU too, so that only stored bytes cross PCIe, or, with
inflate="host", by zlib on host threads.

Values, this package's own rule (not xarray's dtype promotion): fill = `_FillValue`, else `missing_value`; a sample equal to it BY
VALUE in its stored type becomes NaN (-0.0 equals 0.0; a NaN fill matches every NaN); with `scale_factor` or `add_offset` every other
sample is float32(float64(v) * scale + offset), two rounded float64 operations and one rounding to float32; otherwise
v.astype(float32) (float32 keeps its bits).  A chunk that was never written reads as the storage fill value through the same rule
(0 if none is defined).  A file whose y ascends is returned north-up.

Writing (reference data_prep.py:826-830: `save_array_to_grid(save_netcdf=True)`; data_prep.py:410-441: `xyz_to_grid(outfile=...)`;
DESIGN.md 6m): `save_grid_to_netcdf` (host) and `write_netcdf_resident` (dbm_chunk_encode: chunks cut, shuffled and deflated on the
GPU, only the stored bytes cross PCIe) write one float32 variable over y, x as a netCDF-4 file of the dialect above, byte for byte the
same file from either; the second half of this module.
"""
import dataclasses
import os
import struct

import numpy as np

from . import _lib, block_reads
from .block_reads import BlockPlan as ChunkPlan   # (the plan of a netCDF variable holds all eight columns)
from .block_writes import blocks_per_call, deflate_slot, encoded_batches, resident_plane_to_write, write_options
from .resident import DeviceArray, GridGeometry, devptr

INFLATE_DEFAULT = "device"    # where read_netcdf_resident inflates deflated chunks (the measurements that decided it)
BAND_BYTES = 1 << 24          # contiguous and classic data go through as row bands of about this many bytes (always < 2^31)

_SIGNATURE = b"\x89HDF\r\n\x1a\n"
_UNDEF = 0xFFFFFFFFFFFFFFFF
_FILTER_NAMES = {1: "deflate", 2: "shuffle", 3: "fletcher32", 4: "szip", 5: "nbit", 6: "scaleoffset", 32000: "lzf", 32001: "blosc",
                 32004: "lz4", 32008: "bitshuffle", 32015: "zstd"}
# NumPy kind + size -> dbm_chunk_decode's sample_type
_SAMPLE_TYPES = {("u", 1): 0, ("i", 2): 1, ("u", 2): 2, ("i", 4): 3, ("f", 4): 4, ("f", 8): 5, ("i", 1): 6}
_NEEDED = ("_FillValue", "missing_value", "scale_factor", "add_offset", "node_offset")
_CLASSIC_TYPES = {1: ">i1", 2: "S1", 3: ">i2", 4: ">i4", 5: ">f4", 6: ">f8"}


class _File:
    """The bytes of a file with checked reads: every structure is read through `at`, which names it when it lies outside."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            self.size = os.fstat(f.fileno()).st_size
            # headers are small and scattered: the file is mapped, not read
            self.buf = np.memmap(path, dtype=np.uint8, mode="r") if self.size else np.zeros(0, np.uint8)
        self.base = 0

    def at(self, pos, n, what):
        pos, n = int(pos), int(n)
        if pos < 0 or n < 0 or pos + n > self.size:
            raise ValueError(f"{self.path}: {what} at offset {pos} ({n} bytes) lies outside the file ({self.size} bytes): truncated?")
        return bytes(self.buf[pos:pos + n])

    def addr(self, pos, n, what):
        """`at` for an address of the HDF5 file (relative to the base address)."""
        return self.at(self.base + int(pos), n, what)


def _u(data, pos, size):
    return int.from_bytes(data[pos:pos + size], "little")


# ---- HDF5 messages ----
@dataclasses.dataclass
class _Datatype:
    cls: int
    size: int
    dtype: object      # np.dtype with byte order, or None
    text: str          # for messages


def _parse_datatype(d, path, what):
    if len(d) < 8:
        raise ValueError(f"{path}: {what}: datatype message of {len(d)} bytes: truncated")
    cls, version = d[0] & 15, d[0] >> 4
    bits = d[1] | d[2] << 8 | d[3] << 16
    size = _u(d, 4, 4)
    order = ">" if bits & 1 else "<"
    if cls == 0 and len(d) >= 12:
        offset, precision = struct.unpack_from("<HH", d, 8)
        signed = bool(bits & 8)
        text = f"fixed-point, {size} bytes, precision {precision}, bit offset {offset}, {'signed' if signed else 'unsigned'}"
        ok = size in (1, 2, 4, 8) and precision == 8 * size and offset == 0
        return _Datatype(cls, size, np.dtype(f"{order}{'i' if signed else 'u'}{size}") if ok else None, text)
    if cls == 1 and len(d) >= 20:
        offset, precision, eloc, esize, mloc, msize, bias = struct.unpack_from("<HHBBBBI", d, 8)
        text = f"floating-point, {size} bytes, precision {precision}, bit offset {offset}, exponent {esize} bits at {eloc}, mantissa {msize} bits at {mloc}"
        ieee = {4: (32, 23, 8, 0, 23, 127), 8: (64, 52, 11, 0, 52, 1023)}.get(size)
        ok = ieee == (precision, eloc, esize, mloc, msize, bias) and offset == 0 and not bits & 0x40
        return _Datatype(cls, size, np.dtype(f"{order}f{size}") if ok else None, text)
    if cls == 3:
        return _Datatype(cls, size, np.dtype(f"S{size}") if size else None, f"string of {size} bytes")
    names = {2: "time", 4: "bit field", 5: "opaque", 6: "compound", 7: "reference", 8: "enumeration", 9: "variable-length", 10: "array"}
    return _Datatype(cls, size, None, f"{names.get(cls, 'class %d' % cls)} (version {version})")


def _parse_dataspace(d, path, what, L):
    if len(d) < 4:
        raise ValueError(f"{path}: {what}: dataspace message of {len(d)} bytes: truncated")
    version, rank = d[0], d[1]
    if version == 1:
        pos = 8
    elif version == 2:
        pos = 4
        if d[3] == 2:
            return None   # a null dataspace: no elements
    else:
        raise ValueError(f"{path}: {what}: dataspace message version {version}: versions 1 and 2 are read")
    if len(d) < pos + rank * L:
        raise ValueError(f"{path}: {what}: dataspace message of {len(d)} bytes for rank {rank}: truncated")
    return tuple(_u(d, pos + k * L, L) for k in range(rank))


class _Object:
    """The messages of one object header: (type, data, file offset of the data) in order."""

    def __init__(self, f, addr, O, L, name):
        self.f, self.O, self.L, self.name, self.messages = f, O, L, name, []
        head = f.addr(addr, 16, f"the object header of {name!r}")
        if head[:4] == b"OHDR":
            self._v2(addr, head)
        elif head[0] == 1:
            self._v1(addr, head)
        else:
            raise ValueError(f"{f.path}: the object header of {name!r} at address {addr} starts {head[:4]!r}: versions 1 and 2 are read")

    def _v1(self, addr, head):
        f, name = self.f, self.name
        nmsg, size = struct.unpack_from("<H", head, 2)[0], struct.unpack_from("<I", head, 8)[0]
        blocks = [(addr + 16, size)]
        while blocks and len(self.messages) < nmsg + 64:
            start, size = blocks.pop(0)
            data = f.addr(start, size, f"the messages of {name!r}")
            pos = 0
            while pos + 8 <= len(data):
                typ, msize, flags = struct.unpack_from("<HHB", data, pos)
                if pos + 8 + msize > len(data):
                    raise ValueError(f"{f.path}: {name!r}: header message type {typ} of {msize} bytes runs past its block: truncated header")
                body = data[pos + 8:pos + 8 + msize]
                if typ == 0x10:
                    blocks.append((_u(body, 0, self.O), _u(body, self.O, self.L)))
                else:
                    self.messages.append((typ, body, f.base + start + pos + 8, flags))
                pos += 8 + msize

    def _v2(self, addr, head):
        f, name = self.f, self.name
        if head[4] != 2:
            raise ValueError(f"{f.path}: the object header of {name!r} has version {head[4]}: versions 1 and 2 are read")
        flags = head[5]
        pos = 6 + (16 if flags & 0x20 else 0) + (4 if flags & 0x10 else 0)
        width = 1 << (flags & 3)
        head = f.addr(addr, pos + width, f"the object header of {name!r}")
        size = _u(head, pos, width)
        order = 2 if flags & 0x04 else 0
        blocks = [(addr + pos + width, size)]   # (the checksum follows the chunk's `size` bytes of messages)
        seen = 0
        while blocks:
            start, size = blocks.pop(0)
            seen += 1
            if seen > 4096:
                raise ValueError(f"{f.path}: {name!r}: more than 4096 header continuation blocks")
            data = f.addr(start, size, f"the messages of {name!r}")
            p = 0
            while p + 4 + order <= len(data):
                typ, msize, mflags = struct.unpack_from("<BHB", data, p)
                p += 4 + order
                if p + msize > len(data):
                    raise ValueError(f"{f.path}: {name!r}: header message type {typ} of {msize} bytes runs past its block: truncated header")
                body = data[p:p + msize]
                if typ == 0x10:
                    caddr, clen = _u(body, 0, self.O), _u(body, self.O, self.L)
                    if f.addr(caddr, 4, f"a continuation block of {name!r}") != b"OCHK":
                        raise ValueError(f"{f.path}: {name!r}: the continuation block at address {caddr} lacks the signature OCHK")
                    blocks.append((caddr + 4, clen - 8))
                else:
                    self.messages.append((typ, body, f.base + start + p, mflags))
                p += msize

    def find(self, typ):
        return [m for m in self.messages if m[0] == typ]


def _attribute(f, body, L, owner):
    """(name, value or None) of an attribute message (versions 1..3): None for the types that are not decoded."""
    version = body[0]
    if version not in (1, 2, 3):
        raise ValueError(f"{f.path}: {owner}: attribute message version {version}: versions 1 to 3 are read")
    flags = body[1] if version > 1 else 0
    nsize, tsize, ssize = struct.unpack_from("<HHH", body, 2)
    pos = 8 + (1 if version == 3 else 0)
    pad = (lambda n: -(-n // 8) * 8) if version == 1 else (lambda n: n)
    name = body[pos:pos + nsize].split(b"\0")[0].decode("utf-8", "replace")
    pos += pad(nsize)
    tbody = body[pos:pos + tsize]
    pos += pad(tsize)
    sbody = body[pos:pos + ssize]
    pos += pad(ssize)
    what = f"attribute {name!r} of {owner}"
    if flags & 3:
        return name, None, "a shared datatype or dataspace"
    dt = _parse_datatype(tbody, f.path, what)
    shape = _parse_dataspace(sbody, f.path, what, L)
    if dt.dtype is None or shape is None or len(shape) > 1:
        return name, None, dt.text if dt.dtype is None else f"a dataspace of shape {shape}"
    count = shape[0] if shape else 1
    data = body[pos:pos + count * dt.size]
    if len(data) < count * dt.size:
        raise ValueError(f"{f.path}: {what}: {len(data)} bytes of data for {count} values of {dt.size} bytes: truncated")
    value = np.frombuffer(data, dtype=dt.dtype, count=count)
    if dt.cls == 3:
        value = [v.split(b"\0")[0].decode("utf-8", "replace") for v in value.tolist()]
        return name, (value[0] if not shape else value), None
    value = value.astype(dt.dtype.newbyteorder("="))
    return name, (value[0] if not shape else value), None


def _attributes(f, obj, L, owner):
    for typ, body, _, _ in obj.find(0x15):
        if len(body) >= 2:
            pos = 2 + (2 if body[1] & 1 else 0)
            if _u(body, pos, obj.O) != _UNDEF:
                raise ValueError(f"{f.path}: {owner}: dense attribute storage (the attribute-info message carries the fractal-heap address "
                                 f"{_u(body, pos, obj.O)}) is not read: only compact attributes, stored in the object header")
    out = {}
    for typ, body, _, _ in obj.find(0x0C):
        name, value, why = _attribute(f, body, L, owner)
        if value is None and name in _NEEDED:
            raise ValueError(f"{f.path}: attribute {name!r} of {owner} is {why}: scalar and 1-D numeric values and fixed-length strings are decoded")
        if value is not None:
            out[name] = value
    return out


# ---- the root group ----
def _root_links(f, root, O, L):
    """{name: object header address} of the root group's hard links."""
    links = {}
    for typ, body, _, _ in root.find(0x02):     # link info
        pos = 2 + (8 if body[1] & 1 else 0)
        heap = _u(body, pos, O)
        if heap != _UNDEF:
            raise ValueError(f"{f.path}: the root group uses dense link storage (its link-info message carries the fractal-heap address {heap}): "
                             "only compact links, stored in the object header (at most 8 by default), are read")
    for typ, body, _, _ in root.find(0x06):     # link
        if body[0] != 1:
            raise ValueError(f"{f.path}: link message version {body[0]}: version 1 is read")
        flags, pos = body[1], 2
        ltype = 0
        if flags & 0x08:
            ltype, pos = body[pos], pos + 1
        if flags & 0x04:
            pos += 8
        if flags & 0x10:
            pos += 1
        w = 1 << (flags & 3)
        n = _u(body, pos, w)
        pos += w
        name = body[pos:pos + n].decode("utf-8", "replace")
        pos += n
        if ltype == 0:   # (soft and external links are not followed)
            links[name] = _u(body, pos, O)
    for typ, body, _, _ in root.find(0x11):     # symbol table: version-1 B-tree + local heap
        btree, heap = _u(body, 0, O), _u(body, O, O)
        h = f.addr(heap, 8 + 2 * L + O, "the root group's local heap")
        if h[:4] != b"HEAP":
            raise ValueError(f"{f.path}: the root group's local heap at address {heap} lacks the signature HEAP")
        hsize, hdata = _u(h, 8, L), _u(h, 8 + 2 * L, O)
        names = f.addr(hdata, hsize, "the data segment of the root group's local heap")

        def walk(addr, depth=0):
            if depth > 32:
                raise ValueError(f"{f.path}: the root group's B-tree is deeper than 32 levels")
            node = f.addr(addr, 8 + 2 * O, "a node of the root group's B-tree")
            if node[:4] == b"SNOD":
                count = struct.unpack_from("<H", node, 6)[0]
                entries = f.addr(addr + 8, count * (2 * O + 24), "the entries of a symbol-table node")
                for k in range(count):
                    noff, oaddr = _u(entries, k * (2 * O + 24), O), _u(entries, k * (2 * O + 24) + O, O)
                    if noff >= len(names):
                        raise ValueError(f"{f.path}: a symbol-table entry names offset {noff} of a local heap of {len(names)} bytes")
                    links[names[noff:].split(b"\0")[0].decode("utf-8", "replace")] = oaddr
                return
            if node[:4] != b"TREE" or node[4] != 0:
                raise ValueError(f"{f.path}: a node of the root group's B-tree at address {addr} starts {node[:5]!r}: TREE of type 0 or SNOD expected")
            used = struct.unpack_from("<H", node, 6)[0]
            body = f.addr(addr + 8 + 2 * O, used * (L + O) + L, "the keys of a group B-tree node")
            for k in range(used):
                walk(_u(body, L + k * (L + O), O), depth + 1)

        walk(btree)
    return links


# ---- one dataset ----
class NetcdfVariable:
    """One variable of a netCDF file as `open_netcdf` accepts it.  shape (H, W) (rank 1 for the coordinates it reads itself); dtype
    the stored NumPy dtype with its byte order; layout "compact", "contiguous", "chunked" (HDF5) or "classic"; chunk_shape (None unless
    chunked); filters a tuple of "shuffle" / "deflate" in pipeline order; storage_fill the HDF5 fill value (a NumPy scalar of dtype's
    native form, or None); fill / scale / offset: `_FillValue` (else `missing_value`), `scale_factor`, `add_offset` (None: absent);
    attrs the decoded attributes; geometry a GridGeometry of the variable as it is RETURNED (north-up), or None without coordinates;
    flipped: the file's rows run south to north and are reversed on the way out."""

    def __init__(self, f, name, shape, dtype, layout, attrs):
        self.path, self._f, self.name, self.shape, self.dtype, self.layout, self.attrs = f.path, f, name, tuple(shape), dtype, layout, attrs
        self.chunk_shape, self.filters, self.storage_fill = None, (), None
        self._address, self._chunks = None, {}    # contiguous: absolute file offset (None: never written); chunked: index -> (offset, bytes, mask)
        self.geometry, self.flipped = None, False
        native = dtype.newbyteorder("=")

        def number(key):
            v = attrs.get(key)
            if v is None:
                return None
            v = np.asarray(v).ravel()
            if v.size != 1 or v.dtype.kind not in "iuf":
                raise ValueError(f"{self.path}: attribute {key!r} of {name!r} = {attrs[key]!r}: one number expected")
            return v[0]

        fill = number("_FillValue")
        if fill is None:
            fill = number("missing_value")
        with np.errstate(all="ignore"):
            self.fill = None if fill is None else np.asarray(fill).astype(native)[()]
        scale, offset = number("scale_factor"), number("add_offset")
        self.scale = None if scale is None else float(scale)
        self.offset = None if offset is None else float(offset)

    @property
    def sample_type(self):
        return _SAMPLE_TYPES[(self.dtype.kind, self.dtype.itemsize)]

    @property
    def width(self):
        return self.shape[-1]

    @property
    def height(self):
        return self.shape[0] if len(self.shape) == 2 else 1

    def _block_shape(self):
        if self.layout == "chunked":
            return self.chunk_shape if len(self.shape) == 2 else (1, self.chunk_shape[0])
        row = self.width * self.dtype.itemsize
        return max(1, min(self.height, BAND_BYTES // max(row, 1))), self.width

    def window(self, window_bound=None):
        """(row0, col0, H, W) in the returned (north-up) variable: `block_reads.pixel_window`, as GeoTiffFile.window; None: everything."""
        def geometry():
            if self.geometry is None:
                raise ValueError(f"{self.path}: variable {self.name!r} has no coordinates: a window_bound cannot be placed")
            return self.geometry
        return block_reads.pixel_window(geometry, self.height, self.width, window_bound, self.path, repr(self.name))

    def plan(self, window_bound=None):
        """The chunks or row bands a read of `window_bound` (None: everything) needs: a ChunkPlan."""
        row0, col0, H, W = self.window(window_bound)
        FH = self.height
        bh, bw = self._block_shape()
        f0 = FH - row0 - H if self.flipped else row0     # the file rows [f0, f0 + H)
        step = -1 if self.flipped else 1
        rows = []
        if self.layout == "chunked":
            nx = -(-self.width // bw)
            for ty in range(f0 // bh, (f0 + H - 1) // bh + 1):
                for tx in range(col0 // bw, (col0 + W - 1) // bw + 1):
                    index = ty * nx + tx
                    if index not in self._chunks:
                        continue
                    offset, nbytes, mask = self._chunks[index]
                    orow = (FH - 1 - ty * bh - row0) if self.flipped else ty * bh - row0
                    rows.append((offset, nbytes, min(bh, FH - ty * bh), orow, tx * bw - col0, index, step, mask))
        elif self._address is not None:
            rowbytes = self.width * self.dtype.itemsize
            for k, fr in enumerate(range(f0, f0 + H, bh)):
                held = min(bh, f0 + H - fr)
                orow = (FH - 1 - fr - row0) if self.flipped else fr - row0
                rows.append((self._address + fr * rowbytes, held * rowbytes, held, orow, -col0, k, step, 0))
        blocks = np.array(rows, dtype=np.int64).reshape(len(rows), 8)
        for b in blocks:
            if b[ChunkPlan.OFFSET] < 0 or b[ChunkPlan.BYTES] < 1 or b[ChunkPlan.OFFSET] + b[ChunkPlan.BYTES] > self._f.size:
                what = "chunk" if self.layout == "chunked" else "row band"
                raise ValueError(f"{self.path}: {what} {b[ChunkPlan.INDEX]} of {self.name!r} (address {b[ChunkPlan.OFFSET]}, {b[ChunkPlan.BYTES]} bytes) lies "
                                 f"outside the file ({self._f.size} bytes)")
        return ChunkPlan((row0, col0, H, W), blocks, (bh, bw))

    # the filters a block of filter mask `mask` really went through
    def applied(self, mask):
        return tuple(name for k, name in enumerate(self.filters) if not (int(mask) >> k) & 1)

    def storage_fill_value(self):
        """What a cell no chunk covers holds, in the stored type's native form: the storage fill value, or 0."""
        native = self.dtype.newbyteorder("=")
        return np.zeros((), native)[()] if self.storage_fill is None else self.storage_fill


def _hdf5_variable(f, name, addr, O, L, rank_wanted):
    """The NetcdfVariable of the dataset at `addr`, or None if it is not a dataset of one of `rank_wanted` ranks (refusals that concern
    the variable's own type and storage are raised only for rank 2 -- the variable that is asked for -- and for coordinates)."""
    obj = _Object(f, addr, O, L, name)
    spaces, types, layouts = obj.find(0x01), obj.find(0x03), obj.find(0x08)
    if not spaces or not types or not layouts:
        return None    # a group or a committed datatype
    shape = _parse_dataspace(spaces[0][1], f.path, f"variable {name!r}", L)
    if shape is None or len(shape) not in rank_wanted:
        return shape
    who = f"variable {name!r}"
    dt = _parse_datatype(types[0][1], f.path, who)
    if dt.cls not in (0, 1) or dt.dtype is None or (dt.dtype.kind, dt.dtype.itemsize) not in _SAMPLE_TYPES:
        shown = dt.dtype.name if dt.dtype is not None and dt.cls in (0, 1) else dt.text
        raise ValueError(f"{f.path}: {who} has datatype {shown}: int8, uint8, int16, uint16, int32, float32 and float64, little or big "
                         "endian, are read (uint32, 64-bit integers, other precisions and bit offsets are not)")
    if obj.find(0x07):
        raise ValueError(f"{f.path}: {who} uses external storage (an external-data-files message): only data inside the file is read")
    body, body_at = layouts[0][1], layouts[0][2]
    version = body[0]
    if version == 4:
        if body[1] == 3:
            raise ValueError(f"{f.path}: {who} uses virtual storage (layout class 3): not read")
        if body[1] == 2:
            raise ValueError(f"{f.path}: {who} has a version-4 data layout with a chunk index (type {_v4_index(body)}): "
                             "only version 3 (a version-1 B-tree) is read; `h5format_convert` rewrites the file's layout in place")
        raise ValueError(f"{f.path}: {who} has data layout version 4: version 3 is read; `h5format_convert` rewrites it in place")
    if version != 3:
        raise ValueError(f"{f.path}: {who} has data layout version {version}: version 3 is read")
    cls = body[1]
    attrs = _attributes(f, obj, L, who)
    if cls == 0:
        var = NetcdfVariable(f, name, shape, dt.dtype, "compact", attrs)
        var._address = body_at + 4
        have = struct.unpack_from("<H", body, 2)[0]
    elif cls == 1:
        var = NetcdfVariable(f, name, shape, dt.dtype, "contiguous", attrs)
        a = _u(body, 2, O)
        var._address = None if a == _UNDEF else f.base + a
        have = _u(body, 2 + O, L)
    elif cls == 2:
        var = NetcdfVariable(f, name, shape, dt.dtype, "chunked", attrs)
        nd = body[2]
        if nd != len(shape) + 1:
            raise ValueError(f"{f.path}: {who}: chunked layout of dimensionality {nd} for rank {len(shape)}")
        btree = _u(body, 3, O)
        dims = struct.unpack_from("<%dI" % nd, body, 3 + O)
        if dims[-1] != dt.size or min(dims) < 1:
            raise ValueError(f"{f.path}: {who}: chunk dimensions {dims}: the last one must be the element size {dt.size}")
        var.chunk_shape = tuple(dims[:-1])
        if int(np.prod(dims, dtype=np.int64)) >= 1 << 31:
            raise ValueError(f"{f.path}: {who}: chunks of {var.chunk_shape} samples hold 2^31 bytes or more")
        have = None
    else:
        raise ValueError(f"{f.path}: {who} has data layout class {cls}: compact (0), contiguous (1) and chunked (2) are read")
    want = int(np.prod(shape, dtype=np.int64)) * dt.size
    if have is not None and var._address is not None and have < want:
        raise ValueError(f"{f.path}: {who}: {have} bytes of {var.layout} data for {want}")
    # filters
    for typ, fb, _, _ in obj.find(0x0B):
        fv, nf = fb[0], fb[1]
        if fv not in (1, 2):
            raise ValueError(f"{f.path}: {who}: filter pipeline message version {fv}: versions 1 and 2 are read")
        pos, found = (8 if fv == 1 else 2), []
        for _ in range(nf):
            fid = struct.unpack_from("<H", fb, pos)[0]
            pos += 2
            nlen = 0
            if fv == 1 or fid >= 256:
                nlen = struct.unpack_from("<H", fb, pos)[0]
                pos += 2
            _, ncd = struct.unpack_from("<HH", fb, pos)
            pos += 4
            pos += -(-nlen // 8) * 8 if fv == 1 else nlen
            cd = struct.unpack_from("<%dI" % ncd, fb, pos)
            pos += 4 * ncd + (4 if fv == 1 and ncd % 2 else 0)
            if fid not in (1, 2):
                raise ValueError(f"{f.path}: {who}: filter {fid} ({_FILTER_NAMES.get(fid, 'unknown')}): only 2 (shuffle) and 1 (deflate) are read")
            if fid == 2 and (not cd or cd[0] != dt.size):
                raise ValueError(f"{f.path}: {who}: the shuffle filter's element size {cd[0] if cd else None} differs from the type's {dt.size}")
            found.append(_FILTER_NAMES[fid])
        if found not in ([], ["shuffle"], ["deflate"], ["shuffle", "deflate"]):
            raise ValueError(f"{f.path}: {who}: filter pipeline {found}: shuffle, then deflate, each optional and at most once, is read")
        var.filters = tuple(found)
    if var.filters and var.layout != "chunked":
        raise ValueError(f"{f.path}: {who}: filters {var.filters} on {var.layout} data")
    # fill value: the new message wins over the old one
    native = dt.dtype.newbyteorder("=")
    for typ, fb, _, _ in obj.find(0x04):
        n = _u(fb, 0, 4)
        if n == dt.size:
            var.storage_fill = np.frombuffer(fb[4:4 + n], dtype=dt.dtype)[0].astype(native)
    for typ, fb, _, _ in obj.find(0x05):
        fv = fb[0]
        if fv in (1, 2):
            data = fb[8:8 + _u(fb, 4, 4)] if (fv == 1 or fb[3]) and len(fb) >= 8 else b""
            defined = fb[3] != 0
        elif fv == 3:
            defined = bool(fb[1] & 0x20)
            data = fb[6:6 + _u(fb, 2, 4)] if defined else b""
        else:
            raise ValueError(f"{f.path}: {who}: fill-value message version {fv}: versions 1 to 3 are read")
        if defined and len(data) == dt.size:
            var.storage_fill = np.frombuffer(data, dtype=dt.dtype)[0].astype(native)
    if cls == 2 and btree != _UNDEF:
        _chunk_index(f, var, btree, O, len(shape) + 1)
    return var


def _v4_index(body):
    # version 4, chunked: flags(1), dimensionality(1), dimension size width(1), dims, index type
    try:
        nd, w = body[3], body[4]
        return body[5 + nd * w]
    except IndexError:
        return "?"


def _chunk_index(f, var, btree, O, nd):
    """Walks the version-1 B-tree of a chunked dataset: var._chunks[row-major chunk index] = (absolute offset, bytes, filter mask)."""
    cs = var.chunk_shape
    counts = [-(-s // c) for s, c in zip(var.shape, cs)]
    key = 8 + 8 * nd

    def walk(addr, depth):
        if depth > 32:
            raise ValueError(f"{f.path}: the chunk B-tree of {var.name!r} is deeper than 32 levels")
        node = f.addr(addr, 8 + 2 * O, f"a node of the chunk B-tree of {var.name!r}")
        if node[:4] != b"TREE" or node[4] != 1:
            raise ValueError(f"{f.path}: a node of the chunk B-tree of {var.name!r} at address {addr} starts {node[:5]!r}: TREE of type 1 expected")
        level, used = node[5], struct.unpack_from("<H", node, 6)[0]
        body = f.addr(addr + 8 + 2 * O, used * (key + O) + key, f"the keys of a chunk B-tree node of {var.name!r}")
        for k in range(used):
            p = k * (key + O)
            child = _u(body, p + key, O)
            if level > 0:
                walk(child, depth + 1)
                continue
            nbytes, mask = struct.unpack_from("<II", body, p)
            offs = struct.unpack_from("<%dQ" % nd, body, p + 8)
            index = 0
            for o, c, n in zip(offs[:-1], cs, counts):
                if o % c or o // c >= n:
                    raise ValueError(f"{f.path}: chunk of {var.name!r} at offsets {offs[:-1]}: not on the chunk grid {cs} of shape {var.shape}")
                index = index * n + o // c
            var._chunks[index] = (f.base + child, nbytes, mask)

    walk(btree, 0)


def _open_hdf5(f, start):
    head = f.at(start, 16, "the superblock")
    version = head[8]
    if version in (0, 1):
        head = f.at(start, 24 + (4 if version == 1 else 0) + 4 * 8 + 40, "the superblock")
        O, L = head[13], head[14]
        pos = 24 + (4 if version == 1 else 0)
    elif version in (2, 3):
        head = f.at(start, 12 + 4 * 8 + 4, "the superblock")
        O, L = head[9], head[10]
        pos = 12
    else:
        raise ValueError(f"{f.path}: HDF5 superblock version {version}: versions 0 to 3 are read")
    if O != 8 or L != 8:
        raise ValueError(f"{f.path}: HDF5 superblock: offsets of {O} bytes and lengths of {L} bytes: only 8-byte offsets and lengths are read")
    f.base = start    # (the library, too, takes the superblock's own address as the base address)
    if version in (0, 1):
        root = _u(head, pos + 4 * O + O, O)
    else:
        root = _u(head, pos + 3 * O, O)
    return root, O, L


def _classic_header(f):
    """{name: NetcdfVariable} and the global attributes of a CDF-1 / CDF-2 file."""
    path = f.path
    data = f.at(0, min(f.size, 1 << 26), "the classic header")
    big_offsets = data[3] == 2
    pos = 4

    def need(n, what):
        if pos + n > len(data):
            raise ValueError(f"{path}: the classic header ends inside {what} (offset {pos}, {n} bytes, {len(data)} present): truncated header")

    def u32(what):
        nonlocal pos
        need(4, what)
        v = struct.unpack_from(">I", data, pos)[0]
        pos += 4
        return v

    def name(what):
        nonlocal pos
        n = u32(what)
        need(-(-n // 4) * 4, what)
        s = data[pos:pos + n].decode("utf-8", "replace")
        pos += -(-n // 4) * 4
        return s

    def attrs(what):
        nonlocal pos
        tag, n = u32(what), u32(what)
        if tag not in (0, 0x0C) or (tag == 0 and n):
            raise ValueError(f"{path}: {what}: tag {tag} where an attribute list (12) is expected")
        out = {}
        for _ in range(n):
            key = name(what)
            typ, count = u32(what), u32(what)
            if typ not in _CLASSIC_TYPES:
                raise ValueError(f"{path}: attribute {key!r}: nc_type {typ}: 1 (byte) to 6 (double) are read")
            dt = np.dtype(_CLASSIC_TYPES[typ])
            nbytes = -(-count * dt.itemsize // 4) * 4
            need(nbytes, what)
            raw = np.frombuffer(data, dtype=dt, count=count, offset=pos)
            pos += nbytes
            if typ == 2:
                out[key] = raw.tobytes().split(b"\0")[0].decode("utf-8", "replace")
            else:
                v = raw.astype(dt.newbyteorder("="))
                out[key] = v[0] if count == 1 else v
        return out

    numrecs = u32("numrecs")
    tag, n = u32("the dimension list"), u32("the dimension list")
    if tag not in (0, 0x0A) or (tag == 0 and n):
        raise ValueError(f"{path}: tag {tag} where the dimension list (10) is expected")
    dims = []
    for _ in range(n):
        dname = name("a dimension")
        dims.append((dname, u32("a dimension")))
    gattrs = attrs("the global attributes")
    tag, n = u32("the variable list"), u32("the variable list")
    if tag not in (0, 0x0B) or (tag == 0 and n):
        raise ValueError(f"{path}: tag {tag} where the variable list (11) is expected")
    variables = {}
    for _ in range(n):
        vname = name("a variable")
        ids = [u32("a variable's dimensions") for _ in range(u32("a variable's dimensions"))]
        vattrs = attrs(f"the attributes of {vname!r}")
        typ, _vsize = u32("a variable's type"), u32("a variable's size")
        need(8 if big_offsets else 4, "a variable's offset")
        begin = struct.unpack_from(">Q" if big_offsets else ">I", data, pos)[0]
        pos += 8 if big_offsets else 4
        if any(i >= len(dims) for i in ids):
            raise ValueError(f"{path}: variable {vname!r} names dimension {max(ids)} of {len(dims)}")
        variables[vname] = (ids, vattrs, typ, begin)
    del numrecs
    return dims, gattrs, variables


def _classic_variable(f, dims, vname, entry):
    ids, vattrs, typ, begin = entry
    if ids and dims[ids[0]][1] == 0:
        raise ValueError(f"{f.path}: variable {vname!r} is a record variable (its first dimension {dims[ids[0]][0]!r} is the unlimited one): "
                         "only fixed-size variables are read")
    if typ not in (1, 3, 4, 5, 6):
        raise ValueError(f"{f.path}: variable {vname!r} has nc_type {typ}: byte (1), short (3), int (4), float (5) and double (6) are read")
    var = NetcdfVariable(f, vname, tuple(dims[i][1] for i in ids), np.dtype(_CLASSIC_TYPES[typ]), "classic", vattrs)
    var._address = begin
    return var


def _raw_plane(var, plan, decompress):
    """The window of `plan` in the stored type's native form, as the file holds it after its filters are undone (host)."""
    row0, col0, H, W = plan.window
    bh, bw = plan.block_shape
    native = var.dtype.newbyteorder("=")
    out = np.full((H, W), var.storage_fill_value(), dtype=native)
    for b in plan.blocks:
        data = var._f.at(b[ChunkPlan.OFFSET], b[ChunkPlan.BYTES], f"block {b[ChunkPlan.INDEX]} of {var.name!r}")
        applied = var.applied(b[ChunkPlan.MASK])
        rows = int(b[ChunkPlan.ROWS])
        if "deflate" in applied:
            data = decompress(data, b[ChunkPlan.INDEX])
        whole = var.layout == "chunked"
        want = (bh if whole else rows) * bw * var.dtype.itemsize
        if len(data) != want:
            raise _lib.DbmError(f"{var.path}: block {b[ChunkPlan.INDEX]} of {var.name!r}: {len(data)} decoded bytes, {want} expected")
        if "shuffle" in applied:
            data = np.frombuffer(data, dtype=np.uint8).reshape(var.dtype.itemsize, -1).T.tobytes()
        block = np.frombuffer(data, dtype=var.dtype).reshape(-1, bw)[:rows].astype(native)
        step = int(b[ChunkPlan.STEP])
        orows = int(b[ChunkPlan.OUT_ROW]) + step * np.arange(rows)
        ocols = int(b[ChunkPlan.OUT_COL]) + np.arange(bw)
        rk, ck = (orows >= 0) & (orows < H), (ocols >= 0) & (ocols < W)
        out[np.ix_(orows[rk], ocols[ck])] = block[np.ix_(rk, ck)]
    return out


def convert(raw, fill=None, scale=None, offset=None, mask_and_scale=True):
    """The value rule of this module (its docstring) on an array of stored samples in native byte order -> float32."""
    raw = np.asarray(raw)
    if not mask_and_scale:
        fill = scale = offset = None
    with np.errstate(all="ignore"):
        if scale is not None or offset is not None:
            s = np.float64(1.0 if scale is None else scale)
            o = np.float64(0.0 if offset is None else offset)
            out = (raw.astype(np.float64) * s + o).astype(np.float32)
        else:
            out = raw.astype(np.float32)
        if fill is not None:
            fill = np.asarray(fill).astype(raw.dtype)[()]
            mask = np.isnan(raw) if raw.dtype.kind == "f" and np.isnan(fill) else raw == fill
            out = np.where(mask, np.float32(np.nan), out)
    return out


def _coordinates(f, name, get):
    """(the values of the 1-D variable `name` as float64, its attribute `actual_range` as (low, high) or None), or None if the file has
    no such variable."""
    var = get(name, (1,))
    if not isinstance(var, NetcdfVariable):
        return None
    import zlib

    raw = _raw_plane(var, var.plan(None), lambda data, index: zlib.decompress(data))
    span = np.asarray(var.attrs.get("actual_range", ()), dtype=np.float64).ravel()
    return raw.reshape(-1).astype(np.float64), (span if span.size == 2 and np.isfinite(span).all() and span[1] > span[0] else None)


def open_netcdf(path, variable=None, coords=("x", "y")):
    """Parses a netCDF-4 (HDF5) or classic (CDF-1 / CDF-2) file and returns the NetcdfVariable of `variable` (None: the file's only 2-D
    variable; several: a ValueError that lists them).  coords: the names of the 1-D variables that hold the columns' and the rows'
    coordinates; both present: their lengths must be (W, H), the spacing even (GridGeometry.from_coords), and the registration is the
    root attribute `node_offset` (GMT: 1 pixel, 0 gridline), pixel if absent; y ascending: the variable is returned north-up.  Either
    absent: geometry None.  The module docstring has the dialect; everything else raises ValueError."""
    path = os.fspath(path)
    f = _File(path)
    magic = f.at(0, 4, "the file's magic number") if f.size >= 4 else b""
    if magic[:3] == b"CDF":
        if magic[3] == 5:
            raise ValueError(f"{path}: CDF\\x05 (CDF-5, 64-bit data) is not read: classic CDF\\x01 and CDF\\x02 are")
        if magic[3] not in (1, 2):
            raise ValueError(f"{path}: classic netCDF version {magic[3]}: CDF\\x01 and CDF\\x02 are read")
        dims, gattrs, entries = _classic_header(f)
        names = [n for n, e in entries.items() if len(e[0]) == 2]
        others = {n: len(e[0]) for n, e in entries.items() if len(e[0]) not in (1, 2)}

        def get(name, ranks):
            if name not in entries or len(entries[name][0]) not in ranks:
                return None
            return _classic_variable(f, dims, name, entries[name])
    else:
        start, found = 0, False
        while start + 8 <= f.size:
            if f.at(start, 8, "the superblock signature") == _SIGNATURE:
                found = True
                break
            start = 512 if start == 0 else start * 2
        if not found:
            raise ValueError(f"{path}: neither a classic netCDF file (CDF\\x01, CDF\\x02) nor an HDF5 file (no superblock signature at offset 0, "
                             "512, 1024, ...)")
        root_addr, O, L = _open_hdf5(f, start)
        root = _Object(f, root_addr, O, L, "/")
        links = _root_links(f, root, O, L)
        gattrs = _attributes(f, root, L, "the root group")
        cache = {}

        def get(name, ranks):
            if name not in links:
                return None
            if (name, ranks) not in cache:
                cache[(name, ranks)] = _hdf5_variable(f, name, links[name], O, L, ranks)
            return cache[(name, ranks)]

        names, others = [], {}
        for n in sorted(links):
            if variable is None or n == variable:
                obj = _Object(f, links[n], O, L, n)
                sp = obj.find(0x01)
                if sp and obj.find(0x08):
                    shape = _parse_dataspace(sp[0][1], path, f"variable {n!r}", L)
                    if shape is not None and len(shape) == 2:
                        names.append(n)
                    elif shape is not None and len(shape) != 1:
                        others[n] = len(shape)
                    elif n == variable:
                        raise ValueError(f"{path}: variable {n!r} has rank {0 if shape is None else len(shape)} (shape {shape}): only rank 2 is read")
    if variable is None:
        if len(names) != 1:
            if not names and others:
                listed = ", ".join(f"{n!r} has rank {r}" for n, r in sorted(others.items()))
                raise ValueError(f"{path}: no variable of rank 2 ({listed}): only rank 2 is read")
            raise ValueError(f"{path}: {len(names)} variables of rank 2 ({', '.join(sorted(names)) or 'none'}): name one with `variable`")
        variable = names[0]
    var = get(variable, (2,))
    if var is None:
        raise ValueError(f"{path}: no variable {variable!r} in the root group")
    if not isinstance(var, NetcdfVariable):
        raise ValueError(f"{path}: variable {variable!r} has rank {len(var)} (shape {var}): only rank 2 is read")
    if min(var.shape) < 1:
        raise ValueError(f"{path}: variable {variable!r} is empty (shape {var.shape})")
    var.global_attrs = gattrs
    x, y = (_coordinates(f, c, get) for c in coords)
    if x is not None and y is not None:
        (x, xspan), (y, yspan) = x, y
        H, W = var.shape
        if (x.size, y.size) != (W, H):
            raise ValueError(f"{path}: coordinates {coords[0]!r} ({x.size}) and {coords[1]!r} ({y.size}) do not match {variable!r} of shape {var.shape}")
        node = gattrs.get("node_offset")
        if node is not None and int(np.asarray(node).ravel()[0]) not in (0, 1):
            raise ValueError(f"{path}: root attribute node_offset = {node!r}: 0 (gridline) or 1 (pixel)")
        registration = "gridline" if node is not None and int(np.asarray(node).ravel()[0]) == 0 else "pixel"
        # a single pixel has no spacing of its own: `actual_range`, the pixel's edges as GMT and this module's writers record them,
        # gives one (a second node one pixel further: to the east, to the south)
        if registration == "pixel" and x.size == 1 and xspan is not None:
            x = np.array([x[0], x[0] + (xspan[1] - xspan[0])])
        if registration == "pixel" and y.size == 1 and yspan is not None:
            y = np.array([y[0], y[0] - (yspan[1] - yspan[0])])
        try:
            g = GridGeometry.from_coords(x, y, registration=registration)
        except ValueError as e:
            raise ValueError(f"{path}: coordinates {coords[0]!r} / {coords[1]!r} of {variable!r}: {e}") from None
        if g.dy > 0:
            g, var.flipped = g.flipped_rows(H), True
        var.geometry = g
    return var


def _info(var, plan):
    return {"variable": var.name, "dtype": var.dtype, "layout": var.layout, "tile": plan.block_shape, "chunks": var.chunk_shape,
            "filters": var.filters, "fill": var.fill, "scale": var.scale, "offset": var.offset, "storage_fill": var.storage_fill,
            "window": plan.window, "geometry": block_reads.window_geometry(var.geometry, *plan.window[:2]), "flipped": var.flipped,
            "compression": 8 if "deflate" in var.filters else 1}


def read_netcdf(path, variable=None, window_bound=None, mask_and_scale=True, coords=("x", "y")):
    """The host reader (zlib, NumPy): the statement of what `read_netcdf_resident` computes.  Returns (float32 (H, W), info)."""
    import zlib

    var = open_netcdf(path, variable, coords)
    plan = var.plan(window_bound)

    def decompress(data, index):
        try:
            return zlib.decompress(data)
        except zlib.error as e:
            raise _lib.DbmError(f"{var.path}: block {index} of {var.name!r}: malformed deflate stream ({e})") from None

    raw = _raw_plane(var, plan, decompress)
    return convert(raw, var.fill, var.scale, var.offset, mask_and_scale), _info(var, plan)


def _bits(value, dtype):
    """The bits of `value` as the native `dtype`, in an unsigned 64-bit integer."""
    return int(np.asarray(value, dtype=dtype).reshape(1).view(np.dtype("u%d" % dtype.itemsize))[0])


def read_netcdf_resident(path, variable=None, window_bound=None, workspace_limit=None, ctx=None, inflate=INFLATE_DEFAULT,
                         mask_and_scale=True, coords=("x", "y")):
    """Reads a netCDF variable (`open_netcdf`'s dialect) into HBM: only the stored bytes of the chunks (row bands for contiguous and
    classic data) that the window touches cross PCIe; inflating, un-shuffling, byte order, mask, scale and placement run on the GPU
    (dbm_chunk_decode).  inflate="device", the default, uploads the deflated chunks as they are stored and inflates them on the GPU, one
    wavefront per chunk, so that only compressed bytes cross PCIe; inflate="host" inflates with zlib on host threads and uploads the
    inflated (still shuffled) chunks, which is a little faster for a few hundred chunks and several times slower for a thousand --
    DESIGN.md 6l has the measurements behind the default.  window_bound = (minx, miny, maxx, maxy): the pixels whose centres lie in [minx, maxx) x (miny,
    maxy].  workspace_limit: bytes of staging per batch (default 1 GiB; at least one block goes through at a time).  Returns
    (DeviceArray (H, W), info) with read_netcdf's info keys."""
    workspace_limit = block_reads.read_options(workspace_limit, inflate, "read_netcdf_resident")
    var = open_netcdf(path, variable, coords)
    plan = var.plan(window_bound)
    row0, col0, H, W = plan.window
    bh, bw = plan.block_shape
    native = var.dtype.newbyteorder("=")
    fill, scale, offset = (var.fill, var.scale, var.offset) if mask_and_scale else (None, None, None)
    has_scale = scale is not None or offset is not None
    ctx = ctx or _lib.default_context()
    out = DeviceArray((H, W), ctx)
    covered = var.layout != "chunked" and var._address is not None
    if not covered:   # cells that no chunk covers: the storage fill through the value rule
        first = float(convert(np.asarray([var.storage_fill_value()], dtype=native), fill, scale, offset)[0])
        ctx.call("dbm_fill_f32", devptr(out), H * W, first)

    def read(b):
        return var._f.at(b[ChunkPlan.OFFSET], b[ChunkPlan.BYTES], f"block {b[ChunkPlan.INDEX]} of {var.name!r}")

    # groups of blocks that went through the same filters, each cut into batches within the workspace limit
    groups = {}
    for k, b in enumerate(plan.blocks):
        groups.setdefault(var.applied(b[ChunkPlan.MASK]), []).append(k)
    for applied, members in groups.items():
        on_device = "deflate" in applied and inflate == "device"
        for payload, table in block_reads.staged_batches(plan, members, var.dtype.itemsize, workspace_limit, read, on_device,
                                                         "deflate" in applied, bh if var.layout == "chunked" else 0, True, var.path):
            block_reads.decode_call(ctx, var.path, "dbm_chunk_decode", devptr(payload), payload.size, devptr(table), len(table),
                                    8 if on_device else 1, 1 if "shuffle" in applied else 0, var.sample_type,
                                    1 if var.dtype.byteorder == ">" else 0, bw, bh, 0 if fill is None else 1,
                                    0 if fill is None else _bits(fill, native), 1 if has_scale else 0, 1.0 if scale is None else scale,
                                    0.0 if offset is None else offset, devptr(out), H, W)
    out.written()
    return out, _info(var, plan)


# ---- writing ----
# The mirror of the readers above: netCDF-4 files of one float32 variable over the dimensions y, x (reference data_prep.py:826-830:
# `save_array_to_grid(save_netcdf=True)`; data_prep.py:410-441: `xyz_to_grid(outfile=...)`), written without a library.  The dialect
# is the one `open_netcdf` reads and libhdf5 writes with the low bound "earliest": superblock 0, version-1 object headers, the root
# group by symbol table, layout 3, a version-1 B-tree over the chunks.  The file is determined by the arguments: no timestamps.
_GROUP_LEAF_K, _GROUP_INTERNAL_K, _CHUNK_K = 4, 16, 32    # the superblock's two K; version 0 has no field for the third: 32
_FILL_BITS = 0x7FC00000                                   # _FillValue and the storage fill value: the quiet NaN


def deflate_encode_blocks(blocks, nthreads=None):
    """blocks: (n, block_bytes) uint8 -> list of bytes objects: one zlib stream each, fixed Huffman code (dbm_deflate_encode_blocks: the
    device encoder's loop on host threads)."""
    import ctypes as C

    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    nb, nbytes = blocks.shape
    stride = deflate_slot(nbytes)
    out = np.empty((nb, stride), dtype=np.uint8)
    sizes = (C.c_size_t * max(nb, 1))()
    rc = _lib.lib().dbm_deflate_encode_blocks(blocks.ctypes.data_as(C.c_void_p), nbytes, nb, out.ctypes.data_as(C.c_void_p), stride, sizes,
                                              int(nthreads or min(16, os.cpu_count() or 1)))
    if rc != 0:
        raise _lib.DbmError(f"dbm_deflate_encode_blocks failed ({rc})")
    return [out[i, :sizes[i]].tobytes() for i in range(nb)]


def _pad8(data):
    return data + b"\0" * (-len(data) % 8)


def _message(typ, body, flags=0):
    body = _pad8(body)
    return struct.pack("<HHB3x", typ, len(body), flags) + body


def _object_header(messages):
    body = b"".join(messages)
    return struct.pack("<BxHII4x", 1, len(messages), 1, len(body)) + body


def _float_type(size):
    if size == 4:
        return struct.pack("<BBBBIHHBBBBI", 0x11, 0x20, 31, 0, 4, 0, 32, 23, 8, 0, 23, 127)
    return struct.pack("<BBBBIHHBBBBI", 0x11, 0x20, 63, 0, 8, 0, 64, 52, 11, 0, 52, 1023)


_INT32_TYPE = struct.pack("<BBBBIHH", 0x10, 0x08, 0, 0, 4, 0, 32)


def _dataspace(shape):
    return struct.pack("<BBBx4x", 1, len(shape), 0) + b"".join(struct.pack("<Q", s) for s in shape)


def _attribute_message(name, datatype, shape, data):
    name = name.encode() + b"\0"
    space = _dataspace(shape)
    return _message(0x0C, struct.pack("<BxHHH", 1, len(name), len(datatype), len(space)) + _pad8(name) + _pad8(datatype) + _pad8(space) + data)


def _text_attribute(name, text):
    data = text.encode() + b"\0"
    return _attribute_message(name, struct.pack("<BBBBI", 0x13, 0, 0, 0, len(data)), (), data)


def _chunk_btree(entries, ch, cw, base):
    """The version-1 B-tree (node type 1) over `entries` = [(bytes, address, row offset, column offset)] in chunk order, built level by
    level with sibling links, 2K entries per node; its nodes lie from address `base` on.  Returns (the nodes' bytes, the root's address)."""
    key = lambda nbytes, roff, coff, last=0: struct.pack("<IIQQQ", nbytes, 0, roff, coff, last)   # noqa: E731  (filter mask 0)
    per, node_bytes = 2 * _CHUNK_K, 24 + (2 * _CHUNK_K + 1) * 32 + 2 * _CHUNK_K * 8
    end_key = key(0, entries[-1][2] + ch, entries[-1][3] + cw, 4)     # one chunk past the last one in every dimension
    out, level, at = [], 0, base
    while True:
        groups = [entries[k:k + per] for k in range(0, len(entries), per)]
        address = [at + k * node_bytes for k in range(len(groups))]
        for k, group in enumerate(groups):
            left = address[k - 1] if k > 0 else _UNDEF
            right = address[k + 1] if k + 1 < len(groups) else _UNDEF
            node = b"TREE" + struct.pack("<BBHQQ", 1, level, len(group), left, right)
            node += b"".join(key(e[0], e[2], e[3]) + struct.pack("<Q", e[1]) for e in group)
            node += key(groups[k + 1][0][0], groups[k + 1][0][2], groups[k + 1][0][3]) if k + 1 < len(groups) else end_key
            out.append(node + b"\0" * (node_bytes - len(node)))
        at += len(groups) * node_bytes
        if len(groups) == 1:
            return b"".join(out), address[0]
        entries = [(g[0][0], a, g[0][2], g[0][3]) for g, a in zip(groups, address)]    # a child's first key, and the child
        level += 1


def _write_container(path, window_bound, H, W, variable, ch, cw, shuffle, deflate, y_ascending, streams):
    """The file around the chunk `streams` (an iterable of bytes-like objects in row-major chunk order, consumed one at a time)."""
    g = GridGeometry.from_bounds(window_bound, H, W)
    minx, miny, maxx, maxy = (float(v) for v in window_bound)
    x = g.x0 + np.arange(W, dtype=np.float64) * g.dx
    y = g.y0 + np.arange(H, dtype=np.float64) * g.dy
    if y_ascending:
        y = y[::-1]
    coords = {"x": (np.ascontiguousarray(x, dtype="<f8"), 0, (minx, maxx)), "y": (np.ascontiguousarray(y, dtype="<f8"), 1, (miny, maxy))}
    names = sorted(["x", "y", variable])
    # the local heap's data segment: the empty name at 0, then the names
    heap_data, name_at = b"\0" * 8, {}
    for n in names:
        name_at[n] = len(heap_data)
        heap_data += _pad8(n.encode() + b"\0")
    f64, f32 = _float_type(8), _float_type(4)

    def coordinate_header(name, address):
        values, dimid, span = coords[name]
        return _object_header([
            _message(0x01, _dataspace((values.size,))),
            _message(0x03, f64, 1),
            _message(0x05, struct.pack("<BBBB", 2, 1, 2, 0), 1),                      # fill value: allocated early, never defined
            _message(0x08, struct.pack("<BBQQ", 3, 1, address, values.nbytes)),        # contiguous
            _text_attribute("CLASS", "DIMENSION_SCALE"),
            _text_attribute("NAME", name),
            _attribute_message("_Netcdf4Dimid", _INT32_TYPE, (), struct.pack("<i", dimid)),
            _attribute_message("actual_range", f64, (2,), struct.pack("<dd", *span)),
        ])

    def variable_header(btree):
        filters = []
        if shuffle:
            filters.append(struct.pack("<HHHH", 2, 8, 1, 1) + b"shuffle\0" + struct.pack("<II", 4, 0))
        if deflate:
            filters.append(struct.pack("<HHHH", 1, 8, 1, 1) + b"deflate\0" + struct.pack("<II", 1, 0))
        messages = [
            _message(0x01, _dataspace((H, W))),
            _message(0x03, f32, 1),
            _message(0x05, struct.pack("<BBBBII", 2, 3, 2, 1, 4, _FILL_BITS), 1),      # allocated incrementally, the fill value NaN
        ]
        if filters:
            messages.append(_message(0x0B, struct.pack("<BB6x", 1, len(filters)) + b"".join(filters), 1))
        messages += [
            _message(0x08, struct.pack("<BBBQIII", 3, 2, 3, btree, ch, cw, 4)),       # chunked: a version-1 B-tree
            _attribute_message("_FillValue", f32, (1,), struct.pack("<I", _FILL_BITS)),
            _attribute_message("_Netcdf4Coordinates", _INT32_TYPE, (2,), struct.pack("<ii", coords["y"][1], coords["x"][1])),
        ]
        return _object_header(messages)

    def root_header(btree, heap):
        return _object_header([
            _message(0x11, struct.pack("<QQ", btree, heap)),
            _text_attribute("Conventions", "CF-1.7"),
            _attribute_message("node_offset", _INT32_TYPE, (), struct.pack("<i", 1)),
        ])

    # addresses: superblock, root header, group B-tree, heap, symbol node, the three headers, the coordinates, the chunks, their B-tree
    root_at = 96
    btree_at = root_at + len(root_header(0, 0))
    heap_at = btree_at + 24 + (2 * _GROUP_INTERNAL_K + 1) * 8 + 2 * _GROUP_INTERNAL_K * 8
    heap_data_at = heap_at + 32
    snod_at = heap_data_at + len(heap_data)
    at = snod_at + 8 + 2 * _GROUP_LEAF_K * 40
    header_at = {}
    for n in names:
        header_at[n] = at
        at += len(variable_header(0)) if n == variable else len(coordinate_header(n, 0))
    data_at = {}
    for n in ("x", "y"):
        data_at[n] = at
        at += coords[n][0].nbytes
    chunks_at = at

    def head(btree, end):
        superblock = _SIGNATURE + struct.pack("<BBBBBBBxHHI", 0, 0, 0, 0, 0, 8, 8, _GROUP_LEAF_K, _GROUP_INTERNAL_K, 0)
        superblock += struct.pack("<QQQQ", 0, _UNDEF, end, _UNDEF)
        superblock += struct.pack("<QQI4xQQ", 0, root_at, 1, btree_at, heap_at)        # the root group's symbol table entry
        group = b"TREE" + struct.pack("<BBHQQ", 0, 0, 1, _UNDEF, _UNDEF) + struct.pack("<QQQ", 0, snod_at, name_at[names[-1]])
        group += b"\0" * (heap_at - btree_at - len(group))
        heap = b"HEAP" + struct.pack("<B3xQQQ", 0, len(heap_data), 1, heap_data_at)   # free-list head 1: no free block
        snod = b"SNOD" + struct.pack("<BxH", 1, len(names))
        snod += b"".join(struct.pack("<QQI4x16x", name_at[n], header_at[n], 0) for n in names)
        snod += b"\0" * (8 + 2 * _GROUP_LEAF_K * 40 - len(snod))
        headers = b"".join(variable_header(btree) if n == variable else coordinate_header(n, data_at[n]) for n in names)
        out = superblock + root_header(btree_at, heap_at) + group + heap + heap_data + snod + headers + coords["x"][0].tobytes() + coords["y"][0].tobytes()
        assert len(superblock) == 96 and len(out) == chunks_at
        return out

    nx = -(-W // cw)
    entries = []
    with open(path, "wb") as f:
        f.write(b"\0" * chunks_at)
        at = chunks_at
        for k, stream in enumerate(streams):
            pad = -at % 8
            f.write(b"\0" * pad)
            at += pad
            f.write(stream)
            entries.append((len(stream), at, (k // nx) * ch, (k % nx) * cw))
            at += len(stream)
        if len(entries) != -(-H // ch) * nx:
            raise _lib.DbmError(f"{path}: {len(entries)} chunk streams for {-(-H // ch) * nx} chunks")
        pad = -at % 8
        nodes, root = _chunk_btree(entries, ch, cw, at + pad)
        f.write(b"\0" * pad + nodes)
        end = at + pad + len(nodes)
        f.seek(0)
        f.write(head(root, end))
    return path


def _write_arguments(who, window_bound, shape, dtype, variable, chunks, shuffle, compression):
    """The checks the two writers share (every refusal names its argument): (H, W, chunk_h, chunk_w, deflate)."""
    if np.dtype(dtype) != np.float32:
        raise ValueError(f"{who}: array holds {np.dtype(dtype).name}: only float32 planes are written")
    shape = tuple(shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[0] == 1)) or shape[-2] < 1 or shape[-1] < 1:
        raise ValueError(f"{who}: array must be (1, H, W) or (H, W) and not empty; got {shape}")
    H, W = int(shape[-2]), int(shape[-1])
    try:
        bound = [float(v) for v in window_bound]
    except (TypeError, ValueError):
        bound = []
    if len(bound) != 4 or not all(np.isfinite(bound)) or bound[2] <= bound[0] or bound[3] <= bound[1]:
        raise ValueError(f"{who}: window_bound {window_bound!r}: (minx, miny, maxx, maxy), finite, maxx > minx and maxy > miny")
    if not isinstance(variable, str) or not variable or variable in ("x", "y") or not variable.isascii() or "/" in variable:
        raise ValueError(f"{who}: variable {variable!r}: an ASCII name other than 'x' and 'y'")
    try:
        ch, cw = (int(c) for c in chunks)
        whole = (ch, cw) == tuple(chunks)
    except (TypeError, ValueError):
        ch = cw = 0
        whole = False
    if not whole or ch < 1 or cw < 1:
        raise ValueError(f"{who}: chunks {chunks!r}: two chunk sides of at least 1")
    ch, cw = min(ch, H), min(cw, W)
    if ch * cw * 4 >= 1 << 31:
        raise ValueError(f"{who}: chunks of {ch} x {cw} samples hold 2^31 bytes or more")
    text = compression.lower() if isinstance(compression, str) else None
    if text not in ("deflate", "none"):
        raise ValueError(f"{who}: unsupported compression {compression!r} (\"deflate\", \"none\")")
    if not isinstance(shuffle, (bool, np.bool_)):
        raise ValueError(f"{who}: shuffle {shuffle!r}: True or False")
    return H, W, ch, cw, text == "deflate"


def chunk_bytes_of(band, ch, cw, shuffle, y_ascending):
    """The NumPy statement of dbm_chunk_encode's stage (a): the (H, W) float32 `band` as (chunks, ch * cw * 4) uint8, row-major chunk
    order, the file's rows reversed for y_ascending, edge chunks zero padded, the 32-bit patterns little endian, shuffled per chunk."""
    bits = np.ascontiguousarray(band, dtype=np.float32).view(np.uint32)
    if y_ascending:
        bits = bits[::-1]
    H, W = bits.shape
    ny, nx = -(-H // ch), -(-W // cw)
    padded = np.zeros((ny * ch, nx * cw), dtype="<u4")
    padded[:H, :W] = bits
    raw = np.ascontiguousarray(padded.reshape(ny, ch, nx, cw).transpose(0, 2, 1, 3)).view(np.uint8).reshape(ny * nx, ch * cw, 4)
    if shuffle:
        raw = raw.transpose(0, 2, 1)
    return np.ascontiguousarray(raw).reshape(ny * nx, ch * cw * 4)


def save_grid_to_netcdf(path, window_bound, array, variable="z", chunks=(256, 256), shuffle=True, compression="deflate", y_ascending=False,
                        nthreads=None):
    """Writes the float32 (H, W) or (1, H, W) NumPy `array` as the netCDF-4 file `path` and returns the path: the host writer.  The
    variable `variable`(y, x) is chunked (`chunks`, clipped to the plane), shuffled and deflated as asked (compression "deflate" or
    "none"); x and y hold the pixel centres of `window_bound` = (minx, miny, maxx, maxy), the root attribute node_offset = 1 says pixel
    registration, _FillValue is NaN.  y_ascending: the file's rows run south to north (GMT's order); the readers return it north-up.
    NumPy cuts and shuffles, dbm_deflate_encode_blocks encodes on `nthreads` host threads.  `write_netcdf_resident` writes the same
    file, byte for byte, from a plane in HBM."""
    who = "save_grid_to_netcdf"
    if not isinstance(array, np.ndarray):
        raise ValueError(f"{who}: array must be a float32 NumPy array, not {type(array).__name__} (a DeviceArray is written by write_netcdf_resident)")
    H, W, ch, cw, deflate = _write_arguments(who, window_bound, array.shape, array.dtype, variable, chunks, shuffle, compression)
    raw = chunk_bytes_of(array.reshape(H, W), ch, cw, bool(shuffle), bool(y_ascending))
    streams = deflate_encode_blocks(raw, nthreads) if deflate else (r.tobytes() for r in raw)
    return _write_container(os.fspath(path), window_bound, H, W, variable, ch, cw, bool(shuffle), deflate, bool(y_ascending), streams)


def write_netcdf_resident(path, window_bound, array, variable="z", chunks=(256, 256), shuffle=True, compression="deflate", y_ascending=False,
                          workspace_limit=None):
    """The mirror of `read_netcdf_resident`: writes the netCDF-4 file `path` from a plane that lives in HBM and returns the path.
    Cutting the chunks, the row order, the shuffle and deflate (one wavefront per chunk) run on the GPU (dbm_chunk_encode); only the
    stored bytes cross PCIe.  The file is byte for byte the one `save_grid_to_netcdf` writes from the downloaded plane with the same
    arguments.  array: a float32 DeviceArray of shape (1, H, W) or (H, W), or a resident Raster.  workspace_limit: bytes
    of raw blocks plus their stream slots per batch (block_writes: default 1 GiB; one block always goes).  Anything else raises a
    ValueError that names the argument, before any device work."""
    who = "write_netcdf_resident"
    array = resident_plane_to_write(array, who, "save_grid_to_netcdf")
    H, W, ch, cw, deflate = _write_arguments(who, window_bound, array.shape, array.dtype, variable, chunks, shuffle, compression)
    workspace_limit = write_options(workspace_limit, who)
    ctx = array.ctx
    chunk_bytes = ch * cw * 4
    nchunks = -(-H // ch) * -(-W // cw)
    worst = deflate_slot(chunk_bytes) if deflate else chunk_bytes      # a chunk's bytes in the download, before rounding up to even
    groups = -(-ch * cw // 1024)                                       # workgroups per chunk of the cutting kernel
    per_batch = blocks_per_call(workspace_limit, chunk_bytes, worst if deflate else 0, groups, nchunks)

    def encode(first, n, out, sizes):
        ctx.call("dbm_chunk_encode", devptr(array), H, W, ch, cw, -1 if y_ascending else 1, 1 if shuffle else 0, 8 if deflate else 1,
                 first, n, devptr(out), out.size, devptr(sizes))

    return _write_container(os.fspath(path), window_bound, H, W, variable, ch, cw, bool(shuffle), deflate, bool(y_ascending),
                            encoded_batches(nchunks, per_batch, worst, encode))
