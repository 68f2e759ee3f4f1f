"""Host tests (no GPU) of the netCDF writers: the three gaps the feature closes, every stream decoded by zlib against the
restatement's chunk bytes, the container read back through `open_netcdf` / `read_netcdf` bit for bit, the B-tree beyond one node and
beyond two levels, every refusal by name before any device work, the stream conditions of the host encoder and the C declarations."""
import ctypes as C
import inspect
import os
import re
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import netcdf_write_restatement as wr  # noqa: E402

import deepbedmap_amd as dbm  # noqa: E402
from deepbedmap_amd import netcdf  # noqa: E402

bits = wr.bits


# ---- the three gaps ----
def test_save_array_to_grid_writes_the_netcdf_file_beside_an_unchanged_tif(tmp_path):
    a = wr.noise_plane(70, 45)
    plain = dbm.save_array_to_grid(str(tmp_path / "plain"), wr.BOUND, a[None], compression="lzw", tiled=True)
    both = dbm.save_array_to_grid(str(tmp_path / "x"), wr.BOUND, a[None], save_netcdf=True, compression="lzw", tiled=True)
    assert both == str(tmp_path / "x.tif")
    assert open(both, "rb").read() == open(plain, "rb").read()
    assert not os.path.exists(str(tmp_path / "plain.nc"))
    back, info = dbm.read_netcdf(str(tmp_path / "x.nc"), mask_and_scale=False)
    assert np.array_equal(bits(back), bits(a)) and info["variable"] == "z" and info["filters"] == ("shuffle", "deflate")
    assert info["geometry"] == dbm.GridGeometry.from_bounds(wr.BOUND, 70, 45)
    for dtype in (np.int16, np.float64):
        with pytest.raises(ValueError, match="save_array_to_grid: dtype"):
            dbm.save_array_to_grid(str(tmp_path / "i"), wr.BOUND, a[None], save_netcdf=True, dtype=dtype)
    assert not os.path.exists(str(tmp_path / "i.nc"))


def test_write_netcdf_resident_exists_and_xyz_to_grid_takes_outfile():
    assert callable(dbm.write_netcdf_resident) and callable(dbm.save_grid_to_netcdf)
    parameters = list(inspect.signature(dbm.xyz_to_grid).parameters)
    assert parameters[-1] == "outfile" and inspect.signature(dbm.xyz_to_grid).parameters["outfile"].default is None
    assert list(inspect.signature(dbm.write_netcdf_resident).parameters) == ["path", "window_bound", "array", "variable", "chunks", "shuffle",
                                                                            "compression", "y_ascending", "workspace_limit"]
    assert list(inspect.signature(dbm.save_grid_to_netcdf).parameters) == ["path", "window_bound", "array", "variable", "chunks", "shuffle",
                                                                          "compression", "y_ascending", "nthreads"]


# ---- independent decoding, geometry, the chunk index ----
def stored_chunks(var):
    f = var._f
    return {k: f.at(offset, nbytes, "a chunk") for k, (offset, nbytes, mask) in var._chunks.items() if mask == 0}


def check_file(path, a, chunks, shuffle, compression, y_ascending):
    H, W = a.shape
    ch, cw = min(chunks[0], H), min(chunks[1], W)
    var = dbm.open_netcdf(path)
    assert var.shape == (H, W) and var.dtype == np.dtype("<f4") and var.layout == "chunked" and var.chunk_shape == (ch, cw)
    assert var.filters == (("shuffle",) if shuffle else ()) + (("deflate",) if compression == "deflate" else ())
    assert np.isnan(var.fill) and np.isnan(var.storage_fill)
    assert var.geometry == dbm.GridGeometry.from_bounds(wr.bound_of(a.shape), H, W) and var.geometry.registration == "pixel"
    assert var.flipped == (y_ascending and H > 1)
    stored = stored_chunks(var)
    count = -(-H // ch) * -(-W // cw)
    assert sorted(stored) == list(range(count))
    for index, data in stored.items():
        want = wr.chunk_bytes(a, ch, cw, index, y_ascending)
        if shuffle:
            want = wr.shuffle(want, 4)
        if compression == "deflate":
            assert data[:2] == b"\x78\x01" and len(data) <= len(want) + len(want) // 8 + 16
            data = zlib.decompress(data)
        assert data == want, (index, path)
    back, info = dbm.read_netcdf(path, mask_and_scale=False)
    assert np.array_equal(bits(back), bits(a))
    masked, _ = dbm.read_netcdf(path)
    assert wr.same(masked, a)
    return var


@pytest.mark.parametrize("y_ascending", [False, True])
@pytest.mark.parametrize("compression", ["deflate", "none"])
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("chunks", [(16, 16), (32, 16)])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (70, 45)])
def test_every_chunk_decodes_and_the_file_reads_back(tmp_path, shape, chunks, shuffle, compression, y_ascending):
    a = wr.noise_plane(*shape)
    path = dbm.save_grid_to_netcdf(str(tmp_path / "f.nc"), wr.bound_of(shape), a, chunks=chunks, shuffle=shuffle, compression=compression,
                                   y_ascending=y_ascending)
    assert path == str(tmp_path / "f.nc")
    check_file(path, a, chunks, shuffle, compression, y_ascending)


def tree_levels(path):
    """(levels, nodes per level, entries of the widest node) of the chunk B-tree, read from the file's bytes; also checks the sibling links."""
    var = dbm.open_netcdf(path)
    f = var._f
    obj = netcdf._Object(f, netcdf._root_links(f, netcdf._Object(f, 96, 8, 8, "/"), 8, 8)[var.name], 8, 8, var.name)
    root = netcdf._u(obj.find(0x08)[0][1], 3, 8)
    level_nodes, frontier = [], [root]
    while frontier:
        level_nodes.append(frontier)
        children, levels = [], set()
        for k, addr in enumerate(frontier):
            node = f.addr(addr, 24, "a node")
            assert node[:4] == b"TREE" and node[4] == 1
            used = int.from_bytes(node[6:8], "little")
            assert 1 <= used <= 64
            left, right = int.from_bytes(node[8:16], "little"), int.from_bytes(node[16:24], "little")
            assert left == (frontier[k - 1] if k else netcdf._UNDEF) and right == (frontier[k + 1] if k + 1 < len(frontier) else netcdf._UNDEF)
            levels.add(node[5])
            body = f.addr(addr + 24, used * 40 + 32, "keys")
            if node[5] > 0:
                children += [int.from_bytes(body[j * 40 + 32:j * 40 + 40], "little") for j in range(used)]
        assert len(levels) == 1
        frontier = children
    return len(level_nodes), [len(n) for n in level_nodes]


def test_the_chunk_index_beyond_one_node_and_beyond_two_levels(tmp_path):
    a = wr.noise_plane(70, 45)
    path = dbm.save_grid_to_netcdf(str(tmp_path / "nodes.nc"), wr.bound_of(a.shape), a, chunks=(4, 4))
    var = check_file(path, a, (4, 4), True, "deflate", False)
    assert len(var._chunks) == 216
    assert tree_levels(path) == (2, [1, 4])
    b = wr.noise_plane(260, 260, seed=6)
    path = dbm.save_grid_to_netcdf(str(tmp_path / "levels.nc"), wr.bound_of(b.shape), b, chunks=(4, 4), compression="none", y_ascending=True)
    var = check_file(path, b, (4, 4), True, "none", True)
    assert len(var._chunks) == 4225
    assert tree_levels(path) == (3, [1, 2, 67])


def test_one_band_of_three_dimensions_and_a_named_variable(tmp_path):
    a = wr.noise_plane(70, 45)
    path = dbm.save_grid_to_netcdf(str(tmp_path / "bed.nc"), wr.BOUND, a[None], variable="bed", chunks=(256, 256))
    var = dbm.open_netcdf(path)
    assert var.name == "bed" and var.chunk_shape == (70, 45) and var.global_attrs["node_offset"] == 1
    assert var.attrs["_Netcdf4Coordinates"].tolist() == [1, 0]
    again = dbm.save_grid_to_netcdf(str(tmp_path / "again.nc"), wr.BOUND, a, variable="bed")
    assert open(again, "rb").read() == open(path, "rb").read()     # determined by its arguments: no time stamps


# ---- refusals ----
class FakeContext:
    """A context that fails the test if anything reaches the device."""

    def malloc(self, nbytes):
        return 4096

    def free(self, ptr):
        pass

    def call(self, name, *args):
        raise AssertionError(f"{name} was called: the refusal must come before any device work")


def test_refusals_name_the_argument_and_need_no_device(tmp_path):
    out = str(tmp_path / "r.nc")
    ctx = FakeContext()
    good = dbm.DeviceArray((1, 70, 45), ctx=ctx)
    write = dbm.write_netcdf_resident
    with pytest.raises(ValueError, match="write_netcdf_resident: array must be a float32 DeviceArray or a resident Raster, not ndarray"):
        write(out, wr.BOUND, np.zeros((70, 45), dtype=np.float32))
    host_raster = dbm.Raster(np.zeros((70, 45), dtype=np.float32), dbm.GridGeometry.from_bounds(wr.BOUND, 70, 45))
    with pytest.raises(ValueError, match="write_netcdf_resident: array: the Raster is not resident"):
        write(out, wr.BOUND, host_raster)
    with pytest.raises(ValueError, match="save_grid_to_netcdf: array must be a float32 NumPy array, not DeviceArray"):
        dbm.save_grid_to_netcdf(out, wr.BOUND, good)
    for who, call, make in (("write_netcdf_resident", write, lambda shape, dtype=np.float32: dbm.DeviceArray(shape, ctx=ctx, dtype=dtype)),
                            ("save_grid_to_netcdf", dbm.save_grid_to_netcdf, lambda shape, dtype=np.float32: np.zeros(shape, dtype=dtype))):
        for dtype in (np.float64, np.int32, np.uint8):
            with pytest.raises(ValueError, match=f"{who}: array holds {np.dtype(dtype).name}"):
                call(out, wr.BOUND, make((70, 45), dtype))
        for shape in ((2, 70, 45), (70,), (1, 1, 70, 45)):
            with pytest.raises(ValueError, match=rf"{who}: array must be \(1, H, W\) or \(H, W\)"):
                call(out, wr.BOUND, make(shape))
        ok = make((70, 45))
        for chunks in ((0, 16), (16, 0), (-1, 4), (16,), (16, 16, 16), 16, (2.5, 4), None):
            with pytest.raises(ValueError, match=f"{who}: chunks"):
                call(out, wr.BOUND, ok, chunks=chunks)
        for compression in ("lzw", "zstd", 8, None):
            with pytest.raises(ValueError, match=f"{who}: unsupported compression"):
                call(out, wr.BOUND, ok, compression=compression)
        for variable in ("x", "y", "", 3, "a/b"):
            with pytest.raises(ValueError, match=f"{who}: variable"):
                call(out, wr.BOUND, ok, variable=variable)
        for bound in ((0, 0, 0, 1), (0, 0, 1), (0, 0, np.nan, 1), None):
            with pytest.raises(ValueError, match=f"{who}: window_bound"):
                call(out, bound, ok)
        with pytest.raises(ValueError, match=f"{who}: shuffle"):
            call(out, wr.BOUND, ok, shuffle=2)
    for limit in (0, -5, "much"):
        with pytest.raises(ValueError, match="write_netcdf_resident: workspace_limit"):
            write(out, wr.BOUND, good, workspace_limit=limit)
    assert not os.path.exists(out)


# ---- the stream conditions of the host encoder ----
def encode(data, cap=None):
    lib = dbm._lib.lib()
    src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
    cap = len(data) + len(data) // 8 + 16 if cap is None else cap
    out = np.full(cap + 8, 0xAA, dtype=np.uint8)
    size = (C.c_size_t * 1)()
    rc = lib.dbm_deflate_encode_blocks(src.ctypes.data_as(C.c_void_p), len(data), 1, out.ctypes.data_as(C.c_void_p), cap, size, 1)
    assert (out[cap:] == 0xAA).all()
    return rc, out[:size[0]].tobytes()


def test_streams_stay_in_their_slot_and_decode():
    r = np.random.default_rng(11)
    for n in (0, 1, 2, 3, 63, 64, 65, 257, 258, 259, 4096, 32769):
        for data in (r.integers(0, 256, n, dtype=np.uint8).tobytes(), b"\x07" * n, (np.arange(n) % 251).astype(np.uint8).tobytes()):
            rc, stream = encode(data)
            assert rc == 0 and stream[:2] == b"\x78\x01" and len(stream) <= n + n // 8 + 16
            assert zlib.decompress(stream) == data
            assert encode(data, len(stream))[1] == stream
            rc, refused = encode(data, len(stream) - 1)     # one byte short: refused, nothing reported
            assert rc == 2 and refused == b""
    assert encode(b"")[1] == bytes.fromhex("7801030000000001")


def test_a_constant_chunk_is_all_long_matches():
    raw = np.full((256, 256), -2000.0, dtype=np.float32).tobytes()
    for data in (raw, wr.shuffle(raw, 4)):
        rc, stream = encode(data)
        assert rc == 0 and zlib.decompress(stream) == data
        assert len(stream) <= len(raw) // 64, len(stream)      # matches of 258 bytes at >= 13 bits: about raw / 158


def test_a_match_at_the_far_end_of_the_window_is_taken():
    half = np.random.default_rng(12).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    rc, stream = encode(half + half)
    assert rc == 0 and zlib.decompress(stream) == half + half
    assert len(stream) < 0.6 * 65536, len(stream)              # the second half costs little: distance 32 768 is in reach
    rc, stream = encode(half + b"\x55" + half)                  # distance 32 769 is not; the stream must still be right
    assert rc == 0 and zlib.decompress(stream) == half + b"\x55" + half
    assert len(stream) <= 65537 + 65537 // 8 + 16


def test_the_host_encoder_spreads_blocks_over_threads():
    blocks = np.random.default_rng(13).integers(0, 4, (9, 1000), dtype=np.uint8)
    one = netcdf.deflate_encode_blocks(blocks, nthreads=1)
    many = netcdf.deflate_encode_blocks(blocks, nthreads=4)
    assert one == many and [zlib.decompress(s) for s in one] == [b.tobytes() for b in blocks]


def test_the_cutting_statement_of_the_package_is_the_restatements():
    a = wr.noise_plane(70, 45)
    for ch, cw in ((16, 16), (32, 16), (70, 45)):
        for shuffle in (False, True):
            for asc in (False, True):
                got = netcdf.chunk_bytes_of(a, ch, cw, shuffle, asc)
                for index in range(len(got)):
                    want = wr.chunk_bytes(a, ch, cw, index, asc)
                    assert got[index].tobytes() == (wr.shuffle(want, 4) if shuffle else want)


# ---- declarations ----
def test_the_header_declares_both_entry_points_with_citations_and_status():
    text = open(os.path.join(ROOT, "include", "dbm.h")).read()
    assert re.search(r"int dbm_deflate_encode_blocks\(const void\* blocks, size_t block_bytes, int nblocks, void\* out, size_t out_stride,\s*size_t\* "
                     r"out_sizes,\s*int nthreads\);", text)
    i = text.index("int dbm_chunk_encode(")
    assert re.match(r"int dbm_chunk_encode\(dbm_ctx\* ctx, const float\* plane_dev, long H, long W, int chunk_h, int chunk_w, int row_step, int shuffle, "
                    r"int compression,\s*long first, int n_blocks, void\* out_host, size_t out_capacity, size_t\* sizes_host\);", text[i:])
    comment = text[text.rindex("/*", 0, i):i]
    for citation in ("data_prep.py:826-830", "data_prep.py:410-441", "deepbedmap.py:425-437"):
        assert citation in comment, citation
    assert "Status 12" in comment and "status 1, nothing launched" in comment
    assert "dbm_chunk_encode" in text[:text.index("#ifndef DBM_H")]      # the status list at the head
    from deepbedmap_amd import _lib

    assert len(_lib.SIGNATURES["dbm_chunk_encode"]) == 14 and len(_lib.SIGNATURES["dbm_deflate_encode_blocks"]) == 7
