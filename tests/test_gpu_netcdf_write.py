"""-m gpu: `write_netcdf_resident` (dbm_chunk_encode: chunk cutting, row order, HDF5's shuffle and deflate with the fixed Huffman code
by one wavefront per chunk on the device) against the host writer and independent decoders.  The stream is determined by
the rule, so the device's file must equal, byte for byte, the file `save_grid_to_netcdf` writes from the downloaded plane; zlib
(`read_netcdf`) and the device inflater (`read_netcdf_resident`) then return the plane's bits.  No comparison has a tolerance.

Shapes: 1 x 1 and 3 x 5 (chunks of 4 to 60 bytes: the encoder's start and end paths), 70 x 45 with chunks (16, 16) and (32, 16) (partial
chunks in both directions), 300 x 520 with the default 256 x 256 chunks (2 x 3 chunks of 256 KiB, padded right and below), 128 x 128 as
ONE chunk of 64 KiB (positions beyond the 32 KiB window, the 16-bit table entries wrap)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import netcdf_write_restatement as wr  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = wr.BOUND
bits = wr.bits
CASES = [((1, 1), (256, 256)), ((3, 5), (256, 256)), ((70, 45), (16, 16)), ((70, 45), (32, 16)), ((300, 520), (256, 256)),
         ((128, 128), (128, 128))]


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(scope="module")
def plane():
    return wr.noise_plane(300, 520)


def both_files(dbm, tmp_path, a, name="f", **kw):
    """(device-written file, host-written file from the downloaded plane) with the same arguments."""
    dev = dbm.to_device(a)
    got = dbm.write_netcdf_resident(str(tmp_path / (name + "_dev.nc")), wr.bound_of(a.shape), dev, **kw)
    assert got == str(tmp_path / (name + "_dev.nc"))
    kw.pop("workspace_limit", None)
    want = dbm.save_grid_to_netcdf(str(tmp_path / (name + "_host.nc")), wr.bound_of(a.shape), dev.get(), **kw)
    return got, want


def same_bytes(got, want):
    a, b = open(got, "rb").read(), open(want, "rb").read()
    if a != b:
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError(f"{got}: {len(a)} bytes, {want}: {len(b)} bytes, first difference at byte {first}")


@pytest.mark.parametrize("y_ascending", [False, True])
@pytest.mark.parametrize("compression", ["deflate", "none"])
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("shape,chunks", CASES)
def test_the_file_equals_the_host_writers(dbm, tmp_path, plane, shape, chunks, shuffle, compression, y_ascending):
    a = np.ascontiguousarray(plane[:shape[0], :shape[1]])
    got, want = both_files(dbm, tmp_path, a, chunks=chunks, shuffle=shuffle, compression=compression, y_ascending=y_ascending)
    same_bytes(got, want)
    var = dbm.open_netcdf(got)
    assert var.chunk_shape == (min(chunks[0], shape[0]), min(chunks[1], shape[1]))
    assert var.filters == (("shuffle",) if shuffle else ()) + (("deflate",) if compression == "deflate" else ())
    assert len(var._chunks) == -(-shape[0] // var.chunk_shape[0]) * -(-shape[1] // var.chunk_shape[1])


@pytest.mark.parametrize("name", sorted(wr.contents()))
@pytest.mark.parametrize("shuffle", [True, False])
def test_contents_that_reach_every_path(dbm, tmp_path, name, shuffle):
    """Noise, a constant and a half-constant plane, a ramp, NaN regions with a payload, +-inf and -0.0, and uniform random bits (which
    do not compress: the stream is longer than the chunk and uses the slot beyond the raw size)."""
    a = wr.contents()[name]
    got, want = both_files(dbm, tmp_path, a, shuffle=shuffle)
    same_bytes(got, want)
    var = dbm.open_netcdf(got)
    (offset, nbytes, mask), = var._chunks.values()
    assert mask == 0
    if name == "random bits":
        assert a.nbytes < nbytes <= a.nbytes + a.nbytes // 8 + 16
    if name == "constant":
        assert nbytes <= a.nbytes // 64
    back, _ = dbm.read_netcdf(got, mask_and_scale=False)
    assert np.array_equal(bits(back), bits(a))


@pytest.mark.parametrize("y_ascending", [False, True])
@pytest.mark.parametrize("shape,chunks", CASES)
def test_both_readers_return_the_planes_bits(dbm, tmp_path, plane, shape, chunks, y_ascending):
    a = np.ascontiguousarray(plane[:shape[0], :shape[1]])
    path = dbm.write_netcdf_resident(str(tmp_path / "d.nc"), wr.bound_of(shape), dbm.to_device(a[None]), chunks=chunks, y_ascending=y_ascending)
    host, info = dbm.read_netcdf(path, mask_and_scale=False)
    assert np.array_equal(bits(host), bits(a))
    assert info["geometry"] == dbm.GridGeometry.from_bounds(wr.bound_of(shape), *shape)
    assert info["flipped"] == (y_ascending and shape[0] > 1)
    dev, _ = dbm.read_netcdf_resident(path, mask_and_scale=False)
    assert np.array_equal(bits(dev.get()), bits(a))
    masked, _ = dbm.read_netcdf_resident(path)
    assert wr.same(masked.get(), a)


def test_batches_give_the_same_file(dbm, tmp_path, plane):
    a = np.ascontiguousarray(plane[:70, :45])
    dev = dbm.to_device(a)
    whole = dbm.write_netcdf_resident(str(tmp_path / "whole.nc"), BOUND, dev, chunks=(16, 16))
    chunk = 16 * 16 * 4
    for limit in (1, 4 * (chunk + chunk + chunk // 8 + 16)):     # one chunk per call; four per call: 15 chunks in 4 calls
        part = dbm.write_netcdf_resident(str(tmp_path / f"limit{limit}.nc"), BOUND, dev, chunks=(16, 16), workspace_limit=limit)
        same_bytes(part, whole)


def test_dbm_chunk_encode_refuses_before_any_launch(dbm):
    ctx = dbm._lib.default_context()
    dev = dbm.to_device(np.zeros((70, 45), dtype=np.float32))
    out = np.zeros(1 << 16, dtype=np.uint8)
    sizes = np.zeros(16, dtype=np.uintp)
    lib = dbm._lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def refused(plane=dev.ptr, H=70, W=45, ch=16, cw=16, step=1, shuffle=1, compression=8, first=0, n=2, o=p(out), cap=out.size, s=p(sizes)):
        rc = lib.dbm_chunk_encode(ctx.handle, C.c_void_p(plane), H, W, ch, cw, step, shuffle, compression, first, n, o, cap, s)
        return rc, lib.dbm_last_error(ctx.handle).decode()

    assert refused()[0] == 0
    for kw, text in [(dict(plane=None), "NULL plane"), (dict(H=0), "empty plane"), (dict(ch=0), "chunk sides"), (dict(cw=46), "chunk sides"),
                     (dict(ch=71), "chunk sides"), (dict(step=0), "row step"), (dict(step=2), "row step"), (dict(shuffle=2), "shuffle"),
                     (dict(compression=5), "compression"), (dict(first=-1), "chunk range"), (dict(first=14, n=2), "chunk range"),
                     (dict(o=None), "NULL output"), (dict(s=None), "NULL output"), (dict(cap=2 * (1024 + 128 + 16) - 1), "worst case"),
                     (dict(compression=1, cap=2047), "worst case")]:
        rc, message = refused(**kw)
        assert rc == 1 and text in message, (kw, rc, message)
    assert lib.dbm_chunk_encode(None, C.c_void_p(dev.ptr), 70, 45, 16, 16, 1, 1, 8, 0, 2, p(out), out.size, p(sizes)) == 1
    rc, message = refused(H=1 << 16, W=1 << 16, ch=1 << 15, cw=1 << 15)
    assert rc == 1    # (a plane of 2^32 samples; a chunk of 2^32 bytes)
    assert refused(n=0)[0] == 0


def test_xyz_to_grid_writes_its_outfile_from_the_device(dbm, tmp_path):
    """The 20-point cloud of tests/test_gpu_surface.py (the reference's xyz_to_grid doctest, data_prep.py:393-396)."""
    xyz = 600.0 * np.random.RandomState(seed=42).rand(60).reshape(20, 3)
    path = str(tmp_path / "surface.nc")
    got, geometry = dbm.xyz_to_grid(xyz, "0/750/0/750", spacing=250, outfile=path)
    plain, same_geometry = dbm.xyz_to_grid(xyz, "0/750/0/750", spacing=250)
    assert np.array_equal(bits(got), bits(plain)) and geometry == same_geometry
    back, info = dbm.read_netcdf(path, mask_and_scale=False)
    assert np.array_equal(bits(back), bits(got))
    assert info["geometry"] == geometry and info["flipped"] and info["variable"] == "z"
    resident, _ = dbm.xyz_to_grid(xyz, "0/750/0/750", spacing=250, download=False, outfile=str(tmp_path / "resident.nc"))
    assert np.array_equal(bits(resident.get()), bits(got))
    same_bytes(str(tmp_path / "resident.nc"), path)
