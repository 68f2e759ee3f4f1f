"""`deepbedmap_amd.block_writes` on the host (no GPU): what `write_geotiff_resident`, `write_netcdf_resident` and the PNG writers share
-- the batch loop over packed streams, the blocks-per-call rule, the workspace_limit check and the deflate slot -- each against a
statement written out by hand."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def bw():
    from deepbedmap_amd import block_writes

    return block_writes


SIZES = [7, 2, 3, 4, 1]   # odd and even; 7 = worst, odd: its slot is 8 bytes


def stream_of(block):
    return bytes(16 * (block + 1) + i for i in range(SIZES[block]))


class FakeEncode:
    """Packs the blocks first .. first + n - 1 as `pack_streams` does: at even offsets from 0, the sizes next to them; every other
    byte of the buffer is overwritten, so a stream of an earlier batch does not survive the call."""

    def __init__(self):
        self.calls, self.buffers = [], []

    def __call__(self, first, n, out, sizes, *extras):
        assert out.dtype == np.uint8 and sizes.dtype == np.uintp and all(e.dtype == np.uint32 for e in extras)
        self.calls.append((first, n, out.size))
        self.buffers.append((out, sizes) + extras)
        out[:] = 0xEE
        pos = 0
        for k in range(n):
            data = stream_of(first + k)
            assert pos % 2 == 0 and pos + len(data) <= out.size
            out[pos:pos + len(data)] = np.frombuffer(data, dtype=np.uint8)
            sizes[k] = len(data)
            for e, extra in enumerate(extras):
                extra[k] = 1000 * (e + 1) + first + k
            pos += len(data) + len(data) % 2


@pytest.mark.parametrize("per_batch, calls", [(2, [(0, 2, 16), (2, 2, 16), (4, 1, 16)]), (5, [(0, 5, 40)]),
                                              (1, [(k, 1, 8) for k in range(5)])])
def test_encoded_batches(bw, per_batch, calls):
    encode = FakeEncode()
    got = [bytes(s) for s in bw.encoded_batches(5, per_batch, 7, encode)]   # (copied before the next item is taken)
    assert got == [stream_of(b) for b in range(5)]
    assert encode.calls == calls
    assert all(a is b for held in encode.buffers[1:] for a, b in zip(held, encode.buffers[0]))   # one buffer for every batch

    encode = FakeEncode()
    items = bw.encoded_batches(5, per_batch, 7, encode, extras=(np.uint32, np.uint32))
    assert [(bytes(s), a, b) for s, a, b in items] == [(stream_of(b), 1000 + b, 2000 + b) for b in range(5)]
    assert encode.calls == calls and all(len(held) == 4 for held in encode.buffers)
    assert all(a is b for held in encode.buffers[1:] for a, b in zip(held, encode.buffers[0]))


def test_encoded_batches_yields_views_of_the_reused_buffer(bw):
    items = bw.encoded_batches(5, 2, 7, FakeEncode())
    first = next(items)
    assert isinstance(first, memoryview) and bytes(first) == stream_of(0)
    next(items)
    assert bytes(first) == stream_of(0)   # the same batch: still there
    next(items)                           # the next batch overwrites the buffer the view looks into
    assert bytes(first) == stream_of(2) + b"\xee" + stream_of(3)[:3]


def test_encoded_batches_without_blocks_makes_no_call(bw):
    encode = FakeEncode()
    assert list(bw.encoded_batches(0, 1, 7, encode)) == [] and list(bw.encoded_batches(0, 1, 7, encode, extras=(np.uint32,))) == []
    assert encode.calls == []


def test_blocks_per_call(bw):
    # a 512 x 512 float32 LZW tile: 1 048 576 raw bytes + the slot of 3/2 + 64 = 1 572 928; a row of the block per launch unit
    assert bw.blocks_per_call(1 << 30, 1048576, 1572928, 512, 1000) == 409
    assert bw.blocks_per_call(1, 1048576, 1572928, 512, 1000) == 1              # one block always goes through
    # a 16 x 16 chunk: 1024 raw bytes, deflated into a slot of 1024 + 128 + 16 = 1168; one workgroup cuts it
    assert bw.blocks_per_call(10000, 1024, 1168, 1, 20) == 4
    assert bw.blocks_per_call(10000, 1024, 0, 1, 20) == 9                       # not encoded: no slots
    # a PNG band of 100 rows x 301 bytes: 30 100 + 33 878, two workgroups filter it; the host writer: 256 MiB, no slots, one unit
    assert bw.blocks_per_call(1 << 20, 30100, 33878, 2, 50) == 16
    assert bw.blocks_per_call(256 << 20, 30100, 0, 1, 10000) == 8918
    assert bw.blocks_per_call(256 << 20, 30100, 0, 1, 50) == 50
    assert bw.blocks_per_call(1 << 60, 1, 0, 1 << 20, 5000) == 2047             # the launch's grid binds: (2^31 - 1) // 2^20
    assert bw.blocks_per_call(1 << 60, 1, 0, 1, 5000) == 5000                   # the number of blocks binds
    assert bw.blocks_per_call(1 << 30, 1024, 1168, 1, 3) == 3


def test_write_options(bw):
    from deepbedmap_amd import block_reads

    assert bw.write_options(None, "w") == bw.WORKSPACE_DEFAULT == 1 << 30 and bw.WORKSPACE_DEFAULT is block_reads.WORKSPACE_DEFAULT
    assert bw.write_options(7.9, "w") == 7 and bw.write_options(1, "w") == 1
    for bad in (0, -1):
        with pytest.raises(ValueError, match="^w: workspace_limit must be positive$"):
            bw.write_options(bad, "w")
    for bad in ("x", [], object()):
        with pytest.raises(ValueError, match="^w: workspace_limit .* is not a number of bytes$"):
            bw.write_options(bad, "w")


def test_deflate_slot_is_one_object(bw):
    from deepbedmap_amd import netcdf, relief

    assert netcdf.deflate_slot is bw.deflate_slot and relief.deflate_slot is bw.deflate_slot
    assert [bw.deflate_slot(n) for n in (0, 7, 8, 1024, 30100)] == [16, 23, 25, 1168, 33878]
