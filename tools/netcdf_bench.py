"""dbm_chunk_decode on a synthetic netCDF-4 variable, at the ABI level (no HDF5 writer needed): a `--size` x `--size` (default 4096)
float32 plane of DEM-like values cut into `--chunk` x `--chunk` (default 256) chunks, each byte-shuffled and deflated (zlib level 4, as
netCDF-4 files usually are) with NumPy and zlib.

Timed, alternating, each with a host clock around work that ends in a device synchronise, after one untimed round, `--repeats` times:
  - device: ONE dbm_chunk_decode call with compression 8 and shuffle 1 -- the compressed bytes are uploaded, inflated by one wavefront
    per chunk, un-shuffled, masked and placed on the GPU (what `read_netcdf_resident(inflate="device")` does per batch);
  - host: zlib.decompress on 16 threads, then dbm_chunk_decode with compression 1 and shuffle 1 on the inflated chunks (what
    `inflate="host"` does: the upload is 1 / ratio times larger, the kernel the same);
  - host_numpy: zlib on 16 threads, NumPy's un-shuffle and value rule (the restatement's path), and the upload of the finished plane
    (dbm_memcpy_h2d) -- a reader without this kernel.
Every path's plane is compared with the source bit for bit.  Medians, minima and maxima are reported; no speed-up is promised.
Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/netcdf_bench.py [--size N] [--chunk N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILL = np.float32(-9999.0)


def dem(size, rng):
    """Smooth terrain plus small-scale roughness, in metres, with a gap of fill values: what a bed elevation grid looks like."""
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / np.float32(size)
    z = 1500.0 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y) + 400.0 * np.sin(17.0 * x * y) + rng.normal(0.0, 3.0, (size, size))
    z = np.round(z.astype(np.float32), 1)
    z[size // 3:size // 3 + size // 10, size // 2:size // 2 + size // 8] = FILL
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    size, chunk = args.size, args.chunk
    assert size % chunk == 0

    from deepbedmap_amd import DeviceArray, _lib
    from deepbedmap_amd.resident import devptr

    plane = dem(size, np.random.default_rng(0))
    ny = size // chunk
    blocks = plane.reshape(ny, chunk, ny, chunk).transpose(0, 2, 1, 3).reshape(ny * ny, chunk * chunk)
    shuffled = [np.ascontiguousarray(b).view(np.uint8).reshape(-1, 4).T.tobytes() for b in blocks]
    streams = [zlib.compress(s, 4) for s in shuffled]
    sizes = np.array([len(s) for s in streams], dtype=np.int64)
    payload = np.frombuffer(b"".join(streams), dtype=np.uint8)
    table = np.zeros((ny * ny, 8), dtype=np.int64)
    table[:, 0], table[:, 1], table[:, 2] = np.cumsum(sizes) - sizes, sizes, chunk
    table[:, 3], table[:, 4] = (np.arange(ny * ny) // ny) * chunk, (np.arange(ny * ny) % ny) * chunk
    table[:, 5], table[:, 6] = np.arange(ny * ny), 1
    raw_bytes = chunk * chunk * 4
    host_table = table.copy()
    host_table[:, 0], host_table[:, 1] = np.arange(ny * ny) * raw_bytes, raw_bytes
    want = np.where(plane == FILL, np.float32(np.nan), plane)
    fill_bits = int(np.array([FILL]).view(np.uint32)[0])

    ctx = _lib.default_context()
    out = DeviceArray((size, size), ctx)
    pool = ThreadPoolExecutor(max_workers=16)

    def decode(buf, tab, compression):
        ctx.call("dbm_chunk_decode", devptr(buf), buf.size, devptr(tab), len(tab), compression, 1, 4, 0, chunk, chunk, 1, fill_bits, 0, 1.0, 0.0,
                 devptr(out), size, size)   # (the call synchronises the stream)

    def device():
        decode(payload, table, 8)

    def host():
        inflated = np.frombuffer(b"".join(pool.map(zlib.decompress, streams)), dtype=np.uint8)
        decode(inflated, host_table, 1)

    def host_numpy():
        done = np.empty((ny, ny, chunk, chunk), dtype=np.float32)
        for k, raw in enumerate(pool.map(zlib.decompress, streams)):
            v = np.frombuffer(raw, dtype=np.uint8).reshape(4, -1).T.copy().view(np.float32).reshape(chunk, chunk)
            done[k // ny, k % ny] = np.where(v == FILL, np.float32(np.nan), v)
        full = np.ascontiguousarray(done.transpose(0, 2, 1, 3).reshape(size, size))
        ctx.upload(out.ptr, full)
        ctx.synchronize()

    paths = {"device": device, "host": host, "host_numpy": host_numpy}
    times = {k: [] for k in paths}
    equal = {}
    for name, fn in paths.items():   # the untimed round: code objects loaded, every path checked against the source
        ctx.call("dbm_fill_f32", devptr(out), size * size, 0.0)
        fn()
        got = out.get()
        equal[name] = bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)].view(np.uint32),
                                                                                            want[~np.isnan(want)].view(np.uint32)))
    for _ in range(args.repeats):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    res = {"plane": [size, size], "chunk": [chunk, chunk], "chunks": ny * ny, "decoded_bytes": int(plane.nbytes),
           "compressed_bytes": int(payload.size), "ratio": round(plane.nbytes / payload.size, 2), "repeats": args.repeats,
           "equals_source_bit_for_bit": equal}
    for name, t in times.items():
        res[name] = {"median_ms": round(1e3 * statistics.median(t), 2), "min_ms": round(1e3 * min(t), 2), "max_ms": round(1e3 * max(t), 2),
                     "decoded_GBps_at_median": round(plane.nbytes / statistics.median(t) / 1e9, 2)}
    res["host_over_device"] = round(statistics.median(times["host"]) / statistics.median(times["device"]), 2)
    res["host_numpy_over_device"] = round(statistics.median(times["host_numpy"]) / statistics.median(times["device"]), 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
