"""read_geotiff_resident (dbm_tiff_decode: LZW decode by one wavefront per block, conversion, placement) on a synthetic DEM, against
the host reader of the same file.

A tiled LZW float32 GeoTIFF of `--size` x `--size` samples (default 8192: 1024 blocks of 256 x 256) is written with the package's own
writer from a seed: smooth terrain (sums of long waves plus a little noise, quantised to 1/8 m so that LZW finds repeats, as it does
in REMA's tiles) with a nodata region (constant -9999: long strings).  `read_geotiff_resident` is timed between two device
synchronisations -- file reads, upload, decode and placement included, the file in the page cache after one untimed read --,
`read_geotiff` (the host path: one thread, one block after another) once on the same file, and the two results are compared bit for
bit.  There is no speed target for this workload.  Prints one JSON line; `--out FILE` writes it too.

`--compression deflate [--level L] [--predictor P]`: the same DEM as a tiled deflate file, written here (`zlib.compress` per tile under
predictor 1, 2 or 3, through the package's tags and container: the package's writers refuse deflate), read with `inflate="device"`
(tiff_inflate.hip: one wavefront per block) and with `inflate="host"` (zlib on host threads, the decoded blocks uploaded), `--repeats`
times each, both compared with the source bit for bit.  `--keep FILE` leaves the file there for another reader to be timed on.
Usage: python tools/geotiff_bench.py [--size N] [--repeats R] [--workspace-limit BYTES] [--no-host]
                                     [--compression lzw|deflate] [--level L] [--predictor P] [--keep FILE]
"""
import argparse
import json
import os
import sys
import shutil
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_dem(size, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    z = np.zeros((size, size), dtype=np.float32)
    for _ in range(6):
        kx, ky = rng.uniform(-0.01, 0.01, 2).astype(np.float32)
        z += np.float32(rng.uniform(50, 400)) * np.sin(kx * x + ky * y + np.float32(rng.uniform(0, 6.28)))
    z += rng.normal(0, 0.25, z.shape).astype(np.float32)
    z = np.round(z * 8) / 8 + 1500
    z[size // 8:size // 3, size // 2:] = -9999.0   # ocean / no coverage
    return z.astype(np.float32)


def write_deflate(path, dem, bound, level, predictor):
    """The DEM as 256 x 256 deflate tiles: what libtiff's predictors leave of each tile, one zlib stream per tile."""
    from deepbedmap_amd import geotiff

    H, W = dem.shape
    blocks, _, _ = geotiff._tiles_of(dem, geotiff.TILE, geotiff.TILE)
    n, th, tw = blocks.shape
    if predictor == 3:   # per row: byte plane k holds byte k of every sample, most significant first; then differences modulo 256
        planes = np.ascontiguousarray(blocks.astype(">f4")).view(np.uint8).reshape(n, th, tw, 4)
        rows = np.ascontiguousarray(planes.transpose(0, 1, 3, 2)).reshape(n, th, 4 * tw)
        raw = rows.copy()
        raw[..., 1:] = rows[..., 1:] - rows[..., :-1]
    elif predictor == 2:
        raw = geotiff._difference_blocks(blocks).view(np.uint8)
    else:
        raw = blocks.view(np.uint8)
    streams = [zlib.compress(r.tobytes(), level) for r in raw.reshape(n, -1)]
    tags = geotiff._image_tags(H, W, dem.dtype, 8, predictor, True, th, tw, bound, -9999, geotiff.EPSG_ANTARCTIC_POLAR_STEREOGRAPHIC, True)
    return geotiff._write_container(path, True, tags, streams)


def timed_reads(dbm, ctx, path, repeats, **kw):
    dev, _ = dbm.read_geotiff_resident(path, ctx=ctx, **kw)   # untimed: page cache, first launches
    times = []
    for _ in range(repeats):
        del dev
        ctx.synchronize()
        t0 = time.perf_counter()
        dev, _ = dbm.read_geotiff_resident(path, ctx=ctx, **kw)
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return dev, times


def deflate_main(args):
    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib

    size = args.size
    dem = synthetic_dem(size, args.seed)
    res = {"size": [size, size], "dtype": "float32", "compression": "deflate", "level": args.level, "predictor": args.predictor,
           "tile": [256, 256]}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        path = write_deflate(os.path.join(tmp, "dem.tif"), dem, (0.0, 0.0, 100.0 * size, 100.0 * size), args.level, args.predictor)
        res["write_s"] = round(time.perf_counter() - t0, 3)
        plan = dbm.open_geotiff(path).plan()
        compressed = int(plan.blocks[:, 1].sum())
        decoded = len(plan) * 256 * 256 * 4
        res.update(blocks=len(plan), file_MB=round(os.path.getsize(path) / 1e6, 2), compressed_ratio=round(decoded / compressed, 3))
        ctx = _lib.default_context()
        good = True
        for where in ("device", "host"):
            dev, times = timed_reads(dbm, ctx, path, args.repeats, workspace_limit=args.workspace_limit, inflate=where)
            best = min(times)
            res[where + "_s"] = [round(t, 4) for t in times]
            res[where + "_decoded_GB_per_s"] = round(decoded / best / 1e9, 3)
            res[where + "_equals_source"] = bool(np.array_equal(dev.get().view(np.uint32), dem.view(np.uint32)))
            good = good and res[where + "_equals_source"]
        res["host_over_device"] = round(min(res["host_s"]) / min(res["device_s"]), 2)
        if args.keep:
            shutil.copyfile(path, args.keep)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if good else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workspace-limit", type=int, default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host reader (and the comparison with it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compression", choices=["lzw", "deflate"], default="lzw")
    ap.add_argument("--level", type=int, default=6, help="zlib level of the deflate file")
    ap.add_argument("--predictor", type=int, choices=[1, 2, 3], default=1, help="TIFF Predictor of the deflate file")
    ap.add_argument("--keep", default=None, help="deflate: copy the file here before the temporary directory goes")
    args = ap.parse_args()
    if args.compression == "deflate":
        return deflate_main(args)

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib

    size = args.size
    dem = synthetic_dem(size, args.seed)
    res = {"size": [size, size], "dtype": "float32", "compression": "lzw", "tile": [256, 256]}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        path = dbm.save_array_to_grid(os.path.join(tmp, "dem"), (0.0, 0.0, 100.0 * size, 100.0 * size), dem[None], tiled=True, compression="lzw",
                                      nodataval=-9999)
        res["write_s"] = round(time.perf_counter() - t0, 3)
        gf = dbm.open_geotiff(path)
        plan = gf.plan()
        compressed = int(plan.blocks[:, 1].sum())
        decoded = len(plan) * 256 * 256 * 4
        res.update(blocks=len(plan), file_MB=round(os.path.getsize(path) / 1e6, 2), compressed_ratio=round(decoded / compressed, 3))
        ctx = _lib.default_context()
        dev, _ = dbm.read_geotiff_resident(path, workspace_limit=args.workspace_limit, ctx=ctx)   # untimed: page cache, first launches
        times = []
        for _ in range(args.repeats):
            del dev
            ctx.synchronize()
            t0 = time.perf_counter()
            dev, _ = dbm.read_geotiff_resident(path, workspace_limit=args.workspace_limit, ctx=ctx)
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        best = min(times)
        res.update(resident_s=[round(t, 4) for t in times], blocks_per_s=round(len(plan) / best, 1), decoded_GB_per_s=round(decoded / best / 1e9, 3))
        got = dev.get().view(np.uint32)
        res["equals_source"] = bool(np.array_equal(got, dem.view(np.uint32)))
        if args.no_host:
            res["host_s"] = "not measured"
        else:
            t0 = time.perf_counter()
            ref, _ = dbm.read_geotiff(path)
            res["host_s"] = round(time.perf_counter() - t0, 3)
            res["equals_host_reader"] = bool(np.array_equal(got, np.ascontiguousarray(ref[0]).view(np.uint32)))
            res["speedup_over_host"] = round(res["host_s"] / best, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["equals_source"] and res.get("equals_host_reader", True) else 1


if __name__ == "__main__":
    sys.exit(main())
