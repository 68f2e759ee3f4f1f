"""write_geotiff_resident (dbm_tiff_encode: cast, tile cutting, predictor and LZW encode by one wavefront per block on the device)
against save_array_to_grid on the same resident canvas (the cast on the device, the int16 plane downloaded, tiles cut with NumPy,
LZW on host threads).

The canvas is the synthetic DEM of tools/geotiff_bench.py (smooth terrain quantised to 1/8 m, a nodata region) as a resident float32
DeviceArray of `--sizes` x `--sizes` samples (default 4096 and 8192).  Both writers write it as int16, tiled, LZW, with predictor 1 and
2, into a temporary directory.  Each timing is taken between two device synchronisations with the file write included; the best of
`--repeats` (default 3) is reported after one untimed call.  Printed per case: seconds, blocks/s, raw GB/s (int16 bytes of the padded
blocks), the compression ratio, and whether the two files are byte-identical.  There is no speed target for this workload.  Prints one
JSON line per size; `--out PREFIX` writes PREFIX_<size>.json too.
Usage: python tools/geotiff_write_bench.py [--sizes N ...] [--repeats R] [--workspace-limit BYTES] [--out PREFIX]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geotiff_bench import synthetic_dem  # noqa: E402


def timed(ctx, repeats, write):
    write()   # untimed: first launches, allocations, page cache
    times = []
    for _ in range(repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        write()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workspace-limit", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib

    ctx = _lib.default_context()
    ok = True
    for size in args.sizes:
        canvas = dbm.to_device(synthetic_dem(size, args.seed)[None], ctx)
        bound = (0.0, 0.0, 100.0 * size, 100.0 * size)
        blocks = (-(-size // 256)) ** 2
        raw = blocks * 256 * 256 * 2
        res = {"size": [size, size], "dtype": "int16", "compression": "lzw", "tile": [256, 256], "blocks": blocks, "raw_MB": round(raw / 1e6, 2)}
        with tempfile.TemporaryDirectory() as tmp:
            for predictor in (1, 2):
                dev_path, host_path = os.path.join(tmp, f"dev{predictor}"), os.path.join(tmp, f"host{predictor}")
                kw = dict(dtype=np.int16, tiled=True, compression="lzw", predictor=predictor, nodataval=-9999)
                t_dev = timed(ctx, args.repeats, lambda: dbm.write_geotiff_resident(dev_path, bound, canvas, workspace_limit=args.workspace_limit, **kw))
                t_host = timed(ctx, args.repeats, lambda: dbm.save_array_to_grid(host_path, bound, canvas, **kw))
                same = open(dev_path + ".tif", "rb").read() == open(host_path + ".tif", "rb").read()
                ok = ok and same
                compressed = int(np.sum(dbm.open_geotiff(dev_path + ".tif").counts))
                case = {"compression_ratio": round(raw / compressed, 3), "file_MB": round(os.path.getsize(dev_path + ".tif") / 1e6, 2),
                        "files_identical": bool(same)}
                for name, times in (("resident", t_dev), ("host", t_host)):
                    best = min(times)
                    case[name] = {"s": [round(t, 4) for t in times], "best_s": round(best, 4), "blocks_per_s": round(blocks / best, 1),
                                  "raw_GB_per_s": round(raw / best / 1e9, 3)}
                case["resident_over_host"] = round(min(t_host) / min(t_dev), 2)   # > 1: the device writer is faster
                res[f"predictor_{predictor}"] = case
        res["continent_18000x22000"] = "not measured"
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(f"{args.out}_{size}.json", "w") as f:
                f.write(line + "\n")
        del canvas
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
