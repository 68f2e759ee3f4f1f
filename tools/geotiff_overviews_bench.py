"""What overviews cost: write_geotiff_resident of a resident canvas with overviews="auto" against overviews=0, and dbm_grid_overviews
(pyramid.hip) alone.  DESIGN.md 6j, "Overviews", quotes the numbers; there is no speed target.

The canvas is a synthetic DEM of `--shape` samples (default 18000 x 22000, the stitched continent): smooth terrain quantised to
1/8 m with a nodata region, as in tools/geotiff_bench.py.  It is written as int16, tiled, LZW, predictor 1.  Every write is timed
between two device synchronisations with the file write included; the two variants alternate, and the median of `--repeats` (default
5) is reported after one untimed call of each.  The halving alone is timed the same way around `--halvings` (default 20) calls in a row.
Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/geotiff_overviews_bench.py [--shape H W] [--repeats R] [--halvings N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_dem(H, W, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    y, x = np.arange(H, dtype=np.float32)[:, None], np.arange(W, dtype=np.float32)[None, :]
    z = rng.standard_normal((H, W), dtype=np.float32)
    z *= np.float32(0.25)
    for _ in range(6):
        kx, ky = rng.uniform(-0.01, 0.01, 2).astype(np.float32)
        z += np.float32(rng.uniform(50, 400)) * np.sin(kx * x + (ky * y + np.float32(rng.uniform(0, 6.28))))
    np.round(z * 8, out=z)
    z /= 8
    z += 1500
    z[H // 8:H // 3, W // 2:] = -9999.0   # ocean / no coverage
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[18000, 22000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--halvings", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib
    from deepbedmap_amd.resident import devptr

    ctx = _lib.default_context()
    H, W = args.shape
    canvas = dbm.to_device(synthetic_dem(H, W, args.seed), ctx)
    bound = (0.0, 0.0, 100.0 * W, 100.0 * H)
    shapes = dbm.overview_shapes(H, W, "auto")
    kw = dict(dtype=np.int16, tiled=True, compression="lzw", predictor=1, nodataval=-9999)
    res = {"shape": [H, W], "dtype": "int16", "compression": "lzw", "tile": [256, 256], "overviews": [list(s) for s in shapes]}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {0: os.path.join(tmp, "base"), "auto": os.path.join(tmp, "pyramid")}

        def write(overviews):
            ctx.synchronize()
            t0 = time.perf_counter()
            dbm.write_geotiff_resident(paths[overviews], bound, canvas, overviews=overviews, **kw)
            ctx.synchronize()
            return time.perf_counter() - t0

        write(0), write("auto")   # untimed: first launches, allocations, page cache
        times = {0: [], "auto": []}
        for _ in range(args.repeats):
            for overviews in (0, "auto"):
                times[overviews].append(write(overviews))
        for overviews, name in ((0, "write_overviews_0"), ("auto", "write_overviews_auto")):
            res[name] = {"s": [round(t, 4) for t in times[overviews]], "median_s": round(statistics.median(times[overviews]), 4),
                         "file_MB": round(os.path.getsize(paths[overviews] + ".tif") / 1e6, 2)}
        res["auto_over_0"] = round(res["write_overviews_auto"]["median_s"] / res["write_overviews_0"]["median_s"], 3)
        res["samples_auto_over_0"] = round(1 + sum(h * w for h, w in shapes) / (H * W), 4)

        # where the difference goes: every level written as a file of its own (the levels hold the int16 samples as floats: the cast
        # is the identity), medians as above
        levels = dbm.build_overviews(canvas, "auto", dtype=np.int16, nodataval=-9999)
        res["levels_alone"] = []
        for k, level in enumerate(levels, 1):
            path = os.path.join(tmp, f"level{k}")

            def write_level():
                ctx.synchronize()
                t0 = time.perf_counter()
                dbm.write_geotiff_resident(path, bound, level, **kw)
                ctx.synchronize()
                return time.perf_counter() - t0

            write_level()
            t = [write_level() for _ in range(args.repeats)]
            res["levels_alone"].append({"shape": list(level.shape), "blocks": -(-level.shape[0] // 256) * -(-level.shape[1] // 256),
                                        "median_s": round(statistics.median(t), 4), "file_MB": round(os.path.getsize(path + ".tif") / 1e6, 2)})
        del levels

    # the halving alone: `halvings` calls in a row between two synchronisations
    out = dbm.DeviceArray((sum(h * w for h, w in shapes),), ctx)
    nodata = C.c_double(-9999.0)

    def halve():
        ctx.call("dbm_grid_overviews", devptr(canvas), H, W, 1, C.byref(nodata), len(shapes), devptr(out))

    halve()
    runs = []
    for _ in range(args.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.halvings):
            halve()
        ctx.synchronize()
        runs.append((time.perf_counter() - t0) / args.halvings)
    moved = 4 * H * W + 4 * sum(h * w for h, w in shapes)   # the canvas read once, every level written once (re-reads of level 3 and 6 aside)
    med = statistics.median(runs)
    res["dbm_grid_overviews"] = {"levels": len(shapes), "s": [round(t, 6) for t in runs], "median_s": round(med, 6),
                                 "bytes_moved_GB": round(moved / 1e9, 3), "GB_per_s": round(moved / med / 1e9, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
