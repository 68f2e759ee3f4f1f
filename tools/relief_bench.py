"""What rendering the DEM costs (DESIGN.md 6n quotes the numbers; there is no speed target): relief_image (dbm_grid_relief) shaded and
unshaded, write_png_resident (dbm_png_encode) of the full image and of its reduce=2 level against save_png on host threads and PIL's
Image.save (zlib level 6), and the file sizes at half and at double the default band_rows.

The canvas is the synthetic DEM of tools/geotiff_overviews_bench.py at `--shape` (default 18000 x 22000), its no-coverage region as
NaN, coloured by the reference's table stretched to +-4500.  Kernel calls are timed as `--calls` calls in a row between two device
synchronisations, writers as one call between two synchronisations with the file write included; medians of `--repeats`.  The JSON
result is rewritten to `--out` after every section, so that a run that is cut short leaves what it measured.
`--host-only` skips everything that needs a GPU (the image then comes from relief_image_host): a rehearsal of the host sections;
`--relief-only` stops after the kernels.
Usage: python tools/relief_bench.py [--shape H W] [--repeats R] [--calls N] [--threads T] [--no-pil-full] [--host-only] [--relief-only] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[18000, 22000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-pil-full", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--relief-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import deepbedmap_amd as dbm
    from deepbedmap_amd import relief
    from geotiff_overviews_bench import synthetic_dem

    H, W = args.shape
    res = {"shape": [H, W], "channels": 4, "filter": 1, "host_threads": args.threads}

    def note():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    cpt = dbm.make_cpt(dbm.read_cpt(os.path.join(ROOT, "tests", "golden", "oleron.cpt")), (-4500, 4500))
    z = synthetic_dem(H, W, args.seed)
    z[z == np.float32(-9999.0)] = np.nan
    gpu = not args.host_only
    ctx = dbm.default_context() if gpu else None

    def sync():
        if gpu:
            ctx.synchronize()

    def timed(fn, repeats):
        fn()   # untimed: first launches, allocations, page cache
        runs = []
        for _ in range(repeats):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            runs.append(time.perf_counter() - t0)
        return runs

    if gpu:
        canvas = dbm.to_device(z, ctx)
        sin_a, cos_a, _ = relief.shading_parameters("+d")
        stats = relief.shade_stats(canvas, sin_a, cos_a)
        runs = timed(lambda: relief.shade_stats(canvas, sin_a, cos_a), args.repeats)
        res["shade_stats"] = {"n_mean_sigma": list(stats), "median_ms": round(1e3 * statistics.median(runs), 3)}
        moved = 8 * H * W   # 4 bytes in, 4 bytes out per pixel
        for name, kw in (("relief_unshaded", {}), ("relief_shaded", dict(shading="+d", stats=stats))):
            def calls():
                for _ in range(args.calls):
                    relief.relief_image(canvas, cpt, **kw)
            runs = [t / args.calls for t in timed(calls, args.repeats)]
            med = statistics.median(runs)
            res[name] = {"ms": [round(1e3 * t, 3) for t in runs], "median_ms": round(1e3 * med, 3), "bytes_moved_GB": round(moved / 1e9, 3),
                         "GB_per_s": round(moved / med / 1e9, 1), "share_of_6290_GB_per_s": round(moved / med / 6.29e12, 3)}
        note()
        if args.relief_only:
            print(note(), flush=True)
            return 0
        level2 = dbm.build_overviews(canvas, 2, np.float32, float("nan"))[-1]
        images = {"full": relief.relief_image(canvas, cpt, shading="+d", stats=stats),
                  "reduce2": relief.relief_image(level2, cpt, shading="+d")}
        del canvas
        host_images = {k: v.get() for k, v in images.items()}
    else:
        from deepbedmap_amd.geotiff import overview_pyramid

        host_images = {"full": relief.relief_image_host(z, cpt, shading="+d"),
                       "reduce2": relief.relief_image_host(overview_pyramid(z, 2, np.nan)[-1], cpt, shading="+d")}
    del z

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "a.png")
        for name in ("reduce2", "full"):
            h, w = host_images[name].shape[:2]
            rows = relief.default_band_rows(w, 4)
            entry = {"shape": [h, w], "raw_MB": round(host_images[name].nbytes / 1e6, 2), "band_rows": rows, "bands": -(-h // rows)}
            if gpu:
                runs = timed(lambda: dbm.write_png_resident(path, images[name]), args.repeats)
                entry["write_png_resident"] = {"s": [round(t, 4) for t in runs], "median_s": round(statistics.median(runs), 4),
                                               "file_MB": round(os.path.getsize(path) / 1e6, 2)}
                for label, r in (("half", max(1, rows // 2)), ("double", rows * 2)):
                    if r != rows:
                        dbm.write_png_resident(path, images[name], band_rows=r)
                        entry["band_rows_" + label] = {"band_rows": r, "file_MB": round(os.path.getsize(path) / 1e6, 2)}
                for f in (0, 2):
                    dbm.write_png_resident(path, images[name], filter=f)
                    entry[f"filter_{f}_file_MB"] = round(os.path.getsize(path) / 1e6, 2)
            res[name] = entry
            note()
            runs = timed(lambda: dbm.save_png(path, host_images[name], nthreads=args.threads), 1 if name == "full" else args.repeats)
            entry["save_png"] = {"s": [round(t, 4) for t in runs], "median_s": round(statistics.median(runs), 4),
                                 "file_MB": round(os.path.getsize(path) / 1e6, 2)}
            note()
        try:
            from PIL import Image
        except ImportError:
            Image = None
        for name in ("reduce2", "full"):
            if Image is None or (name == "full" and args.no_pil_full):
                continue
            t0 = time.perf_counter()
            Image.fromarray(host_images[name]).save(path, compress_level=6)
            res[name]["pil_level6"] = {"s": round(time.perf_counter() - t0, 3), "file_MB": round(os.path.getsize(path) / 1e6, 2)}
            note()
    print(note(), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
