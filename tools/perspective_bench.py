"""What the perspective view costs (there is no speed target): `plot_3d_view` -- relief, perspective, PNG -- of a test-area
sized plane (1008 x 1408) and of level 2 of the continent's pyramid (the synthetic DEM of tools/geotiff_overviews_bench.py at `--shape`,
default 18000 x 22000, reduced twice: 4500 x 5500), and its parts: `relief_image`, `perspective_image` (dbm_grid_minmax, the block
prepass and the render), `write_png_resident`.

The no-coverage region of the DEM is NaN: holes of the surface.  The view is the reference's (azimuth 202.5, elevation 60, level -1400,
tenfold exaggeration at 250 m; the level's pixels are 1000 m), `--width` pixels wide (default 1600) with the grey facade.  Each part is
timed as one call between two device synchronisations, `plot_3d_view` with its file write included; medians of `--repeats` after one
untimed call.  The JSON result is rewritten to `--out` after every section.  `--host` also times `perspective_image_host` (the plain
walk on `--threads` host threads) on the small plane and requires its bytes to equal the device's.
Usage: python tools/perspective_bench.py [--shape H W] [--width N] [--repeats R] [--threads T] [--host] [--small-only] [--out FILE]
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
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import deepbedmap_amd as dbm
    from geotiff_overviews_bench import synthetic_dem

    res = {"width": args.width, "view": {"azimuth": 202.5, "elevation": 60.0, "level": -1400.0, "exaggeration": 10.0}}

    def note():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    cpt = dbm.make_cpt(dbm.read_cpt(os.path.join(ROOT, "tests", "golden", "oleron.cpt")), (-4500, 4500))
    ctx = dbm.default_context()

    def timed(fn):
        fn()   # untimed: first launches, allocations, page cache
        runs = []
        for _ in range(args.repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            runs.append(time.perf_counter() - t0)
        return {"ms": [round(1e3 * t, 3) for t in runs], "median_ms": round(1e3 * statistics.median(runs), 3)}

    def section(name, plane, pixel_size):
        H, W = plane.shape
        raster = dbm.Raster(plane, dbm.GridGeometry(0.0, 0.0, pixel_size, -pixel_size))
        view = dbm.View(pixel_size=pixel_size)
        entry = {"shape": [H, W], "pixel_size": pixel_size}
        res[name] = entry
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "view.png")
            entry["plot_3d_view"] = timed(lambda: dbm.plot_3d_view(raster, path, cpt, shading="+d", width=args.width))
            entry["file_MB"] = round(os.path.getsize(path) / 1e6, 2)
            note()
            drape = dbm.relief_image(plane, cpt, shading="+d")
            entry["relief_image"] = timed(lambda: dbm.relief_image(plane, cpt, shading="+d"))
            image, ids = dbm.perspective_image(plane, drape, view, width=args.width, facade=(128, 128, 128, 255), return_hits=True)
            ids = ids.get()
            entry["image"] = [int(image.shape[1]), int(image.shape[0])]
            entry["pixels"] = {"surface": int((ids >= 0).sum()), "wall": int((ids == -2).sum()), "none": int((ids == -1).sum())}
            entry["perspective_image"] = timed(lambda: dbm.perspective_image(plane, drape, view, width=args.width, facade=(128, 128, 128, 255)))
            entry["write_png_resident"] = timed(lambda: dbm.write_png_resident(path, image))
            note()
            if args.host and name == "test_area":
                z, d = plane.get(), drape.get()
                t0 = time.perf_counter()
                host = dbm.perspective_image_host(z, d, view, width=args.width, facade=(128, 128, 128, 255), nthreads=args.threads)
                entry["perspective_image_host"] = {"s": round(time.perf_counter() - t0, 3), "threads": args.threads,
                                                   "same_bytes": bool(np.array_equal(host, image.get()))}
                note()
                if not entry["perspective_image_host"]["same_bytes"]:
                    raise SystemExit("the host entry and the device disagree")

    z = synthetic_dem(1008, 1408, args.seed)
    z[z == np.float32(-9999.0)] = np.nan
    section("test_area", dbm.to_device(z, ctx), 250.0)
    if not args.small_only:
        H, W = args.shape
        z = synthetic_dem(H, W, args.seed)
        z[z == np.float32(-9999.0)] = np.nan
        canvas = dbm.to_device(z, ctx)
        del z
        level2 = dbm.build_overviews(canvas, 2, np.float32, float("nan"))[-1]
        del canvas
        section("continent_level2", level2, 1000.0)
    print(note(), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
