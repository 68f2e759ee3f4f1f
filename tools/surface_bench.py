"""From a point cloud to the pixel-registered 250 m raster on the synthetic survey of tools/blockmedian_bench.py (~2 x 10^7 points on
criss-crossing flight lines over ~750 km x 750 km, about 3092 x 3685 blocks): block medians, the tension surface
(dbm_grid_tension_surface), the distance mask (dbm_grid_distance_mask) and the gridline -> pixel resampling (dbm_grid_to_pixel), every
stage on resident data.

Each stage is timed with a host clock around calls that end in a device synchronise (the surface: one call after one warm-up call on a
small sub-grid, since a call runs for seconds; the others: after two warm-up calls, over at least `--seconds`).  For the surface the
tool prints the iterations, the time per iteration (the call's time over the iterations: set-up, the read-backs every 32 iterations and
the final pass included) and the bytes one iteration of the three kernels must move -- operator: p read, free-node mask read, Ap
written (17 bytes per node); update: x, r, p, Ap read, x, r written (48); direction: r, p read, p written (24) -- over that time.  No
speed target exists for this workload.  The only CPU comparison available is SciPy's sparse direct solve of the same problem on a
sub-grid small enough to factor (`--cpu-nodes` on a side, from the middle of the raster; 0 skips it), assumed to run on one thread.
Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/surface_bench.py [--points N] [--seconds S] [--tol T] [--max-iter K] [--cpu-nodes M]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BYTES_PER_NODE_AND_ITERATION = 17 + 48 + 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--tension", type=float, default=0.35)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--cpu-nodes", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    from blockmedian_bench import INC, survey_lines, timed
    from deepbedmap_amd import _lib, gridding

    rng = np.random.default_rng(0)
    n = args.points
    lib, ctx = _lib.lib(), _lib.default_context()
    xyz = dbm.reproject(dbm.DevicePoints(survey_lines(n, rng), ctx))
    r4, _ = gridding.region_of(xyz, INC)
    H, W = gridding.block_shape(r4, INC)
    res = {"points": n, "spacing": INC, "region": gridding.get_region(xyz, INC), "nodes": [H, W], "tension": args.tension, "tol": args.tol,
           "min_seconds_per_figure": args.seconds}

    t0 = time.perf_counter()
    medians, geometry = dbm.blockmedian_grid(xyz, r4, INC, download=False)
    ctx.synchronize()
    res["blockmedian_grid_ms"] = round(1e3 * (time.perf_counter() - t0), 3)

    sub = medians.get()[H // 2 - 32:H // 2 + 32, W // 2 - 32:W // 2 + 32]
    dbm.tension_surface(sub, tension=args.tension, tol=args.tol, max_iter=args.max_iter)   # warm-up: code objects, allocator
    surface = dbm.DeviceArray((H, W), ctx)
    info = np.zeros(4)
    t0 = time.perf_counter()
    rc = lib.dbm_grid_tension_surface(ctx.handle, C.c_void_p(medians.ptr), H, W, args.tension, args.tol, args.max_iter, C.c_void_p(surface.ptr),
                                      info.ctypes.data_as(C.POINTER(C.c_double)))
    ms = 1e3 * (time.perf_counter() - t0)
    if rc not in (0, 10):
        _lib.check(rc, ctx.handle)
    iters = int(info[0])
    per_iter = ms / max(iters, 1)
    nbytes = BYTES_PER_NODE_AND_ITERATION * H * W
    res["surface"] = {"status": rc, "ms": round(ms, 2), "iterations": iters, "relative_residual": float(info[1]), "constraints": int(info[2]),
                      "free": int(info[3]), "ms_per_iteration": round(per_iter, 4), "bytes_per_iteration": int(nbytes),
                      "bytes_per_iteration_over_time_GBps": round(nbytes / (per_iter * 1e-3) / 1e9, 1)}

    masked = dbm.DeviceArray((H, W), ctx)

    def mask():
        _lib.check(lib.dbm_memcpy2d_d2d(ctx.handle, C.c_void_p(masked.ptr), 4 * W, C.c_void_p(surface.ptr), 4 * W, 4 * W, H), ctx.handle)
        _lib.check(lib.dbm_grid_distance_mask(ctx.handle, C.c_void_p(medians.ptr), C.c_void_p(masked.ptr), H, W, 3), ctx.handle)

    def copy_only():
        _lib.check(lib.dbm_memcpy2d_d2d(ctx.handle, C.c_void_p(masked.ptr), 4 * W, C.c_void_p(surface.ptr), 4 * W, 4 * W, H), ctx.handle)

    ms_copy, _ = timed(copy_only, ctx, args.seconds)
    ms_mask, calls = timed(mask, ctx, args.seconds)
    res["distance_mask"] = {"ms": round(ms_mask - ms_copy, 4), "ms_with_the_copy_that_restores_its_input": round(ms_mask, 4), "calls_timed": calls,
                            "radius": 3}
    pixel = dbm.DeviceArray((H - 1, W - 1), ctx)

    def to_pixel():
        _lib.check(lib.dbm_grid_to_pixel(ctx.handle, C.c_void_p(masked.ptr), H, W, 0.5, C.c_void_p(pixel.ptr)), ctx.handle)

    ms_pix, calls = timed(to_pixel, ctx, args.seconds)
    res["to_pixel"] = {"ms": round(ms_pix, 4), "calls_timed": calls, "min_bytes_over_time_GBps": round(8 * H * W / (ms_pix * 1e-3) / 1e9, 1)}
    out = pixel.get()
    res["pixels_kept"] = int(np.isfinite(out).sum())
    res["pixels"] = int(out.size)

    m = args.cpu_nodes
    if m >= 3:
        try:
            import surface_restatement as sr
        except ImportError:
            sr = None
        if sr is None:
            res["scipy"] = "not importable"
        else:
            sub = medians.get()[H // 2 - m // 2:H // 2 - m // 2 + m, W // 2 - m // 2:W // 2 - m // 2 + m]
            t0 = time.perf_counter()
            got, sinfo = dbm.tension_surface(sub, tension=args.tension, tol=args.tol, max_iter=args.max_iter)
            gpu_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            want = sr.tension_surface(sub, args.tension)
            cpu_s = time.perf_counter() - t0
            # not observed: SuperLU's factorisation behind scipy.sparse.linalg.spsolve is single-threaded; an assumption about SciPy
            res["scipy_subgrid"] = {"nodes": [m, m], "constraints": sinfo["constraints"], "gpu_s_upload_and_download_included": round(gpu_s, 4),
                                    "gpu_iterations": sinfo["iterations"], "scipy_assemble_and_spsolve_s": round(cpu_s, 2),
                                    "cpu_threads_assumed_for_scipy": 1,
                                    "max_abs_difference_m": float(np.abs(got.astype(np.float64) - want).max())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
