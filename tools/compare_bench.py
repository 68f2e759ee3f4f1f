"""dbm_grid_rescale and dbm_grid_rolling_std at the reference's sizes (deepbedmap.py:323-356, paper_figures.py:847-931), grids resident
in HBM:

  cubic_x4      BEDMAP2's continent plane, 6667 x 6667, x4 with order 3 (`.astype(np.int32)`, anti_aliasing, clip) -> 26 668 x 26 668
  linear_down   a 45 000 x 55 000 plane (the 100 m synthetic grid's size), scale 1 / 2.5, order 1, anti_aliasing -> 18 000 x 22 000
  roughness     standard_deviation_2d, window 5, on an 18 000 x 22 000 canvas with predict_tiled's 76-pixel NaN frame

For each: the host clock between two device synchronisations around enough calls to fill `--seconds` (default 0.4 s, at least 3 calls),
after one warm-up call that also grows the workspace; the algorithmic bytes (input read once + output written once, float32) over that
time next to the chip's measured 6.29 TB/s copy rate; a parity check of a corner block against the float64 restatement
(tests/comparison_restatement.py); and the time of the same operation on ONE CPU thread (scipy.ndimage for the rescales, the restatement
for the roughness) on a `--cpu-edge` x `--cpu-edge` sub-plane, scaled to the full plane by area (marked `extrapolated`).
Prints one JSON line; `--out FILE` writes it too.  Usage: python tools/compare_bench.py [--seconds S] [--no-cpu] [--only NAME]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBS = 6.29


def timed(ctx, call, seconds):
    call()   # warm-up: grows the workspace, loads the code objects
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    one = time.perf_counter() - t0
    reps = max(3, int(math.ceil(seconds / max(one, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps, reps


def report(res, name, sec, reps, nbytes):
    res[name + "_ms"] = round(1e3 * sec, 4)
    res[name + "_calls_timed"] = reps
    res[name + "_algorithmic_GB"] = round(nbytes / 1e9, 3)
    res[name + "_TBs"] = round(nbytes / sec / 1e12, 4)
    res[name + "_fraction_of_copy_rate"] = round(nbytes / sec / 1e12 / COPY_TBS, 4)


def scipy_rescale(x, out_shape, order, as_int):
    from scipy import ndimage

    x = (x.astype(np.int32) if as_int else x).astype(np.float64)
    lo, hi = x.min(), x.max()
    sigma = [max(0.0, (x.shape[k] / out_shape[k] - 1) / 2) for k in range(2)]
    x = ndimage.gaussian_filter(x, sigma, mode="mirror")
    y = ndimage.zoom(x, (out_shape[0] / x.shape[0], out_shape[1] / x.shape[1]), order=order, mode="mirror", grid_mode=True)
    return np.clip(y, lo, hi).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--cpu-edge", type=int, default=2000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default=None, choices=["cubic_x4", "linear_down", "roughness"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    import comparison_restatement as cr
    from deepbedmap_amd import _lib

    ctx = dbm.default_context()
    lib = _lib.lib()

    def rescale_into(src, out, order):
        # the entry point itself, into an output allocated once (the Python layer allocates its result, and freeing it synchronises)
        _lib.check(lib.dbm_grid_rescale(ctx.handle, C.c_void_p(src.ptr), src.shape[0], src.shape[1], out.shape[0], out.shape[1], order, 1, 1, 1,
                                        C.c_void_p(out.ptr)), ctx.handle)

    rng = np.random.default_rng(0)
    res = {"seconds_per_measurement": args.seconds, "copy_rate_TBs": COPY_TBS, "cpu_threads": 1}

    def smooth(H, W):
        rows = np.cumsum(rng.normal(0, 5, H)).astype(np.float32)
        cols = np.cumsum(rng.normal(0, 5, W)).astype(np.float32)
        return np.add.outer(rows, cols)

    def cpu_time(fn, full_area, edge_area):
        if args.no_cpu:
            return {"cpu": "not measured"}
        t0 = time.perf_counter()
        fn()
        sec = time.perf_counter() - t0
        return {"cpu_subplane_s": round(sec, 3), "cpu_full_plane_s_extrapolated": round(sec * full_area / edge_area, 1)}

    if args.only in (None, "cubic_x4"):
        H = W = 6667
        host = smooth(H, W) + rng.normal(0, 30, (H, W)).astype(np.float32)
        src = dbm.to_device(host)
        out = dbm.DeviceArray((4 * H, 4 * W), ctx)
        sec, reps = timed(ctx, lambda: rescale_into(src, out, 3), args.seconds)
        del out
        report(res, "cubic_x4", sec, reps, 4 * H * W + 4 * 16 * H * W)
        got = dbm.rescale(src, 4, order=3, as_int=True).get()[-400:, -400:]
        crop = host[-300:, -300:]
        xi = host.astype(np.int32)
        want = np.clip(cr.rescale64(crop, 4, order=3, clip=False, as_int=True), xi.min(), xi.max()).astype(np.float32)[-400:, -400:]
        res["cubic_x4_corner_max_error"] = float(np.abs(got.astype(np.float64) - want).max())
        res["cubic_x4_corner_bound"] = 2.0 ** -23 * float(np.abs(host).max())
        e = args.cpu_edge
        for k, v in cpu_time(lambda: scipy_rescale(host[:e, :e], (4 * e, 4 * e), 3, True), H * W, e * e).items():
            res["cubic_x4_" + k] = v
        del src, got

    if args.only in (None, "linear_down"):
        H, W = 45_000, 55_000
        seed = dbm.to_device(smooth(H // 10, W // 10))
        src = dbm.rescale(seed, 10, order=1)          # the big plane is made on the device: 9.9 GB never cross the bus
        assert src.shape == (H, W)
        out = dbm.DeviceArray((18_000, 22_000), ctx)
        sec, reps = timed(ctx, lambda: rescale_into(src, out, 1), args.seconds)
        del out
        report(res, "linear_down", sec, reps, 4 * H * W + 4 * 18_000 * 22_000)
        e = args.cpu_edge
        sub = smooth(e, e)
        for k, v in cpu_time(lambda: scipy_rescale(sub, cr.output_shape((e, e), 1 / 2.5), 1, True), H * W, e * e).items():
            res["linear_down_" + k] = v
        small = sub[:1000, :1200]
        got = dbm.rescale(small, 1 / 2.5, order=1, as_int=True).get()
        res["linear_down_small_plane_max_error"] = float(np.abs(got.astype(np.float64) - cr.rescale(small, 1 / 2.5, 1, as_int=True)).max())
        res["linear_down_small_plane_bound"] = 2.0 ** -23 * float(np.abs(small).max())
        del src, seed

    if args.only in (None, "roughness"):
        H, W = 18_000, 22_000
        host = smooth(H, W)
        host[:76] = host[-76:] = np.nan
        host[:, :76] = host[:, -76:] = np.nan
        canvas = dbm.to_device(host)
        out = dbm.DeviceArray((H, W), ctx)
        sec, reps = timed(ctx, lambda: _lib.check(lib.dbm_grid_rolling_std(ctx.handle, C.c_void_p(canvas.ptr), H, W, 5, C.c_void_p(out.ptr)),
                                                  ctx.handle), args.seconds)
        del out
        report(res, "roughness", sec, reps, 8 * H * W)
        got = dbm.standard_deviation_2d(canvas, 5).get()[:600, :600]
        want = cr.standard_deviation_2d(host[:602, :602], 5)[:600, :600]
        f = ~np.isnan(want)
        res["roughness_corner_nan_pattern_equal"] = bool(np.array_equal(np.isnan(got), np.isnan(want)))
        res["roughness_corner_max_error_ulps"] = float((np.abs(got[f].astype(np.float64) - want[f]) / np.spacing(np.abs(want[f]))).max())
        e = args.cpu_edge
        for k, v in cpu_time(lambda: cr.standard_deviation_2d(host[76:76 + e, 76:76 + e], 5), H * W, e * e).items():
            res["roughness_" + k] = v

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
