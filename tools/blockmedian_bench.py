"""dbm_points_polar_stereographic, dbm_points_region and dbm_points_blockmedian on a synthetic survey: ~2 x 10^7 points about 15 m apart
along criss-crossing flight lines (half along meridians, half along parallels) over ~750 km x 750 km around 77 S -- about 3000 blocks of
250 m on a side, 15-20 points per block and pass, twice that where lines cross.  Everything is resident in HBM (device pointers).

Each call is timed with a host clock around `iters` calls that end in a device synchronise, after warm-up calls, over a window of at
least `--seconds`; printed per call: ms, points/s, and the bytes the call must at least move (one read of the table plus one write of
its outputs) over the time, next to nothing else -- no speed target exists for this workload.  If pandas is importable the block table
is also computed with `DataFrame.groupby(block).median()` on the same rows (the only CPU comparison available here; assumed to run on one thread, as pandas' Cython group-by loops do) and
compared bit for bit.  Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/blockmedian_bench.py [--points N] [--seconds S] [--no-cpu]
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

INC = 250.0
LAT = (-80.4, -73.7)    # 6.7 degrees of latitude: ~750 km
LON = (-15.0, 15.0)     # 30 degrees of longitude at 77 S: ~750 km


def survey_lines(n, rng):
    """(n, 3) longitude, latitude (degrees), z: straight lines in longitude / latitude of 50 000 points each, alternately along a
    meridian (15 m steps) and along a parallel (11-19 m steps, by latitude), a few metres of cross-track jitter, z a smooth bed + noise"""
    seg = 50_000
    k = (n + seg - 1) // seg
    u = np.linspace(0.0, 1.0, seg)
    lon = np.empty((k, seg))
    lat = np.empty((k, seg))
    ns = np.arange(k) % 2 == 0
    at = rng.uniform(0.0, 1.0, k)
    lon[ns] = (LON[0] + at[ns] * (LON[1] - LON[0]))[:, None] + rng.normal(0, 1e-4, (int(ns.sum()), seg))
    lat[ns] = LAT[0] + u[None, :] * (LAT[1] - LAT[0])
    lat[~ns] = (LAT[0] + at[~ns] * (LAT[1] - LAT[0]))[:, None] + rng.normal(0, 2e-5, (int((~ns).sum()), seg))
    lon[~ns] = LON[0] + u[None, :] * (LON[1] - LON[0])
    lon, lat = lon.ravel()[:n], lat.ravel()[:n]
    z = 1500.0 * np.sin(lon * 0.7) * np.cos(lat * 1.3) - 500.0 + rng.normal(0, 20.0, n)
    return np.ascontiguousarray(np.stack([lon, lat, z], axis=1))


def timed(call, ctx, seconds, warmup=2):
    for _ in range(warmup):
        call()
    ctx.synchronize()
    iters, elapsed = 0, 0.0
    t0 = time.perf_counter()
    while elapsed < seconds:
        call()
        ctx.synchronize()
        iters += 1
        elapsed = time.perf_counter() - t0
    return 1e3 * elapsed / iters, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib, gridding
    import gridding_restatement as gr

    rng = np.random.default_rng(0)
    n = args.points
    lonlat = survey_lines(n, rng)
    lib, ctx = _lib.lib(), _lib.default_context()
    src = dbm.DevicePoints(lonlat, ctx)
    xyz = dbm.DevicePoints(lonlat, ctx)     # overwritten by the projection
    proj = np.array(gridding.EPSG3031, dtype=np.float64)
    res = {"points": n, "spacing": INC, "min_seconds_per_figure": args.seconds}

    def project():
        _lib.check(lib.dbm_points_polar_stereographic(ctx.handle, C.c_void_p(src.ptr), n, 3, proj.ctypes.data_as(C.POINTER(C.c_double)),
                                                      C.c_void_p(xyz.ptr), _lib.DEVICE_PTRS), ctx.handle)

    def report(name, ms, iters, nbytes):
        res[name] = {"ms": round(ms, 4), "calls_timed": iters, "points_per_s": round(n / (ms * 1e-3), 1), "min_bytes": int(nbytes),
                     "min_bytes_over_time_GBps": round(nbytes / (ms * 1e-3) / 1e9, 2)}

    ms, iters = timed(project, ctx, args.seconds)
    report("time_polar_stereographic", ms, iters, 2 * 24 * n)

    rdev = ctx.malloc(64)

    def region():
        _lib.check(lib.dbm_points_region(ctx.handle, C.c_void_p(xyz.ptr), n, 3, INC, C.c_void_p(rdev), C.c_void_p(rdev + 32), _lib.DEVICE_PTRS),
                   ctx.handle)

    ms, iters = timed(region, ctx, args.seconds)
    report("time_region", ms, iters, 24 * n + 40)
    r4, count = gridding.region_of(xyz, INC)
    H, W = gridding.block_shape(r4, INC)
    res.update(region=gridding.get_region(xyz, INC), finite_rows=count, blocks=[H, W])

    cap = min(n, H * W)
    tdev = ctx.malloc(24 * cap)
    grid = dbm.DeviceArray((H, W), ctx)
    cdev = ctx.malloc(4 * H * W)
    r4a = np.array(r4, dtype=np.float64)
    m = C.c_int64(0)

    def medians():
        _lib.check(lib.dbm_points_blockmedian(ctx.handle, C.c_void_p(xyz.ptr), n, r4a.ctypes.data_as(C.POINTER(C.c_double)), INC, C.c_void_p(tdev),
                                              cap, C.byref(m), C.c_void_p(grid.ptr), C.c_void_p(cdev), _lib.DEVICE_PTRS), ctx.handle)

    ms, iters = timed(medians, ctx, args.seconds)
    mm = int(m.value)
    report("time_blockmedian", ms, iters, 24 * n + 24 * mm + 8 * H * W)
    counts = np.empty((H, W), dtype=np.int32)
    _lib.check(lib.dbm_memcpy_d2h(ctx.handle, counts.ctypes.data_as(C.c_void_p), C.c_void_p(cdev), counts.nbytes), ctx.handle)
    filled = counts[counts > 0]
    bounds = (0,) + tuple(gridding.BLOCKMEDIAN_CLASS_BOUNDARIES) + (int(filled.max()) if filled.size else 0,)
    res.update(non_empty_blocks=mm, points_used=int(counts.sum()), median_population=float(np.median(filled)) if filled.size else 0.0,
               largest_population=int(filled.max()) if filled.size else 0,
               blocks_per_size_class=[int(((filled > lo) & (filled <= hi)).sum()) for lo, hi in zip(bounds[:-1], bounds[1:])])
    # end to end through the Python layer (table and raster downloaded)
    t1 = time.perf_counter()
    table = dbm.blockmedian(xyz, r4, INC)
    res["python_blockmedian_ms"] = round(1e3 * (time.perf_counter() - t1), 2)

    if not args.no_cpu:
        try:
            import pandas as pd
        except ImportError:
            pd = None
        if pd is None:
            res["pandas"] = "not importable"
        else:
            host = np.empty((n, 3))
            _lib.check(lib.dbm_memcpy_d2h(ctx.handle, host.ctypes.data_as(C.c_void_p), C.c_void_p(xyz.ptr), host.nbytes), ctx.handle)
            t1 = time.perf_counter()
            blk = gr.assign(host, r4, INC)
            res["cpu_assign_numpy_s"] = round(time.perf_counter() - t1, 2)
            df = pd.DataFrame({"block": blk, "x": host[:, 0], "y": host[:, 1], "z": host[:, 2]})
            df = df[df.block >= 0]
            t1 = time.perf_counter()
            want = df.groupby("block")[["x", "y", "z"]].median()
            res["cpu_pandas_groupby_median_s"] = round(time.perf_counter() - t1, 2)
            # not observed: pandas' groupby median is a single-threaded Cython loop (no BLAS, no OpenMP); an assumption about pandas
            res["cpu_threads_assumed_for_pandas"] = 1
            res["table_equals_pandas_bit_for_bit"] = bool(want.shape == table.shape and np.array_equal(
                want.to_numpy().view(np.uint64), table.view(np.uint64)))
    for p in (rdev, tdev, cdev):
        ctx.free(p)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
