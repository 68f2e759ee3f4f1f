"""dbm_grid_track on the continent's canvas: 18 000 x 22 000 float32 (1.58 GB, resident), bicubic, points resident in HBM.

Times 10^7 points along synthetic ordered flight lines and 10^7 uniformly random points (device pointers, z_interpolated + the
error statistics; host clock around `iters` calls that end in a device synchronise), checks the first 10^5 of each against the
float64 NumPy restatement (tests/track_restatement.py), and times that restatement on the same 10^7 points (one CPU thread).
Prints one JSON line; `--out FILE` writes it too.  Usage: python tools/track_bench.py [--points N] [--iters K] [--no-cpu]
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


def ordered_tracks(n, H, W, rng, spacing=0.1):
    """Flight lines: straight segments of 5000 points at `spacing` pixels (25 m at 250 m pixels), random headings, ordered."""
    seg = 5000
    k = (n + seg - 1) // seg
    starts_t = rng.uniform(0.1 * W, 0.9 * W, k)
    starts_s = rng.uniform(0.1 * H, 0.9 * H, k)
    ang = rng.uniform(0, 2 * np.pi, k)
    step = np.arange(seg) * spacing
    t = (starts_t[:, None] + np.cos(ang)[:, None] * step[None, :]).ravel()[:n]
    s = (starts_s[:, None] + np.sin(ang)[:, None] * step[None, :]).ravel()[:n]
    return t, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib
    import track_restatement as tr

    H, W = 18_000, 22_000
    rng = np.random.default_rng(0)
    t0 = time.time()
    rows = np.cumsum(rng.normal(0, 5, H)).astype(np.float32)
    cols = np.cumsum(rng.normal(0, 5, W)).astype(np.float32)
    host = np.add.outer(rows, cols)
    host[:76] = np.nan   # the canvas's NaN frame (top rows)
    canvas = dbm.to_device(host)
    setup_s = time.time() - t0
    geom = dbm.GridGeometry.from_bounds((-2_700_000.0, -2_200_000.0, 2_800_000.0, 2_300_000.0), H, W)
    g = geom.as_array()
    ctx = canvas.ctx
    lib = _lib.lib()
    n = args.points
    res = {"canvas": [H, W], "points": n, "interpolation": "bicubic", "iters": args.iters, "setup_s": round(setup_s, 1)}
    for kind in ("ordered", "random"):
        if kind == "ordered":
            t, s = ordered_tracks(n, H, W, rng)
        else:
            t, s = rng.uniform(-0.5, W - 0.5, n), rng.uniform(-0.5, H - 0.5, n)
        pts = np.ascontiguousarray(np.stack([geom.x0 + t * geom.dx, geom.y0 + s * geom.dy, rng.normal(0, 10, n)], axis=1))
        dp = dbm.DevicePoints(pts, ctx)
        zdev, sdev = dp.outputs()

        def call(z=True):
            _lib.check(lib.dbm_grid_track(ctx.handle, C.c_void_p(canvas.ptr), H, W, g.ctypes.data_as(C.POINTER(C.c_double)),
                                          C.c_void_p(dp.ptr), n, 3, 2, 0.5, C.c_void_p(zdev) if z else None, C.c_void_p(sdev),
                                          _lib.DEVICE_PTRS), ctx.handle)

        for z in (True, False):
            for _ in range(3):
                call(z)
            ctx.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.iters):
                call(z)
            ctx.synchronize()
            res[f"{kind}_{'values_and_stats' if z else 'stats_only'}_ms"] = round(1e3 * (time.perf_counter() - t1) / args.iters, 4)
        # end to end through the Python layer (host copy of z_interpolated included)
        t1 = time.perf_counter()
        zi, st = dbm.grdtrack(dp, canvas, geom)
        res[f"{kind}_python_grdtrack_ms"] = round(1e3 * (time.perf_counter() - t1), 2)
        m = min(n, 100_000)
        want = tr.sample(host, (H, W), tuple(g), pts[:m, 0], pts[:m, 1], "bicubic")
        ok = np.array_equal(np.isnan(zi[:m]), np.isnan(want))
        f = ~np.isnan(want)
        ok = ok and bool(np.all(np.abs(zi[:m][f] - want[f]) <= 1e-9 * (1 + np.abs(want[f]))))
        res[f"{kind}_parity_first_{m}"] = bool(ok)
        res[f"{kind}_count"] = st.count
        res[f"{kind}_rmse"] = st.rmse
        if not args.no_cpu:
            t1 = time.perf_counter()
            zc = tr.sample_chunked(host, (H, W), tuple(g), pts[:, 0], pts[:, 1], "bicubic")
            res[f"{kind}_cpu_restatement_s"] = round(time.perf_counter() - t1, 2)
            sc = tr.stats(zc, pts[:, 2])
            res[f"{kind}_cpu_rmse_rel_diff"] = abs(sc["rmse"] - st.rmse) / sc["rmse"]
        del dp
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
