"""The whole error table and the error histogram of one grid at ~10^6 survey points (deepbedmap.py:550-563, 575-608): on the device
(`describe_on_tracks(bins=25)`: dbm_grid_track, dbm_track_error_quantiles, dbm_track_error_histogram; z_interpolated stays in HBM)
against the only route there was before -- `grdtrack` with z_interpolated downloaded, then pandas' `describe()` and `np.histogram` on
the host.  Both routes are timed alternately on the same resident points and grid (host clock around calls that end with their results
on the host), their tables are compared, and the medians of `--repeats` rounds are printed as one JSON line; `--out FILE` writes it too.
Usage: python tools/track_dist_bench.py [--points N] [--repeats K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pandas as pd

    import deepbedmap_amd as dbm

    H = W = 3000
    n = args.points
    r = np.random.default_rng(0)
    grid = dbm.to_device(np.add.outer(np.cumsum(r.normal(0, 5, H)), np.cumsum(r.normal(0, 5, W))).astype(np.float32))
    geom = dbm.GridGeometry.from_bounds((0.0, 0.0, 250.0 * W, 250.0 * H), H, W)
    seg = 5000                                                        # flight lines: ordered segments at 25 m steps
    k = (n + seg - 1) // seg
    ang, step = r.uniform(0, 2 * np.pi, k), np.arange(seg) * 0.1
    t = (r.uniform(0.1 * W, 0.9 * W, k)[:, None] + np.cos(ang)[:, None] * step).ravel()[:n]
    s = (r.uniform(0.1 * H, 0.9 * H, k)[:, None] + np.sin(ang)[:, None] * step).ravel()[:n]
    pts = np.ascontiguousarray(np.stack([geom.x0 + t * geom.dx, geom.y0 + s * geom.dy, np.zeros(n)], axis=1))
    z, _ = dbm.grdtrack(pts, grid, geom)
    pts[:, 2] = z - r.normal(-20.0, 60.0, n)                          # errors of metres
    pts[r.random(n) < 0.01, 2] = np.nan
    dp = dbm.DevicePoints(pts, grid.ctx)

    def device():
        d = dbm.describe_on_tracks(dp, {"g": (grid, geom)}, bins=25)["g"]
        return d.as_dict(), d.histogram[0]

    def host():
        zi, _ = dbm.grdtrack(dp, grid, geom)                          # downloads n float64
        e = pd.Series(zi - pts[:, 2])
        return dict(e.describe()), np.histogram(e[np.isfinite(e)], bins=25)[0]

    times = {"device": [], "host": []}
    for i in range(args.repeats + 3):                                 # three warm-up rounds
        for name, fn in (("device", device), ("host", host)):
            grid.ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if i >= 3:
                times[name].append(dt)
            if name == "device":
                got = out
        for key in ("count", "min", "25%", "50%", "75%", "max"):
            assert got[0][key] == out[0][key], (key, got[0][key], out[0][key])
        assert np.array_equal(got[1], out[1])
    res = {"points": n, "grid": [H, W], "bins": 25, "repeats": args.repeats, "finite_errors": int(got[0]["count"]),
           "device_ms_median": round(1e3 * float(np.median(times["device"])), 3), "device_ms_min": round(1e3 * min(times["device"]), 3),
           "device_ms_max": round(1e3 * max(times["device"]), 3),
           "host_route_ms_median": round(1e3 * float(np.median(times["host"])), 3), "host_route_ms_min": round(1e3 * min(times["host"]), 3),
           "host_route_ms_max": round(1e3 * max(times["host"]), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
