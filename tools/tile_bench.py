"""dbm_grid_tile and dbm_grid_filled_windows on the reference's training-set geometry, on synthetic resident rasters made from a seed.

4028 windows of 9 km (data_prep.py:745-751) are cut the way data_prep.py:757-771, 880-911 cut them: X and W3 at 1000 m from a
6667 x 6667 plane (padding 1000 m: 11 x 11), W1 at 100 m from a 45 020 x 55 020 plane (110 x 110; 9.9 GB, uploaded in row blocks),
W2 at 500 m from 450 m rasters of 12 445 x 12 445 (22 x 22, VX and VY through the window stride), Y sliced at 250 m from a 16 000 x
16 000 grid (36 x 36).  The filled-window search runs on a 10 000 x 10 000 grid (36 x 36 windows, step 3).  Per kernel: the time
between two device synchronisations over enough repetitions to fill a good fraction of a second (host clock), the bytes the
algorithm needs (from the shapes: every raster node a window touches once, every output once) over that time, and the time of the
NumPy restatement (tests/tile_restatement.py) of the same call on one CPU thread.  The first windows of each class are checked
against the restatement.  Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/tile_bench.py [--windows N] [--seconds S] [--no-cpu] [--no-w1]
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


def separable_plane(dbm, H, W, rng, block=1000):
    """a[r] + b[c] in float32, uploaded in row blocks (the host never holds the plane); returns (DeviceArray, value callable)."""
    from deepbedmap_amd import _lib

    a = np.cumsum(rng.normal(0, 5, H)).astype(np.float32)
    b = np.cumsum(rng.normal(0, 5, W)).astype(np.float32)
    dev = dbm.DeviceArray((H, W))
    for r0 in range(0, H, block):
        host = np.add.outer(a[r0:r0 + block], b)
        _lib.check(_lib.lib().dbm_memcpy_h2d(dev.ctx.handle, C.c_void_p(dev.ptr + 4 * r0 * W), host.ctypes.data_as(C.c_void_p), host.nbytes),
                   dev.ctx.handle)
    return dev, (lambda rr, cc: a[rr] + b[cc])


def centred(dbm, H, W, d):
    """north-up geometry of an (H, W) plane of spacing d centred on the pole"""
    return dbm.GridGeometry(-0.5 * W * d + d / 2, 0.5 * H * d - d / 2, d, -d)


def timed(ctx, call, seconds):
    call()
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    once = time.perf_counter() - t0
    reps = max(3, int(seconds / max(once, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps, reps


def tile_bytes(n, out_h, out_w, res, d):
    """every node a window touches read once + every output written once, float32"""
    nodes = (int(np.ceil((out_h - 1) * res / d)) + 2) * (int(np.ceil((out_w - 1) * res / d)) + 2)
    return 4 * n * (nodes + out_h * out_w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4028)
    ap.add_argument("--seconds", type=float, default=0.4, help="timed repetitions fill about this long per kernel")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-w1", action="store_true", help="skip the 9.9 GB plane")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib, tiling
    import tile_restatement as tl

    rng = np.random.default_rng(0)
    n = args.windows
    # windows of 9 km on the 250 m lattice, inside +-2 000 km (every raster covers them with their padding)
    left = -2_000_000.0 + 250.0 * rng.integers(0, 15_900, n)
    bottom = -2_000_000.0 + 250.0 * rng.integers(0, 15_900, n)
    windows = np.stack([left, bottom, left + 9000.0, bottom + 9000.0], axis=1)
    res = {"windows": n, "seconds_per_kernel": args.seconds}
    ctx = _lib.default_context()
    lib = _lib.lib()

    classes = [("X_W3_1000m", 6667, 6667, 1000.0, dict(padding=1000)),
               ("W2_500m_from_450m", 12_445, 12_445, 450.0, dict(padding=1000, resolution=500)),
               ("Y_250m_sliced", 16_000, 16_000, 250.0, dict(interpolate=False))]
    if not args.no_w1:
        classes.insert(1, ("W1_100m", 45_020, 55_020, 100.0, dict(padding=1000)))
    for name, H, W, d, kw in classes:
        t0 = time.perf_counter()
        dev, val = separable_plane(dbm, H, W, rng)
        geom = centred(dbm, H, W, d)
        raster = dbm.Raster(dev, geom)
        plan = tiling._plan(raster, windows, kw.get("padding", 0), kw.get("resolution"), None, kw.get("interpolate", True))
        out_h, out_w = plan[3], plan[4]
        channels = 2 if "W2" in name else 1
        out = dbm.DeviceArray((n, channels, out_h, out_w), ctx)
        entry = {"raster": [H, W], "spacing_m": d, "tile": [out_h, out_w], "setup_s": round(time.perf_counter() - t0, 1)}

        def call():
            tiling._cut(raster, plan, None, False, out.ptr, channels * out_h * out_w, want_counts=False)

        dt, reps = timed(ctx, call, args.seconds)
        nbytes = tile_bytes(n, out_h, out_w, plan[2], d)
        entry.update(ms_per_call=round(1e3 * dt, 4), repetitions=reps, algorithmic_MB=round(nbytes / 1e6, 2),
                     algorithmic_GB_per_s=round(nbytes / dt / 1e9, 1), outputs=n * out_h * out_w)
        m = min(n, 64)
        got = dbm.selective_tile(raster, windows[:m], **kw).get()
        want, _ = tl.tile(val, (H, W), tuple(geom.as_array()), windows[:m], **kw)
        tol = np.spacing(np.abs(want)).astype(np.float64) + 16 * 2.0 ** -53 * float(np.abs(want).max())
        entry[f"parity_first_{m}"] = bool(np.all(np.abs(got.astype(np.float64) - want) <= tol))
        if args.no_cpu:
            entry["cpu_restatement_s"] = "not measured"
        else:
            t0 = time.perf_counter()
            tl.tile(val, (H, W), tuple(geom.as_array()), windows, **kw)
            entry["cpu_restatement_s"] = round(time.perf_counter() - t0, 2)
        res[name] = entry
        del raster, dev, out

    # the filled-window search: 10 000 x 10 000 at 250 m with blobs of NaN
    H = W = 10_000
    host = rng.normal(0, 100, (H, W)).astype(np.float32)
    for _ in range(400):
        r0, c0 = rng.integers(0, H), rng.integers(0, W)
        host[r0:r0 + rng.integers(1, 400), c0:c0 + rng.integers(1, 400)] = np.nan
    dev = dbm.to_device(host)
    size, step = 36, 3
    ny, nx = (H - size) // step + 1, (W - size) // step + 1
    fdev = ctx.malloc(ny * nx)

    def search():
        _lib.check(lib.dbm_grid_filled_windows(ctx.handle, C.c_void_p(dev.ptr), H, W, size, step, 0, 0, C.c_void_p(fdev)), ctx.handle)

    dt, reps = timed(ctx, search, args.seconds)
    rows = (ny - 1) * step + size
    nbytes = 4 * rows * ((nx - 1) * step + size) + rows * nx * (1 + size // step) + ny * nx
    flags = np.empty((ny, nx), np.uint8)
    _lib.check(lib.dbm_memcpy_d2h(ctx.handle, flags.ctypes.data_as(C.c_void_p), C.c_void_p(fdev), flags.nbytes), ctx.handle)
    ctx.free(fdev)
    entry = {"raster": [H, W], "window": size, "step": step, "candidates": ny * nx, "filled": int(flags.sum()), "ms_per_call": round(1e3 * dt, 4),
             "repetitions": reps, "algorithmic_MB": round(nbytes / 1e6, 2), "algorithmic_GB_per_s": round(nbytes / dt / 1e9, 1)}
    if args.no_cpu:
        entry["cpu_restatement_s"] = "not measured"
        entry["parity"] = "not measured"
    else:
        t0 = time.perf_counter()
        want = tl.filled_windows(host, (0.0, 0.0, 250.0, -250.0), size, step)
        entry["cpu_restatement_s"] = round(time.perf_counter() - t0, 2)
        entry["parity"] = bool(np.array_equal(flags, want))
    res["filled_windows"] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
