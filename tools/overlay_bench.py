"""What drawing the maps' vector layers costs (DESIGN.md 6p quotes the numbers; there is no speed target): `draw_layers`
(dbm_image_overlay) of three layers on the continent at 250 m -- an 18000 x 22000 x 4 image, S = 4: 500 000 segments of width 1.5 along
a closed synthetic ring (the grounding line), 4028 boxes of 36 x 36 pixels (the training tiles), 2 000 000 discs of diameter 3 along
synthetic tracks (a season's survey points) -- against `relief_image` and `write_png_resident` of the same picture, and the binned
schedule against the unbinned one on a 4096 x 4096 crop across the ring, where the unbinned one finishes in seconds.

Every call is timed between two device synchronisations after one untimed call; medians of `--repeats`.  Tables are resident (a
Polygons, a DevicePoints), as the product has them.  The JSON result is rewritten to `--out` after every section.  `--layers-only`
draws the three layers on a blank image and stops: what tools/kernel_trace.sh traces for the time per stage (cull, bin, paint).
`--host-only` builds the primitives, checks their counts and stops (a rehearsal without a GPU).
Usage: python tools/overlay_bench.py [--shape H W] [--crop N] [--repeats R] [--seed S] [--layers-only] [--host-only] [--out FILE]
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

PX = 250.0


def primitives(H, W, seed, n_ring=500_000, n_boxes=4028, n_tracks=200, per_track=10_000):
    """(geometry tuple, ring segments, box bounds, track points) in map coordinates; pixel (r, c) has its centre at (x0 + c dx, y0 + r dy)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    geom = (-PX * (W // 2), PX * (H // 2), PX, -PX)
    radius = 0.39 * min(H, W)
    th = 2 * np.pi * np.arange(n_ring) / n_ring
    rad = radius * (1 + 0.15 * np.sin(5 * th) + 0.05 * np.sin(17 * th + 1.0))
    c, r = W / 2 + rad * np.cos(th), H / 2 + rad * np.sin(th)
    x, y = geom[0] + c * PX, geom[1] - r * PX
    ring = np.stack([x, y, np.roll(x, -1), np.roll(y, -1)], axis=1)
    a, d = rng.uniform(0, 2 * np.pi, n_boxes), radius * 0.8 * np.sqrt(rng.uniform(0, 1, n_boxes))
    bx, by = geom[0] + np.round(W / 2 + d * np.cos(a)) * PX, geom[1] - np.round(H / 2 + d * np.sin(a)) * PX
    boxes = np.stack([bx, by - 36 * PX, bx + 36 * PX, by], axis=1)
    t = np.linspace(0.0, 1.0, per_track)[None, :]
    p0, p1 = rng.uniform(0.05, 0.95, (2, n_tracks, 1)), rng.uniform(0.05, 0.95, (2, n_tracks, 1))
    wig = 40.0 * np.sin(2 * np.pi * rng.uniform(2, 9, (n_tracks, 1)) * t)
    tc, tr = (p0[0] + (p1[0] - p0[0]) * t) * W + wig, (p0[1] + (p1[1] - p0[1]) * t) * H - wig
    tracks = np.stack([geom[0] + tc.ravel() * PX, geom[1] - tr.ravel() * PX, np.zeros(tc.size)], axis=1)
    return geom, ring, boxes, tracks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[18000, 22000])
    ap.add_argument("--crop", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layers-only", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    import deepbedmap_amd as dbm
    from deepbedmap_amd import overlay, relief

    H, W = args.shape
    geom, ring, boxes, tracks = primitives(H, W, args.seed)
    res = {"shape": [H, W], "channels": 4, "samples": 4,
           "layers": {"ring": {"segments": len(ring), "width": 1.5}, "boxes": {"boxes": len(boxes), "segments": 4 * len(boxes), "width": 1.0},
                      "tracks": {"discs": len(tracks), "diameter": 3.0}}}

    def note():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    if args.host_only:
        print(note(), flush=True)
        return 0

    ctx = dbm.default_context()
    g = dbm.GridGeometry(*geom, registration="pixel")
    layers = {"ring": dbm.Layer.lines(dbm.Polygons(ring, n_rings=1), 1.5, (0, 0, 0)),
              "boxes": dbm.Layer.lines(dbm.Polygons(dbm.Layer.boxes(boxes, 1.0, (0, 0, 0)).primitives, n_rings=len(boxes)), 1.0, (238, 154, 0)),
              "tracks": dbm.Layer.points(dbm.DevicePoints(tracks, ctx), 3.0, (255, 165, 0, 200))}
    for layer in layers.values():
        if isinstance(layer.primitives, dbm.Polygons):
            layer.primitives.device(ctx)      # the upload is not what is timed

    def timed(fn, repeats):
        fn()   # untimed: first launches, allocations
        runs = []
        for _ in range(repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            runs.append(time.perf_counter() - t0)
        return runs

    def ms(runs):
        return {"ms": [round(1e3 * t, 3) for t in runs], "median_ms": round(1e3 * statistics.median(runs), 3)}

    def draw(image, geometry, names, limit=None):
        out = {}
        for name in names:
            entry = ms(timed(lambda: dbm.draw_layers(image, geometry, [layers[name]], samples=4, workspace_limit=limit), args.repeats))
            entry.update(overlay.last_stats(ctx))
            out[name] = entry
        entry = ms(timed(lambda: dbm.draw_layers(image, geometry, [layers[n] for n in names], samples=4, workspace_limit=limit), args.repeats))
        out["all"] = entry
        return out

    if args.layers_only:
        image = dbm.DeviceArray((H, W, 4), ctx, dtype=np.uint8)
        ctx.call("dbm_fill_f32", dbm.resident.devptr(image), H * W, 1.5)
        for _ in range(2):
            dbm.draw_layers(image, g, list(layers.values()), samples=4)
        ctx.synchronize()
        print(note(), flush=True)
        return 0

    # the crop: both schedules on the same pixels
    n = args.crop
    c0, r0 = W // 2 - n // 2, max(0, int(H / 2 - 0.39 * min(H, W)) - n // 2)
    crop_g = dbm.GridGeometry(geom[0] + c0 * PX, geom[1] - r0 * PX, PX, -PX, registration="pixel")
    crop = dbm.DeviceArray((n, n, 4), ctx, dtype=np.uint8)
    ctx.call("dbm_fill_f32", dbm.resident.devptr(crop), n * n, 1.5)
    def once(limit):
        """The three layers, one call each, onto the blank crop: (times and statistics, the bytes)."""
        ctx.call("dbm_fill_f32", dbm.resident.devptr(crop), n * n, 1.5)
        out = {}
        for name, layer in layers.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            dbm.draw_layers(crop, crop_g, [layer], samples=4, workspace_limit=limit)
            ctx.synchronize()
            out[name] = {"ms": round(1e3 * (time.perf_counter() - t0), 3)}
            out[name].update(overlay.last_stats(ctx))
        out["all"] = {"ms": round(sum(v["ms"] for v in out.values()), 3)}
        return out, crop.get()

    res["crop"] = {"shape": [n, n], "origin_pixel": [r0, c0], "binned": draw(crop, crop_g, list(layers))}
    note()
    res["crop"]["binned_once"], binned_bytes = once(None)
    res["crop"]["unbinned_once"], unbinned_bytes = once(1)
    res["crop"]["same_bytes"] = bool(np.array_equal(unbinned_bytes, binned_bytes))
    del crop, binned_bytes, unbinned_bytes
    note()

    # the continent: relief, layers, PNG of the same picture
    from geotiff_overviews_bench import synthetic_dem

    z = synthetic_dem(H, W, args.seed)
    z[z == np.float32(-9999.0)] = np.nan
    canvas = dbm.to_device(z, ctx)
    del z
    cpt = dbm.make_cpt(dbm.read_cpt(os.path.join(ROOT, "tests", "golden", "oleron.cpt")), (-4500, 4500))
    res["relief_unshaded"] = ms(timed(lambda: relief.relief_image(canvas, cpt), args.repeats))
    image = relief.relief_image(canvas, cpt)
    del canvas
    res["full"] = draw(image, g, list(layers))
    note()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "map.png")
        runs = timed(lambda: dbm.write_png_resident(path, image), args.repeats)
        res["write_png_resident"] = {"s": [round(t, 4) for t in runs], "median_s": round(statistics.median(runs), 4),
                                     "file_MB": round(os.path.getsize(path) / 1e6, 2)}
    print(note(), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
