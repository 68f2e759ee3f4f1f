"""dbm_grid_polygon_mask on a seeded synthetic coastline: a midpoint-displacement ring of ~10^6 vertices and ~2000 km radius (star-shaped
around the pole, so it never crosses itself) plus a few hundred island and hole rings -- the vertex count of the real grounding line is
not known here, 10^6 edges is an assumption -- against two grids: (a) 2000 x 2000 nodes at 250 m straddling the coast and (b) the
continent at 1 km, both with a buffer of 10 km.  The edge table is resident in HBM (one upload).

Per grid, after warm-up calls: ms per call over a window of at least `--seconds` (host clock around calls, each of which ends in a device
synchronise), nodes/s, the culled list sizes, the bin entries, and the edge-node tests the schedule performs at most, counted from the
lists (256 lanes per tile; early exits of near wavefronts and the parity shortcut are not subtracted).  The unbinned schedule
(workspace_limit = 1 byte) runs on the same inputs in the same run, calls alternated with the binned ones, and the two masks are compared
byte for byte; on the continent grid it tests every culled edge against every node, so `--no-unbinned-continent` leaves it out there.
No speed target exists for this workload.  Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/polygon_bench.py [--levels 17] [--seconds S] [--no-unbinned-continent] [--grids a,b]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS = 2.0e6
BUFFER = 10_000.0


def coastline(levels, rng):
    """(n, 2) vertices, n = 8 * 2^levels: the radius over the angle by midpoint displacement (periodic), 150 km at the first level, x 0.6 per level"""
    r = np.full(8, RADIUS) + rng.normal(0, 100e3, 8)
    amp = 150e3
    for _ in range(levels):
        mid = 0.5 * (r + np.roll(r, -1)) + rng.normal(0, amp, len(r))
        r = np.stack([r, mid], axis=1).ravel()
        amp *= 0.6
    th = 2 * np.pi * np.arange(len(r)) / len(r)
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=1), r


def small_rings(count, rng, rmin, rmax):
    rings = []
    for _ in range(count):
        th, rad = rng.uniform(0, 2 * np.pi), rng.uniform(rmin, rmax)
        cx, cy = rad * np.cos(th), rad * np.sin(th)
        k = int(rng.integers(12, 64))
        a = np.sort(rng.uniform(0, 2 * np.pi, k))
        s = rng.uniform(2e3, 20e3) * rng.uniform(0.6, 1.0, k)
        rings.append(np.stack([cx + s * np.cos(a), cy + s * np.sin(a)], axis=1))
    return rings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=17)     # 8 * 2^17 = 1 048 576 vertices
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--grids", default="a,b")
    ap.add_argument("--no-unbinned-continent", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib, polygons

    rng = np.random.default_rng(0)
    coast, radius = coastline(args.levels, rng)
    islands = small_rings(200, rng, 1.05 * radius.max(), 1.15 * radius.max())
    holes = small_rings(100, rng, 0.1 * radius.min(), 0.8 * radius.min())
    poly = dbm.Polygons.from_rings([coast] + islands + holes)
    ctx = _lib.default_context()
    t0 = time.perf_counter()
    poly.device(ctx)
    ctx.synchronize()
    res = {"edges": len(poly), "rings": poly.n_rings, "edges_assumed_not_measured": True, "buffer_m": BUFFER,
           "upload_ms": round(1e3 * (time.perf_counter() - t0), 2), "min_seconds_per_figure": args.seconds}

    k = len(coast) // 16     # a stretch of coast away from the axes
    cx, cy = coast[k]
    extent = 1.2 * radius.max()
    n_b = int(2 * extent // 1000.0) + 1
    grids = {"a": (dbm.GridGeometry(cx - 1000 * 250.0, cy + 1000 * 250.0, 250.0, -250.0), (2000, 2000)),
             "b": (dbm.GridGeometry(-extent, extent, 1000.0, -1000.0), (n_b, n_b))}

    for name in args.grids.split(","):
        geom, shape = grids[name]
        nodes = shape[0] * shape[1]
        tiles = ((shape[0] + polygons.TILE - 1) // polygons.TILE) * ((shape[1] + polygons.TILE - 1) // polygons.TILE)
        tiles_x = (shape[1] + polygons.TILE - 1) // polygons.TILE
        lanes = polygons.TILE ** 2
        unbinned_too = not (name == "b" and args.no_unbinned_continent)
        out = {}

        def call(limit, key):
            m = dbm.polygon_mask(geom, shape, poly, BUFFER, download=False, workspace_limit=limit, ctx=ctx)
            ctx.synchronize()
            out[key] = m
            return polygons.last_stats(ctx)

        modes = [(None, "binned")] + ([(1, "unbinned")] if unbinned_too else [])
        stats = {key: call(limit, key) for limit, key in modes}     # warm-up, both schedules
        spent = {key: 0.0 for _, key in modes}
        calls = {key: 0 for _, key in modes}
        while min(spent.values()) < args.seconds:
            for limit, key in modes:                                 # alternated; a schedule that has filled its window sits out
                if calls[key] and spent[key] >= args.seconds:
                    continue
                t1 = time.perf_counter()
                call(limit, key)
                spent[key] += time.perf_counter() - t1
                calls[key] += 1
        st = stats["binned"]
        assert st["schedule"] == 1, st
        row = {"shape": list(shape), "pixel_m": abs(geom.dx), "nodes": nodes, "tiles": tiles,
               "proximity_edges": st["proximity_edges"], "parity_edges": st["parity_edges"],
               "tile_bin_entries": st["tile_entries"], "band_bin_entries": st["band_entries"]}
        host = out["binned"].get()
        row["nodes_in_mask"] = int(host.sum())
        for _, key in modes:
            ms = 1e3 * spent[key] / calls[key]
            tests = (lanes * (st["tile_entries"] + tiles_x * st["band_entries"]) if key == "binned"
                     else lanes * tiles * (st["proximity_edges"] + st["parity_edges"]))
            row[key] = {"ms": round(ms, 3), "calls_timed": calls[key], "nodes_per_s": round(nodes / (ms * 1e-3), 1),
                        "edge_node_tests_at_most": int(tests), "tests_per_s_at_most": round(tests / (ms * 1e-3), 1)}
        if unbinned_too:
            assert stats["unbinned"]["schedule"] == 0, stats["unbinned"]
            row["unbinned_equals_binned_byte_for_byte"] = bool(np.array_equal(host, out["unbinned"].get()))
        else:
            row["unbinned"] = "not run"
        res["grid_" + name] = row
        out.clear()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
