"""dbm_text_count_lines and dbm_text_parse on a generated CReSIS-style CSV (the DC8 format: Y,X,TIME,THICK,ELEVATION,FRAME,SURFACE,BOTTOM,
QUALITY; X, Y, ELEVATION, BOTTOM used): `--mib` MiB of text (default 256) made of a 16 MiB block of distinct ~100-byte lines, repeated.
About one line in twenty holds an empty BOTTOM (dropped), one in two hundred a CRLF.

Timed, each with a host clock around calls that end in a device synchronise, after warm-up calls, over a window of at least
`--seconds`:
  - the structure pass alone (dbm_text_count_lines on resident text): GB/s of text;
  - the whole parse call on resident text (structure pass again, parse pass, flag scan, compaction, and the call's own scratch
    allocation): GB/s of text; the difference of the two is printed as the parse pass and what follows it;
  - the upload alone (dbm_memcpy_h2d of the bytes from pageable memory): GB/s -- the H2D rate of this run;
  - end to end: `read_text_table(bytes, download=False)`, upload included;
  - `pandas.read_csv(...).dropna()` on the same bytes and host, when pandas is importable, and whether the tables agree bit for bit.
No speed target exists for this workload.  Prints one JSON line; `--out FILE` writes it too.
Usage: python tools/ascii_bench.py [--mib N] [--seconds S] [--no-cpu]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = "Y,X,TIME,THICK,ELEVATION,FRAME,SURFACE,BOTTOM,QUALITY".split(",")
USE = ["X", "Y", "ELEVATION", "BOTTOM"]


def dc8_block(nbytes, rng):
    """about nbytes of distinct lines as the CReSIS CSVs print them"""
    lines, size, k = [], 0, 0
    while size < nbytes:
        lat, lon = rng.uniform(-88.0, -66.0), rng.uniform(-180.0, 180.0)
        thick, elev, surf = rng.uniform(200.0, 3500.0), rng.uniform(300.0, 10000.0), rng.uniform(100.0, 900.0)
        bottom = "" if k % 20 == 7 else "%.2f" % (surf + thick)
        line = "%.6f,%.6f,%.4f,%.2f,%.4f,%d,%.2f,%s,%d%s" % (lat, lon, 40000.0 + 0.05 * k, thick, elev, 2011100701001 + k // 3000, surf, bottom,
                                                             1 + k % 3, "\r\n" if k % 200 == 11 else "\n")
        lines.append(line)
        size += len(line)
        k += 1
    return "".join(lines).encode()


def timed(call, seconds, warmup=2):
    for _ in range(warmup):
        call()
    iters, elapsed = 0, 0.0
    t0 = time.perf_counter()
    while elapsed < seconds:
        call()
        iters += 1
        elapsed = time.perf_counter() - t0
    return elapsed / iters, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib

    block = dc8_block(min(16, args.mib) << 20, np.random.default_rng(0))
    data = ",".join(NAMES).encode() + b"\n" + block * max(1, (args.mib << 20) // len(block))
    buf = np.frombuffer(data, dtype=np.uint8)
    nbytes = buf.size
    lib, ctx = _lib.lib(), _lib.default_context()
    reader = dbm.TextReader(",", 1, NAMES, USE)
    mask = sum(1 << k for k, n in enumerate(NAMES) if n in USE)
    res = {"text_bytes": nbytes, "format": "20xx_Antarctica_DC8", "min_seconds_per_figure": args.seconds}

    text = ctx.malloc(nbytes + 16)

    def upload():
        _lib.check(lib.dbm_memcpy_h2d(ctx.handle, C.c_void_p(text), buf.ctypes.data_as(C.c_void_p), nbytes), ctx.handle)
        ctx.synchronize()

    s, iters = timed(upload, args.seconds, warmup=1)
    res["upload"] = {"ms": round(1e3 * s, 3), "calls_timed": iters, "GBps": round(nbytes / s / 1e9, 2)}

    counts = (C.c_int64 * 2)()

    def structure():
        _lib.check(lib.dbm_text_count_lines(ctx.handle, C.c_void_p(text), nbytes, ord(","), counts, _lib.DEVICE_PTRS), ctx.handle)

    s_structure, iters = timed(structure, args.seconds)
    res["structure_pass"] = {"ms": round(1e3 * s_structure, 3), "calls_timed": iters, "text_GBps": round(nbytes / s_structure / 1e9, 2)}
    cap = int(counts[1]) - reader.skip - 1
    table = ctx.malloc(32 * cap)
    result = (C.c_int64 * 4)()

    def parse():
        _lib.check(lib.dbm_text_parse(ctx.handle, C.c_void_p(text), nbytes, ord(","), reader.skip, len(NAMES), mask, None, 0, C.c_void_p(table),
                                      cap, None, 0, result, _lib.DEVICE_PTRS), ctx.handle)

    s_parse, iters = timed(parse, args.seconds)
    res["parse_call"] = {"ms": round(1e3 * s_parse, 3), "calls_timed": iters, "text_GBps": round(nbytes / s_parse / 1e9, 2)}
    rest = s_parse - s_structure
    res["parse_pass_and_compaction"] = {"ms": round(1e3 * rest, 3), "text_GBps": round(nbytes / rest / 1e9, 2)}
    res.update(lines=int(counts[0]), rows_kept=int(result[0]), rows_left_to_the_host=int(result[1]))
    ctx.free(table)
    ctx.free(text)

    def end_to_end():
        points, _ = dbm.read_text_table(buf, reader, download=False)
        ctx.synchronize()
        return points

    s, iters = timed(end_to_end, args.seconds, warmup=1)
    res["end_to_end_with_upload"] = {"ms": round(1e3 * s, 3), "calls_timed": iters, "text_GBps": round(nbytes / s / 1e9, 2)}

    if not args.no_cpu:
        try:
            import pandas as pd
        except ImportError:
            pd = None
        if pd is None:
            res["pandas"] = "not importable"
        else:
            t0 = time.perf_counter()
            df = pd.read_csv(io.BytesIO(data), sep=",", header=reader.skip, names=NAMES, usecols=USE).dropna()
            res["pandas_read_csv_dropna_s"] = round(time.perf_counter() - t0, 2)
            got, cols = dbm.read_text_table(buf, reader)
            want = df[cols].to_numpy(dtype=np.float64)
            res["table_equals_pandas_bit_for_bit"] = bool(want.shape == got.shape and np.array_equal(want.view(np.uint64), got.view(np.uint64)))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
