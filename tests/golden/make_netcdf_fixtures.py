"""Regenerates tests/golden/netcdf/ (the tests never run this: they read the committed files).

    python tests/golden/make_netcdf_fixtures.py [--h5cc PATH] [--out DIR]

Needs a genuine HDF5 library with its high-level library (h5cc on PATH, or --h5cc): make_netcdf_fixtures.c is compiled with it and
run in the output directory, where it writes the .nc files, dumps what H5Dread returns for every variable (expected/NAME.VAR.bin, the
stored type in native little-endian form) and prints one JSON object per variable.  This script turns the dumps into
expected/NAME.VAR.npy and the objects into manifest.json.  The expected values therefore come from libhdf5, not from the package.
"""
import argparse
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h5cc", default=shutil.which("h5cc") or "h5cc")
    ap.add_argument("--out", default=os.path.join(HERE, "netcdf"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    os.makedirs(os.path.join(out, "expected"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "make_netcdf_fixtures")
        # (a packaged h5cc may name the compiler it was built with; HDF5_CC / HDF5_CLINKER make it use the system's)
        cc = dict(os.environ, HDF5_CC=os.environ.get("HDF5_CC", "cc"), HDF5_CLINKER=os.environ.get("HDF5_CLINKER", "cc"))
        subprocess.run([args.h5cc, "-shlib", "-O1", "-o", exe, os.path.join(HERE, "make_netcdf_fixtures.c"), "-lhdf5_hl", "-lm"], check=True, cwd=tmp, env=cc)
        libdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(args.h5cc))), "lib")
        env = dict(os.environ, LD_LIBRARY_PATH=libdir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
        text = subprocess.run([exe], check=True, cwd=out, env=env, stdout=subprocess.PIPE, text=True).stdout
    entries = json.loads(text)
    for e in entries:
        stem = os.path.join(out, "expected", "%s.%s" % (e["file"][:-3], e["variable"]))
        native = np.dtype(e["dtype"]).newbyteorder("<") if np.dtype(e["dtype"]).itemsize > 1 else np.dtype(e["dtype"])
        np.save(stem + ".npy", np.fromfile(stem + ".bin", dtype=native).reshape(e["shape"]))
        os.remove(stem + ".bin")
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump(entries, f, indent=1, sort_keys=True)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(d, n)) for d, _, names in os.walk(out) for n in names)
    print(f"{len(entries)} variables, {total} bytes in {out}")


if __name__ == "__main__":
    main()
