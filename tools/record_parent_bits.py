#!/usr/bin/env python3
"""Record what a checkout's libdbm.so computes for the op-level cases of tests/exposed_kernel_cases.py (weight gradients of the trunk,
the data-gradient chain, the deformable backward's stored-list gather) into tests/golden/perf_parent_bits.npz, which
tests/test_gpu_exposed_kernels_bitwise.py compares a later library with.  Needs a GPU.

    python tools/record_parent_bits.py --checkout /path/to/parent_checkout     # built there: make -C deepbedmap_amd/csrc

--checkout: the tree whose deepbedmap_amd package (and library) runs the cases -- the PARENT of the commit under test, so that the
record never comes from the code it judges.  The cases themselves come from this tree.  Default: this tree (a later re-recording, after a
change that moves bits on purpose).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkout", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "perf_parent_bits.npz"))
    args = ap.parse_args()
    checkout = os.path.abspath(args.checkout)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, checkout)
    import exposed_kernel_cases as cases

    dbm = cases.load()
    assert os.path.abspath(dbm[0].__file__).startswith(checkout + os.sep), (dbm[0].__file__, checkout)
    print("library:", dbm[1].lib()._dbm_path, flush=True)
    rec = cases.record(dbm, progress=lambda what: print("recorded", what, flush=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"{len(rec)} arrays -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
