#!/usr/bin/env python3
"""One line per kernel of the given .hip sources: demangled name, instruction count, SHA-256 of the normalised instruction text, and the
register / LDS / scratch figures of its metadata.  Two such outputs (before / after) show whether a refactor left a kernel's device
code alone: the same hash and the same figures = the same instructions in the same order with the same registers.

    tools/kernel_isa.py deepbedmap_amd/csrc/deform_window.hip --flags "-mllvm -pragma-unroll-threshold=100000"
    tools/kernel_isa.py a.hip b.hip > after.txt;  (the same on the older tree) > before.txt;  tools/kernel_isa.py --diff before.txt after.txt

Normalisation: comments and directives dropped, white space squeezed, the digits of local labels dropped (`.LBB3_17` -> `.LBB`,
`.Lxw_nolds72` -> `.Lxw_nolds`: those counters run over the whole translation unit, so moving a kernel to another file renumbers them
and changes nothing else).  Nothing here looks for any particular instruction.  --flags: extra compiler flags (what the Makefile adds for
that source); the compile step is tools/hip_asm.py's, shared with scan_store_drains.py."""
import argparse
import hashlib
import os
import re
import shlex
import sys

from hip_asm import compile_to_asm, demangle

LABEL = re.compile(r"(\.L[A-Za-z_]*[A-Za-z])[0-9_]*")
META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels_of(asm):
    """{mangled name: ([normalised lines], {metadata field: value})} of the kernels in one assembly text."""
    lines = asm.splitlines()
    meta, cur = {}, None
    for l in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]:
        if l.startswith("  - "):
            cur = {}
            l = "    " + l[4:]
        m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    out = {}
    for name, fields in meta.items():
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
        body = []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = " ".join(l.split(";")[0].split())
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue
            body.append(LABEL.sub(r"\1", l))
        out[name] = (body, {k: fields.get(k, "?") for k in META})
    return out


def report(paths, flags):
    ok = True
    for path in paths:
        asm, err = compile_to_asm(path, flags)
        if asm is None:
            print(f"{os.path.basename(path)}: compile failed\n{err}", file=sys.stderr)
            ok = False
            continue
        ks = kernels_of(asm)
        for (name, (body, fields)), d in zip(ks.items(), demangle(ks)):
            n = sum(1 for l in body if not l.endswith(":"))
            h = hashlib.sha256("\n".join(body).encode()).hexdigest()
            print(f"{d} insts={n} sha256={h} " + " ".join(f"{k}={v}" for k, v in fields.items()))
    return ok


def diff(before, after):
    rows = [{l.split()[0]: l.split()[1:] for l in open(p) if l.strip()} for p in (before, after)]
    same = True
    for k in sorted(set(rows[0]) | set(rows[1])):
        a, b = rows[0].get(k), rows[1].get(k)
        verdict = "identical" if a == b else "missing" if a is None or b is None else "DIFFERENT"
        same &= a == b
        print(f"{verdict:10s} {k}" + ("" if a == b or a is None or b is None else "\n  " + " ".join(a) + "\n  " + " ".join(b)))
    return same


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*")
    ap.add_argument("--flags", default="", help="extra compiler flags, one string")
    ap.add_argument("--diff", nargs=2, metavar=("BEFORE", "AFTER"), help="compare two saved outputs by kernel name")
    a = ap.parse_args()
    sys.exit(0 if (diff(*a.diff) if a.diff else report(a.files, shlex.split(a.flags))) else 1)
