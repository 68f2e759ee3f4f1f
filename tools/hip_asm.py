"""The compile step the static ISA tools share (scan_store_drains.py, kernel_isa.py): one .hip source of deepbedmap_amd/csrc to gfx950
assembly text, device side only, with the flags of the library's own build."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepbedmap_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def compile_to_asm(path, extra_flags=()):
    """Returns (assembly text, None), or (None, the end of the compiler's messages) if the source does not compile.  Relative includes
    resolve from the source's own directory."""
    path = os.path.abspath(path)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "a.s")
        r = subprocess.run([HIPCC] + FLAGS + list(extra_flags) + ["--cuda-device-only", "-S", "-o", asm, path],
                           capture_output=True, text=True, cwd=os.path.dirname(path))
        if r.returncode != 0:
            return None, r.stderr[-400:]
        with open(asm) as f:
            return f.read(), None


def demangle(names):
    names = list(names)
    if not names:
        return []
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    return [d.replace("(anonymous namespace)::", "").split("(")[0] for d in out[:len(names)]]
