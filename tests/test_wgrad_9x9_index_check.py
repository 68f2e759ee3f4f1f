"""Host only: builds tools/wgrad_9x9_index_check.cpp and runs it -- the replay on the CPU of wgrad_wave_dma_9x9_kernel's index arithmetic
(deepbedmap_amd/csrc/wgrad_9x9_index.h, which the kernel itself uses): every LDS read inside the launch's allocation and on an initialised
cell, the result exactly a brute-force 3 x 3 weight gradient and element by element the framed scheme's.  Once plain, once under
AddressSanitizer and UBSan (a stand-alone program: nothing is loaded into the interpreter).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return path
    raise AssertionError("no C++ compiler found")


@pytest.mark.parametrize("flags", [["-O2"], SANITIZE], ids=["plain", "asan-ubsan"])
def test_index_check(tmp_path, flags):
    exe = str(tmp_path / "wgrad_9x9_index_check")
    cmd = [compiler(), "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "deepbedmap_amd", "csrc"),
                                                os.path.join(ROOT, "tools", "wgrad_9x9_index_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "wgrad_9x9_index_check: ok" in r.stdout and "339 MFMAs per band" in r.stdout, r.stdout
