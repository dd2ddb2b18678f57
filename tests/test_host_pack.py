"""CPU: the host stream's tile packing (sda_amd/csrc/host_pack.h) under AddressSanitizer and UBSan.

tests/host_c/pack_narrow.cc is a stand-alone program (its own main) that includes the header: pack_rows32 against
a scalar loop -- slices that start and end mid-row, 1 / 3 / 16 threads on a shape where they all run and on a
tiny one, the int32 limits (fit), 2^31 and -2^31 - 1 (do not fit) at the first element, the last element and at
thread boundaries, rows at unaligned addresses -- and pack_rows as a byte copy.  It is compiled here with ROCm's
clang++ and run as a child process; the sanitizer runtimes are linked into the program itself.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "pack_narrow.cc")


def _clangxx():
    for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or ""):
        if p and os.path.exists(p):
            return p
    return None


def test_pack_rows32_matches_scalar_loop_under_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    exe = tmp_path / "pack_narrow"
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-O1", "-g", "-pthread", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    tail = (run.stdout + run.stderr)[-4000:]
    assert run.returncode == 0, tail
    assert run.stdout.strip().endswith("pack_narrow OK"), tail
