"""CPU: packed_reveal_plan (sda_amd/csrc/reveal_plan.h) against the tests' restatement, under ASan and UBSan.

tests/host_c/reveal_plan.cc is a stand-alone program (its own main) that includes only the plan header: it reads
`n_idx k t p mode` lines and prints the plan of each.  It is compiled here with ROCm's clang++ and run as a child
process; the sanitizer runtimes are linked into the program itself.  For every case of the GPU matrix and for a sweep
over the bucket, k and p boundaries, the kernel the plan names must be tests/packed_dispatch.py's reveal_kernel, and
its `logged` and detour answers reveal_fixup_count's rule and reveal_takes_detour.
"""
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

from tests import packed_dispatch as PD
from tests import packed_matrix_cases as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "reveal_plan.cc")

SWEEP_K = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 63, 64, 65, 100)
SWEEP_P = (65537, (1 << 24) - 3, (1 << 24) + 43, 2013265921)     # read only against kLazyTruncMinP: need not be prime


def _clangxx():
    for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or ""):
        if p and os.path.exists(p):
            return p
    return None


def _inputs():
    """(n_idx, k, t, p, mode), the matrix cases first."""
    rows = [(c.n_idx, c.sch.secret_count, c.sch.privacy_threshold(), c.sch.prime_modulus, c.mode)
            for c in PM.REVEAL_CASES]
    for k in SWEEP_K:
        ts = [0] + [t for t in range(1, 17) if (k + t + 1) & (k + t) == 0]
        for t in ts:
            for n_idx in range(max(1, t + k), 131):           # fewer than t + k shares: refused before planning
                for p in SWEEP_P:
                    rows += [(n_idx, k, t, p, PD.EXACT), (n_idx, k, t, p, PD.CANONICAL)]
    return rows


def _kernel_name(path, mode, mm, staged, ku, lazy, full):
    if path == "workspace":
        return "wide"
    b = lambda x: "true" if x else "false"                    # noqa: E731
    if mode == PD.CANONICAL:
        return f"packed_reveal_canon_kernel<{mm}, {b(staged)}>"
    return f"packed_reveal_exact_kernel<{mm}, {b(staged)}, {ku}, {b(lazy)}, {b(full)}>"


def test_reveal_plan_matches_the_restatement_under_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    exe = tmp_path / "reveal_plan"
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-O1", "-g", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    rows = _inputs()
    assert len(rows) > 10000
    text = "".join("%d %d %d %d %d\n" % r for r in rows)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows)
    seen = set()
    for (n_idx, k, t, p, mode), line in zip(rows, lines):
        path, fixup = line.split()[0], line.split()[7]
        kmode, mm, staged, ku, lazy, full = (int(x) for x in line.split()[1:7])
        logged = int(line.split()[8])
        what = f"n_idx={n_idx} k={k} t={t} p={p} mode={mode}: {line}"
        sch = SimpleNamespace(prime_modulus=p, privacy_threshold=lambda t=t: t)
        want = PD.reveal_kernel(sch, n_idx, k, mode)
        name = _kernel_name(path, kmode, mm, staged, ku, lazy, full)
        assert name == want, what
        assert bool(logged) == (PD.reveal_fixup_count(want, {(0, 0)}) == 1), what
        assert (path == "detour") == PD.reveal_takes_detour(n_idx, k, mode), what
        # the fix-up behind a logging launch: a wave per batch up to 64 points, a lane per batch at 96
        assert fixup == (("wave" if mm <= 64 else "lane") if logged else "none"), what
        seen.add(name)
    # the sweep reaches every reveal instantiation the matrix names, and the workspace path
    assert {c.kernel for c in PM.REVEAL_CASES} | {"wide"} <= seen
