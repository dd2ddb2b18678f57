"""CPU: packed_repair_plan (sda_amd/csrc/repair_plan.h) against a Python restatement.

tests/host_c/repair_plan.cc is a stand-alone program (its own main) that includes only the plan header: it reads
`n_idx k t` lines and prints the plan of each.  It is compiled here with ROCm's clang++ (the sanitizer runtimes linked
into the program itself) and run as a child process.  Cases: every n_idx from k + t - 1 to n for the schemes of
tests/test_checked_reveal_model.py, and a sweep over (k, t) that crosses the bucket edges 8/9, 16/17 and 32/33 and
the edge k = 8/9.  configs[2]'s scheme and the full-loop scheme must be fused from every clerk count."""
import os
import subprocess

import pytest

from sda_amd import schemes as S
from tests.test_check_plan import _clangxx
from tests.test_checked_reveal_model import SCHEMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "repair_plan.cc")


def plan(n_idx, k, t):
    """(redundancy, path, bucket, locate) as the header decides them."""
    r = n_idx - (k + t)
    if r < 0:
        return 0, "nothing", 0, 0
    if n_idx <= 32 and k <= 8:
        return r, "fused", 8 if n_idx <= 8 else 16 if n_idx <= 16 else 32, int(r >= 2)
    return r, "composed", 0, int(r >= 2)


def _inputs():
    rows = []
    for sch in SCHEMES.values():
        k, t = sch.secret_count, sch.privacy_threshold()
        rows += [(n_idx, k, t) for n_idx in range(k + t - 1, sch.share_count + 1)]
    for k, t in ((1, 0), (1, 2), (3, 4), (5, 2), (8, 7), (8, 23), (9, 6), (11, 4), (17, 14), (33, 30), (500, 11),
                 (511, 512)):
        for n_idx in sorted({k + t - 1, k + t, k + t + 1, k + t + 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 64, 80, 1023}):
            if n_idx >= max(k + t - 1, 1):
                rows.append((n_idx, k, t))
    return rows


def test_restatement_covers_the_edges_and_the_named_schemes_are_fused():
    assert plan(8, 3, 4) == (1, "fused", 8, 0) and plan(9, 3, 4) == (2, "fused", 16, 1)
    assert plan(7, 3, 4) == (0, "fused", 8, 0) and plan(6, 3, 4) == (0, "nothing", 0, 0)
    assert plan(16, 8, 7) == (1, "fused", 16, 0) and plan(17, 8, 7) == (2, "fused", 32, 1)
    assert plan(32, 8, 7)[1:3] == ("fused", 32) and plan(33, 8, 7)[1:3] == ("composed", 0)
    assert plan(16, 9, 6)[1:3] == ("composed", 0) and plan(31, 8, 23) == (0, "fused", 32, 0)
    assert plan(1023, 500, 11) == (512, "composed", 0, 1)
    for sch in (S.CONFIG_PACKED, S.FULL_LOOP_PACKED):
        k, t = sch.secret_count, sch.privacy_threshold()
        assert all(plan(n_idx, k, t)[1] == "fused" for n_idx in range(k + t, sch.share_count + 1))


def test_repair_plan_matches_the_restatement_under_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    exe = tmp_path / "repair_plan"
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-O1", "-g", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    rows = _inputs()
    seen = {(plan(*r)[1], plan(*r)[2]) for r in rows}
    assert {("fused", 8), ("fused", 16), ("fused", 32), ("composed", 0), ("nothing", 0)} <= seen
    text = "".join("%d %d %d\n" % r for r in rows)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows)
    for (n_idx, k, t), line in zip(rows, lines):
        r, path, bucket, locate = line.split()
        assert (int(r), path, int(bucket), int(locate)) == plan(n_idx, k, t), (n_idx, k, t, line)
    for sch in (S.CONFIG_PACKED, S.FULL_LOOP_PACKED):      # the header itself, not only the restatement
        k, t = sch.secret_count, sch.privacy_threshold()
        mine = [l.split()[1] for (n_idx, kk, tt), l in zip(rows, lines) if (kk, tt) == (k, t) and k + t <= n_idx <= sch.share_count]
        assert mine and set(mine) == {"fused"}
