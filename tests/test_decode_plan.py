"""CPU: packed_decode_plan (sda_amd/csrc/decode_plan.h) against a Python restatement.

tests/host_c/decode_plan.cc is a stand-alone program (its own main) that includes only the plan header: it reads
`n_idx k t` lines and prints the plan of each.  It is compiled here with ROCm's clang++ (the sanitizer runtimes linked
into the program itself) and run as a child process.  Cases: every n_idx from k + t - 1 to n for the schemes of
tests/test_checked_reveal_model.py, and a sweep over (k, t) that crosses the bucket edges, the scope's edges 32/33 and
k = 8/9, and every edge of the RMAX list.  configs[2]'s scheme from 26 clerks must decode with RMAX = 12."""
import os
import subprocess

import pytest

from sda_amd import schemes as S
from tests.test_check_plan import _clangxx
from tests.test_checked_reveal_model import SCHEMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "decode_plan.cc")
RMAX = (4, 8, 12, 16, 32)


def plan(n_idx, k, t):
    """(redundancy, radius, path, bucket, rmax, decode) as the header decides them."""
    r = n_idx - (k + t)
    if r < 0:
        return 0, 0, "nothing", 0, 0, 0
    if n_idx > 32 or k > 8:
        return r, r // 2, "unsupported", 0, 0, 0
    bucket = 8 if n_idx <= 8 else 16 if n_idx <= 16 else 32
    if r < 2:
        return r, 0, "first", bucket, 0, 0
    return r, r // 2, "decoded", bucket, min(m for m in RMAX if m >= r), 1


def _inputs():
    rows = []
    for sch in SCHEMES.values():
        k, t = sch.secret_count, sch.privacy_threshold()
        rows += [(n_idx, k, t) for n_idx in range(k + t - 1, sch.share_count + 1)]
    for k, t in ((1, 0), (1, 2), (3, 4), (5, 2), (8, 7), (8, 23), (9, 6), (11, 4), (17, 14), (33, 30), (500, 11)):
        for n_idx in sorted({k + t - 1, k + t, k + t + 1, k + t + 2, k + t + 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64,
                             1023} | {k + t + r for r in (4, 5, 8, 9, 12, 13, 16, 17, 31)}):
            if n_idx >= max(k + t - 1, 1):
                rows.append((n_idx, k, t))
    return rows


def test_restatement_covers_the_edges_and_the_shipped_configuration():
    sch = S.CONFIG_PACKED
    k, t = sch.secret_count, sch.privacy_threshold()
    assert plan(26, k, t) == (11, 5, "decoded", 32, 12, 1) and plan(17, k, t) == (2, 1, "decoded", 32, 4, 1)
    assert plan(16, k, t) == (1, 0, "first", 16, 0, 0) and plan(15, k, t) == (0, 0, "first", 16, 0, 0)
    assert plan(14, k, t)[2] == "nothing"
    assert plan(8, 1, 2) == (5, 2, "decoded", 8, 8, 1) and plan(7, 1, 2)[4] == 4
    assert plan(32, 1, 0) == (31, 15, "decoded", 32, 32, 1)
    assert plan(33, 8, 7)[2] == "unsupported" and plan(20, 9, 6)[2] == "unsupported"
    for n_idx in range(k + t, sch.share_count + 1):
        assert plan(n_idx, k, t)[2] in ("first", "decoded")


def test_decode_plan_matches_the_restatement_under_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    exe = tmp_path / "decode_plan"
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-O1", "-g", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    rows = _inputs()
    seen = {(plan(*r)[2], plan(*r)[4]) for r in rows}
    assert {("decoded", m) for m in RMAX} | {("first", 0), ("nothing", 0), ("unsupported", 0)} <= seen
    text = "".join("%d %d %d\n" % r for r in rows)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows)
    for (n_idx, k, t), line in zip(rows, lines):
        r, rad, path, bucket, rmax, dec = line.split()
        assert (int(r), int(rad), path, int(bucket), int(rmax), int(dec)) == plan(n_idx, k, t), (n_idx, k, t, line)
