"""CPU: make_repair_tables (sda_amd/csrc/packed_common.h), the host builder of the checked reveal's basis Lagrange
rows and inverse weights, against the Lagrange rows of tests/share_check_model.py, under ASan and UBSan.

tests/host_c/repair_tables.cc is a stand-alone program (its own main) around the builder, make_reveal_tables and
make_check_weights; it is compiled here for the host alone with ROCm's clang++ (the sanitizer runtimes linked into the
program itself) and run as a child process.  lam[e][s] must be l_{s+1}(omega_secrets^(e+1)) over the first
L = k + t + 1 points and winv[s] the inverse of the check's weight w[0][s]; with n_idx == k + t there is no winv."""
import os
import subprocess

import numpy as np
import pytest

from tests import checked_reveal_model as R
from tests.test_check_plan import _clangxx
from tests.test_checked_reveal_model import SCHEMES, kt_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "repair_tables.cc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    out = tmp_path_factory.mktemp("repair_tables") / "repair_tables"
    build = subprocess.run([cxx, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(out)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return str(out)


def _run(exe, sch, idx):
    args = [sch.secret_count, sch.privacy_threshold(), sch.prime_modulus, sch.omega_secrets, sch.omega_shares,
            len(idx)] + list(idx)
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.split("\n")
    return lines[0], [int(x) for x in lines[1:] if x]


def _cases():
    rng = np.random.default_rng(41)
    out = []
    for name in ("full_loop", "config", "b8", "b16", "n80"):
        sch = SCHEMES[name]
        kt, n = kt_of(sch), sch.share_count
        for n_idx in sorted({kt, kt + 1, min(kt + 3, n), n}):
            out.append((name, list(range(n_idx))))
            out.append((name, rng.permutation(n)[:n_idx].tolist()))         # a shuffled index subset
    return out


@pytest.mark.parametrize("name,idx", _cases(), ids=lambda v: v if isinstance(v, str) else f"from{len(v)}-first{v[0]}")
def test_tables_are_the_models_lagrange_rows(exe, name, idx):
    sch = SCHEMES[name]
    p, k, kt = sch.prime_modulus, sch.secret_count, kt_of(sch)
    head, words = _run(exe, sch, idx)
    assert head == "duplicate 0"
    lam, winv = R.basis_rows(sch, idx)
    want = [x for row in lam for x in row] + (winv or [])
    assert len(words) == k * kt + (kt if len(idx) > kt else 0)
    assert words == want, (name, idx)
    assert all(0 <= x < p for x in words) and all(0 < x for x in words[k * kt:])


def test_repeated_indices_are_reported(exe):
    sch = SCHEMES["config"]
    assert _run(exe, sch, list(range(16)) + [3])[0] == "duplicate 1"
