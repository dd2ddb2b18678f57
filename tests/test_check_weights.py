"""CPU: make_check_weights (sda_amd/csrc/packed_common.h), the host builder of the share check's parity weights, against
the Lagrange rows of tests/share_check_model.py, under ASan and UBSan.

tests/host_c/check_weights.cc is a stand-alone program (its own main) around the builder and make_reveal_tables; it
is compiled here for the host alone with ROCm's clang++ (the sanitizer runtimes linked into the program itself) and
run as a child process.  Weight [c][s] must be -l_{s+1}(x_{L+c}) mod p over the first L = k + t + 1 points, and
nonzero; repeated clerk indices must be reported as such."""
import os
import subprocess

import numpy as np
import pytest

from tests import share_check_model as M
from tests.test_check_plan import _clangxx
from tests.test_share_check_model import SCHEMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "check_weights.cc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    out = tmp_path_factory.mktemp("check_weights") / "check_weights"
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


@pytest.mark.parametrize("name", list(SCHEMES))
def test_weights_are_the_negated_lagrange_rows(exe, name):
    sch = SCHEMES[name]
    p, kt, n = sch.prime_modulus, sch.secret_count + sch.privacy_threshold(), sch.share_count
    rng = np.random.default_rng(21)
    for n_idx in sorted({kt, kt + 1, min(kt + 3, n), n}):
        idx = rng.permutation(n)[:n_idx].tolist()
        head, w = _run(exe, sch, idx)
        assert head == "duplicate 0"
        xs, L = M.points(sch, idx), kt + 1
        want = [(-row[i]) % p for row in M._lagrange_rows(xs, L, xs[L:], p) for i in range(1, L)]
        assert w == want, (name, n_idx)
        assert all(0 < x < p for x in w)


def test_repeated_indices_are_reported(exe):
    sch = SCHEMES["config"]
    assert _run(exe, sch, list(range(16)) + [3])[0] == "duplicate 1"
