"""CPU: make_check_table (sda_amd/csrc/packed_common.h), the host builder of the one device table the share check and
the checked reveal read -- parity rows, basis Lagrange rows, inverse weights -- under ASan and UBSan.

tests/host_c/check_table.cc is a stand-alone program (its own main) around the builder; it is compiled here for the
host alone with ROCm's clang++ (the sanitizer runtimes linked into the program itself) and run as a child process.
The table must have r + k + 1 rows of ks = k + t rounded up to even words with every pad word 0, an all-zero last row
at r = 0, and, out of Montgomery form, the words of make_check_weights / make_repair_tables: the program compares them
with those builders itself, and here they are held against the Lagrange rows of tests/share_check_model.py as
tests/test_check_weights.py and tests/test_repair_tables.py do."""
import os
import subprocess

import numpy as np
import pytest

from tests import checked_reveal_model as R
from tests import share_check_model as M
from tests.test_check_plan import _clangxx
from tests.test_checked_reveal_model import SCHEMES, kt_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "check_table.cc")
CASES = (("b8", 3), ("b8", 4), ("b8", 8), ("config", 26), ("n80", 40))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    out = tmp_path_factory.mktemp("check_table") / "check_table"
    build = subprocess.run([cxx, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(out)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return str(out)


def _run(exe, sch, idx):
    args = [sch.secret_count, sch.privacy_threshold(), sch.prime_modulus, sch.omega_secrets, sch.omega_shares,
            len(idx)] + list(idx)
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr)[-4000:])
    return [ln for ln in run.stdout.split("\n") if ln]


@pytest.mark.parametrize("shuffled", (False, True))
@pytest.mark.parametrize("name,n_idx", CASES, ids=[f"{a}-from{b}" for a, b in CASES])
def test_table_has_the_documented_layout_and_the_builders_words(exe, name, n_idx, shuffled):
    sch = SCHEMES[name]
    p, k, kt = sch.prime_modulus, sch.secret_count, kt_of(sch)
    r, ks = n_idx - kt, (kt + 1) & ~1
    idx = np.random.default_rng(51).permutation(sch.share_count)[:n_idx].tolist() if shuffled else list(range(n_idx))
    lines = _run(exe, sch, idx)
    assert lines[0] == "duplicate 0" and lines[1] == f"rows {r + k + 1} stride {ks}"
    words = np.array([[int(x) for x in ln.split()] for ln in lines[2:]], np.int64)
    assert words.shape == ((r + k + 1) * ks, 2)
    raw, canon = words[:, 0].reshape(r + k + 1, ks), words[:, 1].reshape(r + k + 1, ks)
    assert (raw >= 0).all() and (raw < p).all()
    assert not raw[:, kt:].any()                                             # every pad word
    assert (raw * pow(1 << 32, p - 2, p) % p == canon).all()                 # p < 2^31: the products fit an i64
    xs, L = M.points(sch, idx), kt + 1
    parity = [[(-row[i]) % p for i in range(1, L)] for row in M._lagrange_rows(xs, L, xs[L:], p)]
    lam, winv = R.basis_rows(sch, idx)
    want = parity + lam + [winv if r else [0] * kt]
    assert len(parity) == r and (winv is None) == (r == 0)
    assert canon[:, :kt].tolist() == want, (name, idx)
    if r == 0:
        assert not raw[k].any()                                              # the winv row
    else:
        assert raw[:r, :kt].all() and raw[r + k, :kt].all()                  # no zero weight, no zero inverse


def test_repeated_indices_are_reported(exe):
    sch = SCHEMES["config"]
    assert _run(exe, sch, list(range(16)) + [3]) == ["duplicate 1"]
    assert _run(exe, SCHEMES["b8"], [2, 5, 2]) == ["duplicate 1"]
