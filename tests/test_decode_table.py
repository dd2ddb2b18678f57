"""CPU: make_decode_table (sda_amd/csrc/decode_tables.h), the host builder of the decoded reveal's table, word for word
against Python integers, under ASan and UBSan.

tests/host_c/decode_table.cc is a stand-alone program (its own main) around the builder; it is compiled here for the
host alone with ROCm's clang++ (the sanitizer runtimes linked into the program itself) and run as a child process.
Row j - 1 holds v_j x_j^i R mod p for i < r and zeros up to rmax, v_j = 1 / prod_{l != j} (x_j - x_l) over all
n_idx + 1 points; then x_j^{-1} R, x_j R and v_j^{-1} R.  The syndromes these rows spell must vanish on a sharing's
shares, which ties the table to the code and not only to its own formula."""
import os
import subprocess

import numpy as np
import pytest

from tests import share_check_model as M
from tests.test_check_plan import _clangxx
from tests.test_checked_reveal_model import SCHEMES, clean_rows, kt_of
from tests.test_decode_plan import plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "decode_table.cc")
CASES = [("b8", 5), ("b8", 8), ("b16", 9), ("b16", 13), ("b16", 16), ("config", 17), ("config", 23), ("config", 26)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    out = tmp_path_factory.mktemp("decode_table") / "decode_table"
    build = subprocess.run([cxx, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(out)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return str(out)


def _run(exe, sch, idx, rmax):
    args = [sch.secret_count, sch.privacy_threshold(), sch.prime_modulus, sch.omega_secrets, sch.omega_shares, rmax,
            len(idx)] + list(idx)
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.split("\n")
    return lines[0], [int(x) for x in lines[1:] if x]


def multipliers(xs, p):
    """v_j for j = 0 .. n_idx over all the points."""
    out = []
    for j, x in enumerate(xs):
        d = 1
        for l, y in enumerate(xs):
            if l != j:
                d = d * (x - y) % p
        out.append(pow(d, p - 2, p))
    return out


@pytest.mark.parametrize("name,n_idx", CASES)
def test_table_words_are_the_python_integers(exe, oracle, name, n_idx):
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    r = n_idx - kt
    rmax = plan(n_idx, sch.secret_count, sch.privacy_threshold())[4]
    rng = np.random.default_rng(40 + n_idx)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    head, words = _run(exe, sch, idx, rmax)
    assert head == "duplicate 0" and len(words) == (rmax + 3) * n_idx
    xs = M.points(sch, idx)
    v = multipliers(xs, p)
    R = 1 << 32
    want = []
    for j in range(1, n_idx + 1):
        want += [v[j] * pow(xs[j], i, p) * R % p if i < r else 0 for i in range(rmax)]
    want += [pow(xs[j], p - 2, p) * R % p for j in range(1, n_idx + 1)]
    want += [xs[j] * R % p for j in range(1, n_idx + 1)]
    want += [pow(v[j], p - 2, p) * R % p for j in range(1, n_idx + 1)]
    assert words == want
    # the rows are a parity check of the code: every syndrome of a sharing vanishes, and a single fault shows in all
    rows, _, _ = clean_rows(oracle, sch, rng, batches=2)
    y = [int(s) % p for s in rows[idx][:, 0]]
    Rinv = pow(R, p - 2, p)
    syn = [sum(words[(j - 1) * rmax + i] * Rinv * y[j - 1] for j in range(1, n_idx + 1)) % p for i in range(r)]
    assert syn == [0] * r
    y[n_idx // 2] = (y[n_idx // 2] + 1) % p
    syn = [sum(words[(j - 1) * rmax + i] * Rinv * y[j - 1] for j in range(1, n_idx + 1)) % p for i in range(r)]
    assert all(syn)


def test_repeated_indices_are_reported(exe):
    sch = SCHEMES["config"]
    head, words = _run(exe, sch, list(range(16)) + [3], 4)
    assert head == "duplicate 1" and not words
