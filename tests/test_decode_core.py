"""CPU: the decoder core (sda_amd/csrc/decode_core.h: Berlekamp-Massey, root search, Forney) on the host, under ASan
and UBSan, against tests/decoded_reveal_model.py.

tests/host_c/decode_core.cc is a stand-alone program (its own main): it builds the decode table, forms the syndromes
of each word from the table's Montgomery words as the kernel's lane does, and runs decode_word with the plan's RMAX
instantiation.  It is compiled here for the host alone with ROCm's clang++ (the sanitizer runtimes linked into the
program itself) and run as a child process.  Words are tests/test_decoded_reveal_model.py's (0 .. e_max + 1 planted
faults, every share moved, a fault in every share) for b8, b16 and configs[2]'s scheme from 17, 19, 23 and 26 clerks;
nu, E and every err_j are compared with the model (err_j = the share minus the value of the polynomial through the
points without E)."""
import os
import subprocess

import numpy as np
import pytest

from tests import decoded_reveal_model as D
from tests import share_check_model as M
from tests.test_check_plan import _clangxx
from tests.test_checked_reveal_model import SCHEMES, clean_rows, kt_of
from tests.test_decode_plan import plan
from tests.test_decoded_reveal_model import SHAPES, planted_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "decode_core.cc")
CASES = SHAPES + [("b16", 16), ("config", 17), ("config", 19), ("config", 23), ("config", 26)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    out = tmp_path_factory.mktemp("decode_core") / "decode_core"
    build = subprocess.run([cxx, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(out)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return str(out)


def error_values(sch, idx, word, E):
    """err_j for j in E: y_j - f(x_j), f through the first L points outside E."""
    p, L = sch.prime_modulus, kt_of(sch) + 1
    xs = M.points(sch, idx)
    ys = [0] + [int(v) % p for v in word]
    keep = [i for i in range(len(xs)) if i not in E][:L]
    rows = M._lagrange_rows([xs[i] for i in keep], L, [xs[j] for j in E], p)
    return [(ys[j] - sum(c * ys[i] for c, i in zip(row, keep))) % p for j, row in zip(E, rows)]


@pytest.mark.parametrize("name,n_idx", CASES)
def test_core_matches_the_model(exe, oracle, name, n_idx):
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    e_max = (n_idx - kt) // 2
    rng = np.random.default_rng(900 + n_idx)
    rows, _, _ = clean_rows(oracle, sch, rng, batches=8)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    words, planted = planted_words(rows, idx, sch, rng, per_count=4)
    verdict, wrong, sets = D.decode(sch, idx, words)
    assert {len(E) for E in sets if E} == set(range(1, e_max + 1)) and None in sets and [] in sets
    args = [sch.secret_count, sch.privacy_threshold(), p, sch.omega_secrets, sch.omega_shares, n_idx] + idx
    text = "".join(" ".join(str(int(v)) for v in words[:, b]) + "\n" for b in range(words.shape[1]))
    run = subprocess.run([exe] + [str(a) for a in args], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    assert lines[0] == "rmax %d" % plan(n_idx, sch.secret_count, sch.privacy_threshold())[4]
    assert len(lines) == 1 + words.shape[1]
    for b, line in enumerate(lines[1:]):
        got = [int(x) for x in line.split()]
        E = sets[b]
        if E is None:
            assert got[0] == 0 and got[2] == 0, (b, line, planted[b])
            continue
        assert got[0] == 1 and got[1] == len(E) and got[2] == int(wrong[b]), (b, line, E)
        assert got[3:] == error_values(sch, idx, words[:, b], E), (b, line, E)
