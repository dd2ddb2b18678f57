"""CPU: tests/decoded_reveal_model.py (the decoded reveal's definitions) held against a brute-force search over every
error set of at most e_max positions, built on share_check_model._consistent, and against the oracle.

Shapes: b8 from 5, 7 and 8 clerks, b16 from 9, 11 and 13.  Words: oracle sharings with 0 .. e_max + 1 planted faults
at random positions, one with every share moved by a constant (a polynomial with f(1) != 0) and one with a fault in
every share.  Every shape must show all three outcomes.  Planted faults within the radius, at positions that mix
basis and check shares, give back the fault-free secrets, and the |E| = 1 answers are share_check_model.verdicts'."""
import itertools

import numpy as np
import pytest

from tests import decoded_reveal_model as D
from tests import share_check_model as M
from tests.test_checked_reveal_model import SCHEMES, clean_rows, kt_of

SHAPES = [("b8", 5), ("b8", 7), ("b8", 8), ("b16", 9), ("b16", 11), ("b16", 13)]
ERRS = lambda p: (1, p - 1, (p - 1) // 2)                              # noqa: E731


def brute(sch, indices, canon):
    """sets[b] by the definition: the smallest E with |E| <= e_max whose removal leaves the points consistent."""
    p, L = sch.prime_modulus, kt_of(sch) + 1
    n_idx, B = canon.shape
    xs = M.points(sch, indices)
    Y = np.zeros((n_idx + 1, B), np.int64)
    Y[1:] = canon % p
    sets = [None] * B
    for b in np.flatnonzero(M._consistent(xs, Y, L, p)):
        sets[b] = []
    for size in range(1, (n_idx - (L - 1)) // 2 + 1):
        found = {}
        for E in itertools.combinations(range(1, n_idx + 1), size):
            keep = [i for i in range(n_idx + 1) if i not in E]
            ok = M._consistent([xs[i] for i in keep], Y[keep], L, p)
            for b in np.flatnonzero(ok):
                if sets[b] is None:
                    assert b not in found, "two error sets of one size explain a batch"
                    found[b] = list(E)
        for b, E in found.items():
            sets[b] = E
    return sets


def planted_words(rows, idx, sch, rng, per_count=6):
    """([n_idx][B] canonical shares, planted[b] = sorted 1-based positions or None for the moved / all-faulted words)."""
    p, n_idx = sch.prime_modulus, len(idx)
    e_max = (n_idx - kt_of(sch)) // 2
    base = rows[idx] % p
    cols, planted = [], []
    for count in range(e_max + 2):
        for i in range(per_count):
            col = base[:, (len(cols)) % base.shape[1]].copy()
            pos = sorted(rng.choice(n_idx, count, replace=False).tolist())
            for j in pos:
                col[j] = (col[j] + ERRS(p)[(i + j) % 3]) % p
            cols.append(col)
            planted.append([j + 1 for j in pos])
    cols.append((base[:, 0] + 7) % p)                                  # every share moved: f(1) != 0
    planted.append(None)
    cols.append((base[:, 1] + rng.integers(1, p, n_idx)) % p)          # a fault in every share
    planted.append(None)
    return np.stack(cols, axis=1), planted


def test_the_linear_solver_and_the_division():
    p = 433
    assert D._solve([[1, 1], [1, 2]], [3, 5], p) == [1, 2]
    assert D._solve([[1, 1], [2, 2]], [3, 5], p) is None
    assert D._solve([[1, 1], [2, 2]], [3, 6], p) == [3, 0]
    q, rem = D._divide([2, 3, 1], [1, 1], p)                          # (x + 1)(x + 2)
    assert q == [2, 1] and not any(rem)
    assert any(D._divide([3, 3, 1], [1, 1], p)[1])


@pytest.mark.parametrize("name,n_idx", SHAPES)
def test_model_equals_the_search_over_all_error_sets(oracle, name, n_idx):
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    e_max = (n_idx - kt) // 2
    assert e_max >= 1
    rng = np.random.default_rng(100 * n_idx + kt)
    rows, Dm, secrets = clean_rows(oracle, sch, rng, batches=8)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    words, planted = planted_words(rows, idx, sch, rng)
    verdict, wrong, sets = D.decode(sch, idx, words)
    want = brute(sch, idx, words)
    assert sets == want
    outcomes = {"consistent" if E == [] else "undecodable" if E is None else "decoded" for E in sets}
    assert outcomes == {"consistent", "decoded", "undecodable"}
    for b, E in enumerate(sets):
        assert verdict[b] == (D.UNDECODABLE if E is None else len(E))
        assert wrong[b] == (0 if E is None else sum(1 << (j - 1) for j in E))
        if planted[b] is not None and len(planted[b]) <= e_max:
            assert E == planted[b]                                     # within the radius: exactly what was planted
        if planted[b] is None:
            assert E is None
    assert {len(E) for E in sets if E} == set(range(1, e_max + 1))
    # |E| = 1 is the share check's "located at j", in both directions (r >= 2 here)
    located = M.verdicts(sch, idx, words)
    for b, E in enumerate(sets):
        if E is not None and len(E) == 1:
            assert located[b] == E[0]
        if 1 <= located[b] <= n_idx:
            assert E == [int(located[b])]
        if located[b] == 0:
            assert E == []


@pytest.mark.parametrize("name,n_idx", SHAPES)
def test_faults_within_the_radius_give_back_the_fault_free_secrets(oracle, name, n_idx):
    sch = SCHEMES[name]
    p, k, kt = sch.prime_modulus, sch.secret_count, kt_of(sch)
    e_max = (n_idx - kt) // 2
    rng = np.random.default_rng(7 * n_idx)
    rows, Dm, secrets = clean_rows(oracle, sch, rng, batches=6)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    sh = rows[idx].copy()
    # batch b: positions that mix basis and check shares where e_max allows it
    plans = [[0], [n_idx - 1], [kt - 1, kt][:e_max], [0, n_idx - 1, kt][:e_max], list(range(e_max)),
             list(range(n_idx - e_max, n_idx))]
    for b, pos in enumerate(plans):
        for j in pos:
            sh[j, b] += ERRS(p)[(b + j) % 3]
    out, verdict, wrong, sets = D.reveal_one(oracle, sch, Dm, idx, sh)
    assert [E for E in sets] == [sorted(j + 1 for j in pos) for pos in plans]
    assert np.array_equal(out, secrets)
    # one fault past the radius: the reveal from the first k + t shares, flagged
    over = rows[idx].copy()
    for j in list(range(e_max)) + [n_idx - 1]:
        over[j, 2] += 1
    out, verdict, wrong, sets = D.reveal_one(oracle, sch, Dm, idx, over)
    assert verdict.tolist() == [0, 0, D.UNDECODABLE, 0, 0, 0] and wrong[2] == 0
    from tests import checked_reveal_model as R
    first = R._reveal(oracle, sch, Dm, idx[:kt], over[:kt] % p)
    assert np.array_equal(out, first) and not np.array_equal(out[2 * k:3 * k], secrets[2 * k:3 * k])


def test_reveal_summarises_the_call(oracle):
    sch = SCHEMES["b16"]
    rng = np.random.default_rng(5)
    rows, Dm, secrets = clean_rows(oracle, sch, rng, batches=6)
    idx = list(range(13))                                              # r = 6, e_max = 3
    sh = np.stack([rows[idx], rows[idx]])
    sh[1, 2, 1] += 1
    sh[1, 12, 1] -= 1
    sh[1, 5, 4] += 3
    for j in range(4):
        sh[0, j, 3] += 1                                               # four faults: undecodable
    out, verdict, wrong, r, radius, bad, first, undecoded, blame = D.reveal(oracle, sch, Dm, idx, sh)
    assert (r, radius, bad, first, undecoded) == (6, 3, 3, 3, 1)
    assert verdict[1].tolist() == [0, 2, 0, 0, 1, 0] and verdict[0, 3] == D.UNDECODABLE
    assert wrong[1, 1] == (1 << 2) | (1 << 12) and wrong[1, 4] == 1 << 5 and wrong[0, 3] == 0
    assert blame[2] == blame[12] == blame[5] == 1 and sum(blame) == 3
    assert np.array_equal(out[1], secrets)
