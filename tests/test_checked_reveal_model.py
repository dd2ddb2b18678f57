"""CPU: tests/checked_reveal_model.py (the checked reveal's definitions) held against the oracle.

A single fault at every position of a fault-free sharing, basis and check, gives back the fault-free canonical
secrets when r >= 2; the leave-one-out reveal and the corrected-basis formula out - lam * s_0 * winv (Python
integers) agree; r = 0 is the plain canonical reveal, r = 1 and two faults in one batch give the reveal from the first
k + t shares."""
import numpy as np
import pytest

from sda_amd import schemes as S
from tests import checked_reveal_model as R
from tests import packed_matrix_cases as PM
from tests import share_check_model as M

SCHEMES = {
    "b8": PM.scheme_for(1, 2, 8, 434),          # p = 433: the fused kernel's 8-share bucket with r up to 5
    "b16": PM.scheme_for(4, 3, 26),             # the 16-share bucket
    "config": S.CONFIG_PACKED,                  # the 32-share bucket
    "full_loop": S.FULL_LOOP_PACKED,            # r = 0 and r = 1 only
    "n80": PM.scheme_for(8, 7, 80),             # the composed path
}
N_IDX = {"b8": (5, 6, 8), "b16": (9, 10, 16), "config": (17, 26), "n80": (40,)}
B = 6


def kt_of(sch):
    return sch.secret_count + sch.privacy_threshold()


def clean_rows(O, sch, rng, batches=B):
    """([n][B] exact signed shares of one oracle sharing, D with a cut tail batch, the canonical secrets)."""
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    D = batches * k - (1 if k > 1 else 0)
    secrets = rng.integers(0, p, D)
    rows = O.packed_generate(R._params(O, sch), secrets, rng.integers(0, p - 1, batches * t))
    return rows, D, secrets


def test_b8_is_the_issues_scheme():
    sch = SCHEMES["b8"]
    assert (sch.secret_count, sch.privacy_threshold(), sch.share_count, sch.prime_modulus) == (1, 2, 8, 433)


@pytest.mark.parametrize("name", list(N_IDX))
def test_one_fault_at_every_position_gives_back_the_fault_free_secrets(oracle, name):
    sch = SCHEMES[name]
    rng = np.random.default_rng(31)
    rows, D, secrets = clean_rows(oracle, sch, rng)
    p, kt = sch.prime_modulus, kt_of(sch)
    for n_idx in N_IDX[name]:
        idx = rng.permutation(sch.share_count)[:n_idx].tolist()
        sh = rows[idx]
        out, verdict = R.reveal_one(oracle, sch, D, idx, sh)
        assert not verdict.any() and np.array_equal(out, secrets)
        if n_idx - kt < 2:
            continue
        for j0 in range(0, n_idx, B):                      # B positions per pass, one per batch
            bad = sh.copy()
            pos = [(j0 + b) % n_idx for b in range(B)]
            for b, j in enumerate(pos):
                bad[j, b] += 1 + b
            out, verdict = R.reveal_one(oracle, sch, D, idx, bad)
            assert verdict.tolist() == [j + 1 for j in pos]
            assert np.array_equal(out, secrets), (name, n_idx, j0)


@pytest.mark.parametrize("name", list(N_IDX))
def test_leave_one_out_equals_the_corrected_basis_formula(oracle, name):
    sch = SCHEMES[name]
    rng = np.random.default_rng(32)
    rows, D, secrets = clean_rows(oracle, sch, rng, batches=1)
    p, k, kt = sch.prime_modulus, sch.secret_count, kt_of(sch)
    n_idx = N_IDX[name][-1]
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    lam, winv = R.basis_rows(sch, idx)
    assert all(0 < x < p for x in winv)
    base = rows[idx][:, 0]
    assert [sum(lam[e][s] * int(base[s]) for s in range(kt)) % p for e in range(D)] == secrets.tolist()[:D]
    for j in sorted({1, 2, kt // 2 + 1, kt}):              # basis positions, 1-based
        bad = base.copy()
        bad[j - 1] = (bad[j - 1] + 12345) % p
        out, verdict = R.reveal_one(oracle, sch, D, idx, bad.reshape(n_idx, 1))
        assert verdict.tolist() == [j]
        assert R.correct_basis(sch, idx, bad, j)[:D] == out.tolist() == secrets.tolist()


@pytest.mark.parametrize("name", ["full_loop", "config", "b8"])
def test_unlocated_batches_are_the_reveal_from_the_first_shares(oracle, name):
    sch = SCHEMES[name]
    rng = np.random.default_rng(33)
    rows, D, secrets = clean_rows(oracle, sch, rng)
    kt, n = kt_of(sch), sch.share_count
    idx = list(range(n))[::-1][:kt + 1]                    # r = 1: detects and flags only
    bad = rows[idx].copy()
    bad[kt, 2] += 1                                        # the check share: the basis is clean
    bad[0, 4] += 1                                         # a basis share: the basis reveal is wrong
    out, verdict = R.reveal_one(oracle, sch, D, idx, bad)
    assert verdict.tolist() == [0, 0, M.UNLOCATED, 0, M.UNLOCATED, 0]
    k = sch.secret_count
    want = R._reveal(oracle, sch, D, idx[:kt], bad[:kt] % sch.prime_modulus)
    assert np.array_equal(out, want)
    assert np.array_equal(out[:4 * k], secrets[:4 * k]) and not np.array_equal(out[4 * k:5 * k], secrets[4 * k:5 * k])
    out0, v0 = R.reveal_one(oracle, sch, D, idx[:kt], bad[:kt])           # r = 0: the plain canonical reveal
    assert not v0.any() and np.array_equal(out0, want)
    if n - kt >= 3:                                        # two faults in one batch at r >= 3
        idx = list(range(kt + 3))
        two = rows[idx].copy()
        two[1, 3] += 1
        two[kt + 2, 3] -= 1
        out, verdict = R.reveal_one(oracle, sch, D, idx, two)
        assert verdict.tolist() == [0, 0, 0, M.UNLOCATED, 0, 0]
        assert np.array_equal(out, R._reveal(oracle, sch, D, idx[:kt], two[:kt] % sch.prime_modulus))


def test_reveal_summarises_like_the_share_check(oracle):
    sch = SCHEMES["config"]
    rng = np.random.default_rng(34)
    rows, D, secrets = clean_rows(oracle, sch, rng)
    idx = list(range(18))
    sh = np.stack([rows[idx], rows[idx]])
    sh[1, 4, 2] += 1
    sh[1, 17, 5] -= 1
    out, verdict, r, bad, first, blame = R.reveal(oracle, sch, D, idx, sh + sch.prime_modulus * 3)
    assert (r, bad, first) == (3, 2, B + 2) and blame[4] == 1 and blame[17] == 1 and sum(blame) == 2
    assert verdict[1, 2] == 5 and verdict[1, 5] == 18
    assert np.array_equal(out[0], secrets) and np.array_equal(out[1], secrets)
