"""CPU: tests/share_check_model.py (the share consistency check's definitions) held against the oracle.

Shares that the oracle generates, and their oracle combine over several participants, are consistent from every clerk
set tried at every n_idx >= k + t; the oracle's reconstruct from two different (k + t)-subsets of a consistent batch
agrees mod p; planted errors give the planted verdicts."""
import numpy as np
import pytest

from sda_amd import schemes as S
from tests import packed_matrix_cases as PM
from tests import share_check_model as M

SCHEMES = {
    "config": S.CONFIG_PACKED,
    "full_loop": S.FULL_LOOP_PACKED,
    "n80": PM.scheme_for(8, 7, 80),
    "small_p": PM.scheme_for(3, 4, 26, 1 << 24),
}
B = 5


def _params(O, sch):
    return O.packed_params(sch.secret_count, sch.share_count, sch.privacy_threshold(), sch.prime_modulus,
                           sch.omega_secrets, sch.omega_shares)


def combined_shares(O, sch, rng, participants=3, batches=B):
    """[n][B]: the oracle's clerk combine of `participants` oracle sharings, in mixed representation."""
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    D = batches * k - (1 if k > 1 else 0)                   # a zero-padded tail batch
    gens = [O.packed_generate(_params(O, sch), rng.integers(0, p, D), rng.integers(0, p - 1, batches * t))
            for _ in range(participants)]
    rows = np.stack([O.combine(p, np.stack([g[c] for g in gens])) for c in range(n)])
    canon = rows % p
    flip = rng.integers(0, 2, rows.shape).astype(bool)      # signed and canonical representatives, mixed
    return np.where(flip & (canon != 0), canon - p, canon), D


def n_idx_values(sch):
    kt, n = sch.secret_count + sch.privacy_threshold(), sch.share_count
    if n <= 26:
        return list(range(kt, n + 1))
    return sorted({kt, kt + 1, kt + 2, kt + 3, 32, 33, n})


@pytest.mark.parametrize("name", list(SCHEMES))
def test_oracle_shares_are_consistent_from_every_clerk_count(oracle, name):
    sch = SCHEMES[name]
    rng = np.random.default_rng(11)
    rows, _ = combined_shares(oracle, sch, rng)
    single = oracle.packed_generate(_params(oracle, sch), rng.integers(0, sch.prime_modulus, B * sch.secret_count),
                                    rng.integers(0, sch.prime_modulus - 1, B * sch.privacy_threshold()))
    for n_idx in n_idx_values(sch):
        for idx in (list(range(n_idx)), sorted(rng.permutation(sch.share_count)[:n_idx].tolist()),
                    rng.permutation(sch.share_count)[:n_idx].tolist()):
            for sh in (rows, single):
                v = M.verdicts(sch, idx, sh[idx])
                assert not v.any(), (name, n_idx, idx, v)


@pytest.mark.parametrize("name", list(SCHEMES))
def test_oracle_reconstruct_agrees_from_two_subsets(oracle, name):
    sch = SCHEMES[name]
    rng = np.random.default_rng(12)
    rows, D = combined_shares(oracle, sch, rng)
    p, kt, n = sch.prime_modulus, sch.secret_count + sch.privacy_threshold(), sch.share_count
    a, b = list(range(kt)), list(range(n - kt, n))
    assert a != b
    rc_a, out_a = oracle.packed_reconstruct(_params(oracle, sch), D, a, rows[a])
    rc_b, out_b = oracle.packed_reconstruct(_params(oracle, sch), D, b, rows[b])
    assert rc_a == 0 and rc_b == 0
    assert np.array_equal(out_a % p, out_b % p)


@pytest.mark.parametrize("name", list(SCHEMES))
def test_planted_errors_give_the_planted_verdicts(oracle, name):
    sch = SCHEMES[name]
    rng = np.random.default_rng(13)
    rows, _ = combined_shares(oracle, sch, rng)
    p, kt, n = sch.prime_modulus, sch.secret_count + sch.privacy_threshold(), sch.share_count
    for n_idx in n_idx_values(sch):
        idx = rng.permutation(n)[:n_idx].tolist()
        r = n_idx - kt
        for e in (1, -5):
            sh = rows[idx].copy()
            pos = [int(rng.integers(0, n_idx)) for _ in range(B)]
            pos[0], pos[-1] = 0, n_idx - 1
            for b, j in enumerate(pos):
                sh[j, b] += e
            v = M.verdicts(sch, idx, sh)
            want = [0] * B if r == 0 else [M.UNLOCATED] * B if r == 1 else [j + 1 for j in pos]
            assert v.tolist() == want, (name, n_idx, e)
        # every share moved by the same constant: a polynomial of degree < L with f(1) != 0
        v = M.verdicts(sch, idx, rows[idx] + 7)
        assert v.tolist() == ([0] * B if r == 0 else [M.UNLOCATED] * B), (name, n_idx)
        if r >= 3:                                           # two errors in one batch cannot be one clerk's
            sh = rows[idx].copy()
            sh[0, 1] += 1
            sh[n_idx - 1, 1] -= 1
            assert M.verdicts(sch, idx, sh).tolist() == [0, M.UNLOCATED] + [0] * (B - 2)


def test_summary_counts_blame_and_first_bad(oracle):
    sch = S.CONFIG_PACKED
    rng = np.random.default_rng(14)
    rows, _ = combined_shares(oracle, sch, rng)
    idx = list(range(18))
    sh = np.stack([rows[idx], rows[idx], rows[idx]])
    sh[1, 4, 2] += 1
    sh[2, 17, 0] -= 1
    sh[2, 17, 4] -= 1
    v, r, bad, first, blame = M.summary(sch, idx, sh)
    assert (r, bad, first) == (3, 3, 1 * B + 2)
    assert blame == [0, 0, 0, 0, 1] + [0] * 12 + [2]
    assert v[1, 2] == 5 and v[2, 0] == 18 and v[2, 4] == 18 and np.count_nonzero(v) == 3
    assert M.summary(sch, idx, sh[:1])[1:4] == (3, 0, M.NO_BAD)
