"""The checked reveal's definitions (include/sda_engine.h, "checked reveal") from the share check's model and the
oracle's reveal.

Verdicts come from tests/share_check_model.py.  Per batch the secrets are oracle.positive(oracle.packed_reconstruct)
of the residues of
    all shares                       (verdict 0),
    the shares without position j    (located at j),
    the first k + t shares           (not located),
so nothing here is shared with the engine: no parity weights, no basis Lagrange rows, no correction formula.  The
oracle runs once per distinct verdict of a vector, over all of its batches, and each batch takes the run of its own
verdict.  Shares are reduced mod p first: the definitions are about residues, and the oracle's wrapping i64 steps are
only exact for values in (-p, p).

basis_rows / correct_basis restate, in Python integers, the formula the engine's fix-up uses; the CPU tests hold it
against the leave-one-out reveal.
"""
import numpy as np

from tests import share_check_model as M

UNLOCATED = M.UNLOCATED


def _params(O, sch):
    return O.packed_params(sch.secret_count, sch.share_count, sch.privacy_threshold(), sch.prime_modulus,
                           sch.omega_secrets, sch.omega_shares)


def _reveal(O, sch, D, idx, rows):
    rc, out = O.packed_reconstruct(_params(O, sch), D, [int(i) for i in idx], np.ascontiguousarray(rows))
    assert rc == 0
    return np.asarray(O.positive(sch.prime_modulus, out), np.int64)


def reveal_one(O, sch, D, indices, shares, verdict=None):
    """shares: [n_idx][B] integers of any magnitude.  Returns (out [D] in [0, p), verdict [B])."""
    p, k = sch.prime_modulus, sch.secret_count
    kt = k + sch.privacy_threshold()
    n_idx = len(indices)
    canon = np.asarray(shares, np.int64).reshape(n_idx, -1) % p
    if verdict is None:
        verdict = M.verdicts(sch, indices, canon)
    out = np.zeros(D, np.int64)
    for v in np.unique(verdict):
        if v == 0:
            keep = list(range(n_idx))
        elif v == UNLOCATED:
            keep = list(range(kt))
        else:
            keep = [i for i in range(n_idx) if i != v - 1]
        full = _reveal(O, sch, D, [indices[i] for i in keep], canon[keep])
        for b in np.flatnonzero(verdict == v):
            out[b * k:min((b + 1) * k, D)] = full[b * k:min((b + 1) * k, D)]
    return out, verdict


def reveal(O, sch, D, indices, shares_vnb):
    """shares_vnb: [V][n_idx][B].  (out [V][D], verdict [V][B], redundancy, bad_batches, first_bad, blame)."""
    verdict, r, bad, first, blame = M.summary(sch, indices, np.asarray(shares_vnb, np.int64) % sch.prime_modulus)
    out = np.stack([reveal_one(O, sch, D, indices, s, verdict[v])[0] for v, s in enumerate(shares_vnb)])
    return out, verdict, r, bad, first, blame


def basis_rows(sch, indices):
    """(lam[e][s], winv[s]): lam = l_{s+1}(omega_secrets^(e+1)) over the first L = k + t + 1 points, e < k, s < k + t;
    winv[s] = 1 / w[0][s] for the check's parity row 0, w[0][s] = -l_{s+1}(x_L) (None when there is no row)."""
    p, k = sch.prime_modulus, sch.secret_count
    L = k + sch.privacy_threshold() + 1
    xs = M.points(sch, indices)
    targets = [pow(sch.omega_secrets, e + 1, p) for e in range(k)]
    lam = [row[1:] for row in M._lagrange_rows(xs, L, targets, p)]
    winv = None
    if len(xs) > L:
        w0 = [(-x) % p for x in M._lagrange_rows(xs, L, [xs[L]], p)[0][1:]]
        winv = [pow(x, p - 2, p) for x in w0]
    return lam, winv


def correct_basis(sch, indices, shares_b, j):
    """One batch (shares_b: n_idx residues) located at the basis position j (1-based, j <= k + t): the basis reveal
    minus lam[e][j-1] * syndrome_0 * winv[j-1], in Python integers."""
    p, k = sch.prime_modulus, sch.secret_count
    kt = k + sch.privacy_threshold()
    lam, winv = basis_rows(sch, indices)
    xs = M.points(sch, indices)
    w0 = [(-x) % p for x in M._lagrange_rows(xs, kt + 1, [xs[kt + 1]], p)[0][1:]]
    y = [int(v) % p for v in shares_b]
    s0 = (y[kt] + sum(w0[s] * y[s] for s in range(kt))) % p
    err = s0 * winv[j - 1] % p
    return [(sum(lam[e][s] * y[s] for s in range(kt)) - lam[e][j - 1] * err) % p for e in range(k)]
