"""The share consistency check's definitions (include/sda_engine.h, "share consistency check") in Python integers.

Points of a batch: (1, 0), then (omega_shares^(indices[j-1] + 1), share_j mod p) for j = 1 .. n_idx.  A batch is
consistent iff one polynomial of degree < L = k + t + 1 passes through all of them: interpolate through the first L
points and evaluate at the rest.  With r = n_idx - (k + t) >= 2 a bad batch is located at position j iff the points
without point j are consistent (brute-force leave-one-out; at most one j can pass).  Point 0 is never a suspect.

Nothing here is shared with the engine: no Montgomery form, no parity weights, no syndromes.  The scalar work is in
Python integers; the per-batch sums run over numpy int64 columns (p < 2^31, so a product of two residues plus a
residue stays below 2^63, and numpy's `%` by a positive modulus is the mathematical residue).
"""
import numpy as np

UNLOCATED = 0xFFFF
NO_BAD = (1 << 64) - 1


def points(sch, indices):
    p = sch.prime_modulus
    return [1] + [pow(sch.omega_shares, int(i) + 1, p) for i in indices]


def _lagrange_rows(xs, L, targets, p):
    """rows[c][i] = l_i(targets[c]) over the basis xs[:L]."""
    den = []
    for i in range(L):
        d = 1
        for j in range(L):
            if j != i:
                d = d * (xs[i] - xs[j]) % p
        den.append(pow(d, p - 2, p))
    rows = []
    for x in targets:
        row = []
        for i in range(L):
            num = 1
            for j in range(L):
                if j != i:
                    num = num * (x - xs[j]) % p
            row.append(num * den[i] % p)
        rows.append(row)
    return rows


def _consistent(xs, Y, L, p):
    """Y: int64 array [m][B] of residues; True per batch iff the m points lie on a polynomial of degree < L."""
    m = len(xs)
    B = Y.shape[1]
    ok = np.ones(B, dtype=bool)
    if m <= L:
        return ok
    rows = _lagrange_rows(xs, L, xs[L:], p)
    for c, row in enumerate(rows):
        acc = np.zeros(B, dtype=np.int64)
        for i in range(L):
            acc = (acc + np.int64(row[i]) * Y[i]) % p
        ok &= acc == Y[L + c]
    return ok


def verdicts(sch, indices, shares):
    """shares: [n_idx][B] integers (any representatives, any magnitude).  Returns the uint16 verdict per batch."""
    p, L = sch.prime_modulus, sch.secret_count + sch.privacy_threshold() + 1
    n_idx = len(indices)
    xs = points(sch, indices)
    assert len(set(xs)) == len(xs), "repeated points"
    assert 2 < p < 1 << 31
    sh = np.asarray(shares, dtype=np.int64).reshape(n_idx, -1)
    B = sh.shape[1]
    Y = np.zeros((n_idx + 1, B), dtype=np.int64)
    Y[1:] = sh % p
    out = np.zeros(B, dtype=np.uint16)
    r = n_idx - (L - 1)
    assert r >= 0
    bad = ~_consistent(xs, Y, L, p)
    out[bad] = UNLOCATED
    if r >= 2 and bad.any():
        cols = np.flatnonzero(bad)
        Yb = Y[:, cols]
        for j in range(1, n_idx + 1):
            keep = [i for i in range(n_idx + 1) if i != j]
            okj = _consistent([xs[i] for i in keep], Yb[keep], L, p)
            assert not (okj & (out[cols] != UNLOCATED)).any(), "two positions explain one batch"
            out[cols[okj]] = j
    return out


def summary(sch, indices, shares_vnb):
    """shares_vnb: [V][n_idx][B].  (verdict [V][B], redundancy, bad_batches, first_bad, blame[n_idx])."""
    n_idx = len(indices)
    v = np.stack([verdicts(sch, indices, s) for s in shares_vnb])
    flat = v.reshape(-1)
    bad = np.flatnonzero(flat)
    blame = [int(np.count_nonzero(flat == j)) for j in range(1, n_idx + 1)]
    r = n_idx - (sch.secret_count + sch.privacy_threshold())
    return v, r, int(bad.size), int(bad[0]) if bad.size else NO_BAD, blame
