"""The decoded reveal's definitions (include/sda_engine.h, "decoded reveal") in Python integers.

Points of a batch as in tests/share_check_model.py: (1, 0), then (omega_shares^(indices[j-1] + 1), share_j mod p).
With r = n_idx - (k + t) and e_max = r // 2 a bad batch is decoded with error set E iff E lies in 1 .. n_idx,
1 <= |E| <= e_max, the points without E are consistent and no smaller such set exists; else it is undecodable.

The model finds E with a Berlekamp-Welch linear solve per bad batch: a monic E(x) of degree e_max and a Q(x) of degree
< L + e_max with Q(x_i) = y_i E(x_i) at all n_idx + 1 points (Gaussian elimination mod p).  When at most e_max points
are wrong, every solution has Q = f E for the one polynomial f of degree < L within that distance of the word; the
model divides, and then checks the definition itself: f has degree < L, f(1) = 0 (point 0 is never in E), and E is the
set of positions where f misses the share, at most e_max of them.  Nothing here is shared with the engine: no
syndromes, no Berlekamp-Massey, no Forney, no Montgomery form.

Secrets come from the oracle as tests/checked_reveal_model.py gets them: its canonical reveal of the shares without E,
or of the first k + t shares for an undecodable batch.
"""
import numpy as np

from tests import checked_reveal_model as R
from tests import share_check_model as M

UNDECODABLE = 0xFFFF


def _solve(rows, rhs, p):
    """One solution of rows * x = rhs mod p (free unknowns 0), or None."""
    n_eq, n_un = len(rows), len(rows[0])
    a = [list(row) + [b] for row, b in zip(rows, rhs)]
    pivots, rank = [], 0
    for col in range(n_un):
        piv = next((i for i in range(rank, n_eq) if a[i][col]), None)
        if piv is None:
            continue
        a[rank], a[piv] = a[piv], a[rank]
        inv = pow(a[rank][col], p - 2, p)
        a[rank] = [v * inv % p for v in a[rank]]
        for i in range(n_eq):
            if i != rank and a[i][col]:
                c = a[i][col]
                a[i] = [(v - c * w) % p for v, w in zip(a[i], a[rank])]
        pivots.append(col)
        rank += 1
    if any(a[i][n_un] for i in range(rank, n_eq)):
        return None
    x = [0] * n_un
    for i, col in enumerate(pivots):
        x[col] = a[i][n_un]
    return x


def _divide(num, den, p):
    """(quotient, remainder) of polynomials as low-first coefficient lists; den is monic."""
    num, q = list(num), [0] * max(len(num) - len(den) + 1, 1)
    for i in range(len(num) - len(den), -1, -1):
        c = num[i + len(den) - 1]
        q[i] = c
        for j, d in enumerate(den):
            num[i + j] = (num[i + j] - c * d) % p
    return q, num


def _eval(poly, x, p):
    acc = 0
    for c in reversed(poly):
        acc = (acc * x + c) % p
    return acc


def decode_one(xs, ys, L, e_max, p):
    """xs, ys: the n_idx + 1 points of one batch (ys[0] == 0).  Returns the sorted error set E (positions 1 .. n_idx),
    [] for a consistent batch, or None when the batch is undecodable."""
    m = len(xs)
    nq = L + e_max
    rows, rhs = [], []
    for x, y in zip(xs, ys):
        pw = [1]
        for _ in range(nq):
            pw.append(pw[-1] * x % p)
        rows.append(pw[:nq] + [(-y * pw[j]) % p for j in range(e_max)])
        rhs.append(y * pw[e_max] % p)
    sol = _solve(rows, rhs, p)
    if sol is None:
        return None
    Q, E = sol[:nq], sol[nq:] + [1]
    f, rem = _divide(Q, E, p)
    if any(rem) or any(f[L:]):
        return None
    f = f[:L]
    if _eval(f, xs[0], p) != ys[0]:
        return None
    err = [j for j in range(1, m) if _eval(f, xs[j], p) != ys[j]]
    return err if len(err) <= e_max else None


def decode(sch, indices, shares):
    """shares: [n_idx][B] integers of any magnitude.  Returns (verdict uint16 [B], wrong uint32 [B], sets) with sets[b]
    the sorted 1-based error set of batch b ([] consistent, None undecodable)."""
    p, L = sch.prime_modulus, sch.secret_count + sch.privacy_threshold() + 1
    n_idx = len(indices)
    xs = M.points(sch, indices)
    assert len(set(xs)) == len(xs), "repeated points"
    sh = np.asarray(shares, dtype=np.int64).reshape(n_idx, -1)
    B = sh.shape[1]
    Y = np.zeros((n_idx + 1, B), dtype=np.int64)
    Y[1:] = sh % p
    r = n_idx - (L - 1)
    assert r >= 0
    e_max = r // 2
    verdict, wrong = np.zeros(B, np.uint16), np.zeros(B, np.uint32)
    sets = [[] for _ in range(B)]
    for b in np.flatnonzero(~M._consistent(xs, Y, L, p)):
        E = decode_one(xs, [int(v) for v in Y[:, b]], L, e_max, p) if e_max else None
        sets[b] = E
        if E is None:
            verdict[b] = UNDECODABLE
        else:
            assert 1 <= len(E) <= e_max
            verdict[b] = len(E)
            wrong[b] = sum(1 << (j - 1) for j in E)
    return verdict, wrong, sets


def reveal_one(O, sch, D, indices, shares, decoded=None):
    """shares: [n_idx][B].  Returns (out [D] in [0, p), verdict [B], wrong [B], sets)."""
    p, k = sch.prime_modulus, sch.secret_count
    kt = k + sch.privacy_threshold()
    n_idx = len(indices)
    canon = np.asarray(shares, np.int64).reshape(n_idx, -1) % p
    verdict, wrong, sets = decoded if decoded is not None else decode(sch, indices, canon)
    out = np.zeros(D, np.int64)
    groups = {}
    for b, E in enumerate(sets):
        groups.setdefault(None if E is None else tuple(E), []).append(b)
    for E, batches in groups.items():
        keep = list(range(kt)) if E is None else [i for i in range(n_idx) if i + 1 not in E]
        full = R._reveal(O, sch, D, [indices[i] for i in keep], canon[keep])
        for b in batches:
            out[b * k:min((b + 1) * k, D)] = full[b * k:min((b + 1) * k, D)]
    return out, verdict, wrong, sets


def reveal(O, sch, D, indices, shares_vnb):
    """shares_vnb: [V][n_idx][B].  (out [V][D], verdict [V][B], wrong [V][B], redundancy, radius, bad_batches,
    first_bad, undecoded, blame[n_idx])."""
    n_idx = len(indices)
    per = [reveal_one(O, sch, D, indices, s) for s in shares_vnb]
    out = np.stack([x[0] for x in per])
    verdict = np.stack([x[1] for x in per])
    wrong = np.stack([x[2] for x in per])
    flat = verdict.reshape(-1)
    bad = np.flatnonzero(flat)
    blame = [int(np.count_nonzero(wrong.reshape(-1) >> np.uint32(j) & np.uint32(1))) for j in range(n_idx)]
    r = n_idx - (sch.secret_count + sch.privacy_threshold())
    return (out, verdict, wrong, r, r // 2, int(bad.size), int(bad[0]) if bad.size else M.NO_BAD,
            int(np.count_nonzero(flat == UNDECODABLE)), blame)
