"""A plain big-integer model of the two role pipelines: Python integers, an explicit wrap64 and a truncated
remainder (the sign of the dividend), one function per reference step.  It is the second, independent reference of
tests/test_gpu_pipeline_matrix.py, next to the step-wise flow over the C oracle (tests/oracle_backend.py).

Two things are taken from the oracle and are not this model's subject: the ChaCha draws of a seed and the
packed-Shamir share generation and reveal (pinned by their own KATs and matrices).  CPU only; no product import beyond
the scheme descriptors.

A reference panic is ModelError(PRECONDITION), a reference Err its status (include/sda_engine.h).  Moduli of i64::MIN
are outside the engine's documented domain and raise UNSUPPORTED here as well.
"""
import numpy as np

from oracle import oracle as O
from sda_amd import schemes as S
from tests import pipeline_dispatch as PD
from tests.oracle_backend import OracleBackend

I64_MIN, I64_MAX = PD.I64_MIN, PD.I64_MAX
EXACT, CANONICAL = PD.EXACT, PD.CANONICAL


class ModelError(Exception):
    def __init__(self, status, cls):
        self.status, self.cls = status, cls
        super().__init__(f"{status}: {cls}")


def wrap64(x):
    """Rust release arithmetic on i64."""
    return (x + 2**63) % 2**64 - 2**63


def trem(x, m):
    """Rust's i64 `x % m`: the remainder has the dividend's sign, the divisor's sign does not matter; `% 0` panics."""
    if m == 0:
        raise ModelError(PD.PRECONDITION, "divisor of zero")
    if m == I64_MIN:
        raise ModelError(PD.UNSUPPORTED, "i64::MIN")
    m = abs(m)
    return -((-x) % m) if x < 0 else x % m


# ---------------------------------------------------------------- one function per reference step
def full_mask(s, mask, m):
    """full.rs:30 / chacha.rs:44: (secret + mask) % modulus."""
    return trem(wrap64(s + mask), m)


def unmask(ms, mask, q):
    """full.rs:62 / chacha.rs:88: (masked_secret - mask) % modulus."""
    return trem(wrap64(ms - mask), q)


def positive(v, m):
    """receive.rs:15: if v < 0 { v + modulus } else { v }, any modulus."""
    return wrap64(v + m) if v < 0 else v


def additive_shares(secret, draws, m):
    """additive.rs:42-48: the draws, then fold(secret, |sum, x| (sum - x) % modulus)."""
    last = secret
    for x in draws:
        last = trem(wrap64(last - x), m)
    return list(draws) + [last]


def combine_rows(rows, m, mismatch):
    """full.rs:39-48 / additive.rs:57-69: result[ix] += value; result[ix] %= modulus over the rows in order, the length
    of row i checked when row i is reached (`mismatch` is what the reference does then)."""
    dim = len(rows[0]) if rows else 0
    out = [0] * dim
    for row in rows:
        if len(row) != dim:
            raise mismatch
        out = [trem(wrap64(r + int(v)), m) for r, v in zip(out, row)]
    return out


def chacha_draws(m, seed_words, count):
    """The first `count` gen_range(0, m) values of ChaChaRng::from_seed(seed_words) -- from the oracle: one seed
    combined onto zeros is (0 + draw) % m = draw."""
    seed = np.asarray([int(w) & 0xFFFFFFFF for w in seed_words], np.int64).reshape(1, -1)
    if seed.shape[1] == 0:
        seed = np.zeros((1, 1), np.int64)            # from_seed(&[]) is the all-zero key
    return [int(v) for v in O.chacha_mask_combine(m, count, seed)]


def chacha_mask_combine(m, dimension, seeds):
    """chacha.rs:57-76."""
    out = [0] * dimension                             # :58
    for seed in seeds:
        if dimension and m <= 0:
            raise ModelError(PD.PRECONDITION, "gen_range")       # :69 gen_range(0, m) panics
        draws = chacha_draws(m, seed, dimension)
        out = [trem(wrap64(r + d), m) for r, d in zip(out, draws)]          # :70-71
    return out


def packed_reveal(ss, dimension, indexed, mode):
    """batched.rs:69-97 over tss' reconstruct (the oracle); CANONICAL: the residues in [0, p) of the same values."""
    B = PD.batches(ss, dimension)
    if B == 0:
        return []                                     # batched.rs:82: no batch, nothing is read
    rows = [r for _, r in indexed]
    enough = len(rows) >= ss.reconstruction_threshold()
    if any(len(r) < (B if enough else 1) for r in rows):
        raise ModelError(PD.PRECONDITION, "index out of bounds")             # batched.rs:84
    if not enough:
        raise ModelError(PD.NOT_ENOUGH_SHARES, "Not enough shares")          # packed_shamir.rs:75, at batch 0
    if mode == CANONICAL and PD.has_duplicates([i for i, _ in indexed]):
        raise ModelError(PD.UNSUPPORTED, "distinct clerk indices")           # the engine's canonical reveal
    exact = [int(v) for v in OracleBackend().secret_reconstruct(ss, dimension, [(i, list(r)) for i, r in indexed])]
    return [v % ss.prime_modulus for v in exact] if mode == CANONICAL else exact


# ---------------------------------------------------------------- the pipelines
def mask_combine(ms, masks):
    """receive.rs:101-117 over masking/{none,full,chacha}.rs."""
    if isinstance(ms, S.NoMasking):
        if any(len(r) for r in masks):
            raise ModelError(PD.PRECONDITION, "masks.iter().all")            # none.rs:23
        return []
    if isinstance(ms, S.FullMasking):
        return combine_rows(masks, ms.modulus, ModelError(PD.PRECONDITION, "mask.len() == dimension"))
    return chacha_mask_combine(ms.modulus, ms.dimension, [list(r)[:8] for r in masks])


def recipient(ms, masks, ss, dimension, indexed, m_out, mode=EXACT):
    """receive.rs:101-157 and RecipientOutput::positive (:14-20): the output values."""
    return recipient_steps(ms, masks, ss, dimension, indexed, m_out, mode)[2]


def recipient_steps(ms, masks, ss, dimension, indexed, m_out, mode=EXACT):
    """(combined mask, masked output, positive output) of the same flow."""
    mask = mask_combine(ms, masks)
    if isinstance(ss, S.Additive):                    # :120-146
        masked = combine_rows([r for _, r in indexed], ss.modulus,
                              ModelError(PD.MISMATCHING_DIMENSION, "Mismatching dimension"))
    else:
        masked = packed_reveal(ss, dimension, indexed, mode)
    if isinstance(ms, S.NoMasking):                   # :149-152; none.rs:28-32
        out = masked
    else:
        if len(mask) != len(masked):
            raise ModelError(PD.PRECONDITION, "mask.len() == masked_secrets.len()")
        out = [unmask(v, k, ms.modulus) for v, k in zip(masked, mask)]
    return mask, masked, [positive(v, m_out) for v in out]


def mask_secrets(ms, secrets, seed=None, full_masks=None):
    """participate.rs:53-54 over masking/{none,full,chacha}.rs: the masked secrets."""
    if isinstance(ms, S.NoMasking):
        return [int(s) for s in secrets]
    if isinstance(ms, S.ChaChaMasking):
        if ms.dimension != len(secrets):
            raise ModelError(PD.PRECONDITION, "dimension == secrets.len()")  # chacha.rs:26
        if len(seed) != ms.seed_words():
            raise ModelError(PD.PRECONDITION, "seed words")      # the caller stands in for chacha.rs:29-33
    if len(secrets) and ms.modulus <= 0:
        raise ModelError(PD.PRECONDITION, "gen_range")           # full.rs:25 / chacha.rs:38
    draws = full_masks if isinstance(ms, S.FullMasking) else chacha_draws(ms.modulus, list(seed)[:8], len(secrets))
    return [full_mask(int(s), int(d), ms.modulus) for s, d in zip(secrets, draws)]


def share_generate(ss, masked, draws, mode=EXACT):
    """participate.rs:75-76: shares [n][B].  Additive: the fold above; PackedShamir: the oracle (tss share)."""
    if isinstance(ss, S.Additive):
        n, D = ss.share_count, len(masked)
        if n == 0:
            raise ModelError(PD.PRECONDITION, "share_count - 1 underflows")  # additive.rs:42
        if ss.modulus <= 0:
            raise ModelError(PD.PRECONDITION, "gen_range")                   # additive.rs:43
        cols = [additive_shares(int(masked[d]), [int(x) for x in draws[d * (n - 1):(d + 1) * (n - 1)]], ss.modulus)
                for d in range(D)]
        return [[cols[d][j] for d in range(D)] for j in range(n)]
    if len(masked) == 0:
        return [[] for _ in range(ss.share_count)]
    sh = OracleBackend().share_generate(ss, np.asarray(masked, np.int64), np.asarray(draws, np.int64))
    p = ss.prime_modulus
    return [[int(v) % p if mode == CANONICAL else int(v) for v in row] for row in sh]


def participant(ms, ss, secrets, draws, seed=None, full_masks=None, mode=EXACT):
    """participate.rs:53-76: (masked secrets, shares [n][B])."""
    masked = mask_secrets(ms, secrets, seed=seed, full_masks=full_masks)
    return masked, share_generate(ss, masked, draws, mode)


def payloads(shares):
    """sodium.rs:36-41: each clerk's shares as varints (the oracle's encoder) -> (bytes back to back, row byte counts)."""
    blobs = [O.varint_encode(np.asarray(row, np.int64)) if len(row) else b"" for row in shares]
    return b"".join(blobs), [len(b) for b in blobs]
