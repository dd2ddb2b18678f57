"""The robust recipient job's definition (include/sda_engine.h, "robust recipient job") in Python integers.

Clerk row i is what the ORACLE decodes from clerk blob i, read over [0, B).  The secrets, verdict, wrong and every
count are tests/decoded_reveal_model.reveal's on those rows (one vector); the combined mask is the oracle's mask
combine (tests/pipeline_model.mask_combine: none.rs / full.rs / chacha.rs); the output is (s - mask) mod p with
Python's big integers -- a residue, not the reference's wrapping `-`.  Nothing here is shared with the engine.
"""
from collections import namedtuple

import numpy as np

from sda_amd import schemes as S
from tests import decoded_reveal_model as DM
from tests import pipeline_dispatch as PD
from tests import pipeline_model as PM

Expected = namedtuple("Expected", "out secrets mask verdict wrong redundancy radius bad_batches first_bad undecoded blame")

# sda_recipient_decoded_last_launch
ROUTE_NONE, ROUTE_FUSED, ROUTE_SEPARATE = 0, 1, 2


def residue(s, mask, p):
    """(s - mask) mod p in [0, p) for integers of any magnitude."""
    return (int(s) - int(mask)) % p


def clerk_rows(indexed_rows, B):
    """[n_idx][B] int64: every clerk's decoded row over [0, B)."""
    return np.asarray([[int(v) for v in list(r)[:B]] for _, r in indexed_rows], np.int64).reshape(len(indexed_rows), B)


def run(O, ms, mask_rows, ss, dimension, indexed_rows, mask=None):
    """indexed_rows: [(clerk index, decoded row)].  mask: the combined mask when the caller hands it over (the device
    form's Full mask), else the oracle's combine of mask_rows."""
    p, k = ss.prime_modulus, ss.secret_count
    B = PD.batches(ss, dimension)
    idx = [i for i, _ in indexed_rows]
    shares = clerk_rows(indexed_rows, B)
    out, verdict, wrong, r, radius, bad, first, undecoded, blame = DM.reveal(O, ss, dimension, idx, shares[None])
    if mask is None:
        mask = PM.mask_combine(ms, mask_rows)
    if isinstance(ms, S.NoMasking):
        mask = [0] * dimension
    assert len(mask) == dimension
    secrets = [int(v) for v in out[0]]
    final = np.asarray([residue(s, m, p) for s, m in zip(secrets, mask)], np.int64)
    return Expected(final, np.asarray(secrets, np.int64), [int(m) for m in mask], verdict[0], wrong[0], r, radius, bad,
                    first, undecoded, blame)


def record(ms, stride, B, fused=True, redo=False):
    """(unmask_route, reveal_runs, compact) of a successful call with a non-empty output: the route from the masking
    alone (the knob SDA_RECIPIENT_FUSE_UNMASK=0: fused=False), two runs only when a ChaCha call's rerun branch is
    taken (SDA_RECIPIENT_REDO=1: no committed input reaches it), compact when the rows' stride is not B."""
    none = isinstance(ms, S.NoMasking)
    route = ROUTE_NONE if none else ROUTE_FUSED if fused else ROUTE_SEPARATE
    return (route, 2 if redo and isinstance(ms, S.ChaChaMasking) else 1, 1 if stride != B else 0)
