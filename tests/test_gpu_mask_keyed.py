"""GPU: Full masking with the mask drawn in the kernel (sda_full_mask_keyed_dev and its int32-mask form).

Every expected value comes from the CPU: the mask from tests/draws_model.py, the masked secrets from a big-integer
wrapping add and Rust's truncated `%`.  The same test also holds the kernel to the engine's existing sequence,
sda_draws_dev followed by sda_secret_mask.  Counts stand on both sides of a ChaCha block (8) and of a workgroup's
tile (DRAWS_TILE = 2048); `first` values leave the first and the last block partial and cross the block counter's
word boundary.  Every output buffer carries guard words and is compared whole.
"""
import ctypes as C

import numpy as np
import pytest

from sda_amd import SdaError, schemes as S
from sda_amd import engine as E
from tests import draws_model as DM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEY, STREAM = DM.TEST_KEY, DM.TEST_STREAM
COUNTS = (1, 7, 8, 9, 2047, 2048, 2049, 4097)
FIRSTS = (0, 1, 7, 8, 2041, 2**32 - 3, 2**35 + 5)
M_THIRD = 6148914691236517205                  # floor(2^64 / 3): 3 m = 2^64 - 1, so the zone is all of u64 -- no retry
MODULI = (433, 2147482801, 2**31, 2**31 + 1, M_THIRD, DM.BOUND_THIRD)   # BOUND_THIRD = M_THIRD + 1: one draw in three retries
NMAX = max(COUNTS)
GUARD = 16
POISON64, POISON32 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B
I64_MIN, I64_MAX = -2**63, 2**63 - 1

assert E.DRAWS_TILE == 2048


def _secrets(m):
    """NMAX signed secrets: inside (-m, m), over all of i64, and the edges at the front (a count of 1 rotates through
    them with `first`) and again around the tile boundary."""
    rng = np.random.default_rng(m % 65521)
    v = [int(x) for x in rng.integers(-(m - 1), m, size=NMAX, dtype=np.int64)]
    wide = rng.integers(I64_MIN, I64_MAX, size=NMAX, dtype=np.int64, endpoint=True)
    for i in range(0, NMAX, 3):
        v[i] = int(wide[i])
    edges = [I64_MIN, I64_MAX, m, -m, m - 1, -(m - 1), 0, 5 * m + 3 if 5 * m + 3 <= I64_MAX else I64_MAX - 1]
    for base in (0, 2040, 4089):
        v[base:base + len(edges)] = edges
    return v


def _trem(v, m):
    r = abs(v) % m
    return -r if v < 0 else r


def _wrap(v):
    return (v + 2**63) % 2**64 - 2**63


def _guarded(values, dtype, poison):
    full = np.full(GUARD + len(values) + GUARD, poison, dtype=dtype)
    full[GUARD:GUARD + len(values)] = values
    return full


def _run(engine, m, secrets, count, first, mask32):
    """(masked buffer, mask buffer) of one call, guards included."""
    sec = torch.as_tensor(np.asarray(secrets[:count], dtype=np.int64)).cuda()
    masked = torch.full((count + 2 * GUARD,), POISON64, dtype=torch.int64, device="cuda")
    mask = torch.full((count + 2 * GUARD,), POISON32 if mask32 else POISON64,
                      dtype=torch.int32 if mask32 else torch.int64, device="cuda")
    engine.full_mask_keyed_dev(m, sec.data_ptr(), count, KEY, STREAM, masked.data_ptr() + 8 * GUARD,
                               mask.data_ptr() + (4 if mask32 else 8) * GUARD, first=first, mask32=mask32)
    torch.cuda.synchronize()
    return masked.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("m", MODULI, ids=[f"m{m}" for m in MODULI])
def test_mask_and_masked_secrets(engine, m):
    secrets = _secrets(m)
    sec_np = np.asarray(secrets, dtype=np.int64)
    retried = 0
    for first in FIRSTS:
        mask, rounds = DM.draws_with_rounds(KEY, STREAM, first, NMAX, m)
        retried += int((rounds > 0).sum())
        want_mask = [int(x) for x in mask]
        want_masked = [_trem(_wrap(s + x), m) for s, x in zip(secrets, want_mask)]
        assert 0 <= min(want_mask) and max(want_mask) < m
        # the engine's existing sequence over the whole range: the draws kernel, then sda_secret_mask
        dd = torch.zeros(NMAX, dtype=torch.int64, device="cuda")
        engine.draws_dev(KEY, STREAM, first, NMAX, m, dd.data_ptr())
        torch.cuda.synchronize()
        seq_mask = dd.cpu().numpy()
        got_mask, seq_masked = engine.secret_mask(S.FullMasking(m), sec_np, full_masks=seq_mask)
        assert seq_mask.tolist() == want_mask and got_mask.tolist() == want_mask
        assert seq_masked.tolist() == want_masked
        for count in COUNTS:
            masked, mk = _run(engine, m, secrets, count, first, mask32=False)
            assert np.array_equal(mk, _guarded(want_mask[:count], np.int64, POISON64)), (m, first, count, "mask")
            assert np.array_equal(masked, _guarded(want_masked[:count], np.int64, POISON64)), (m, first, count)
            if m <= 2**31:
                masked, mk = _run(engine, m, secrets, count, first, mask32=True)
                assert mk.dtype == np.int32
                assert np.array_equal(mk, _guarded(np.asarray(want_mask[:count], dtype=np.int64).astype(np.int32),
                                                   np.int32, POISON32)), (m, first, count, "mask32")
                assert np.array_equal(masked, _guarded(want_masked[:count], np.int64, POISON64)), (m, first, count, 32)
            else:
                with pytest.raises(SdaError) as ei:
                    _run(engine, m, secrets, count, first, mask32=True)
                assert ei.value.status == E.ERR_UNSUPPORTED and "2^31" in str(ei.value)
    if m == DM.BOUND_THIRD:
        assert retried > NMAX * len(FIRSTS) // 4            # the retry rounds are exercised
    if m == 2**31:
        assert max(want_mask) >= 2**30                      # int32 values in the top half of the range


def test_int32_mask_is_refused_above_two_to_the_31_and_writes_nothing(engine):
    sec = torch.arange(64, dtype=torch.int64, device="cuda")
    masked = torch.full((64,), POISON64, dtype=torch.int64, device="cuda")
    mask = torch.full((64,), POISON32, dtype=torch.int32, device="cuda")
    with pytest.raises(SdaError) as ei:
        engine.full_mask_keyed_dev(2**31 + 1, sec.data_ptr(), 64, KEY, STREAM, masked.data_ptr(), mask.data_ptr(),
                                   mask32=True)
    torch.cuda.synchronize()
    assert ei.value.status == E.ERR_UNSUPPORTED
    assert (masked == POISON64).all() and (mask == POISON32).all()


@pytest.mark.parametrize("mask32", [False, True], ids=["i64", "int32"])
def test_status_matrix(engine, mask32):
    """The header's checks in its order; a refused call writes nothing."""
    INV, PRE = E.ERR_INVALID_ARGUMENT, E.ERR_PRECONDITION
    sec = torch.arange(8, dtype=torch.int64, device="cuda")
    masked = torch.full((8,), POISON64, dtype=torch.int64, device="cuda")
    mask = torch.full((8,), POISON32 if mask32 else POISON64, dtype=torch.int32 if mask32 else torch.int64,
                      device="cuda")

    def refused(status, text, m=433, d=8, key=KEY, first=0, sec_ptr=sec.data_ptr(), masked_ptr=masked.data_ptr(),
                mask_ptr=mask.data_ptr()):
        with pytest.raises(SdaError) as ei:
            engine.full_mask_keyed_dev(m, sec_ptr, d, key, STREAM, masked_ptr, mask_ptr, first=first, mask32=mask32)
        torch.cuda.synchronize()
        assert ei.value.status == status and text in str(ei.value), str(ei.value)
        assert (masked == POISON64).all() and (mask == (POISON32 if mask32 else POISON64)).all()

    # 1. NULL key / needed buffer, ahead of the modulus
    refused(INV, "NULL", key=None, m=0)
    refused(INV, "NULL", sec_ptr=None, m=0)
    refused(INV, "NULL", masked_ptr=None, m=0)
    refused(INV, "NULL", mask_ptr=None, m=0)
    # 2. modulus <= 0 with gen_range's message, ahead of the wrap
    for bad in (0, -433):
        refused(PRE, "Rng.gen_range called with low >= high", m=bad, first=2**64 - 1)
    # 3. first + dimension wraps, ahead of the int32 form's bound
    refused(INV, "wraps", first=2**64 - 7, m=2**31 + 1)
    # 4. dimension == 0: nothing launched, no buffer needed
    engine.full_mask_keyed_dev(433, None, 0, KEY, STREAM, None, None, first=2**64 - 1, mask32=mask32)
    # the last element of the index space is still served
    engine.full_mask_keyed_dev(433, sec.data_ptr(), 8, KEY, STREAM, masked.data_ptr(), mask.data_ptr(),
                               first=2**64 - 8, mask32=mask32)
    torch.cuda.synchronize()
    assert mask.cpu().numpy().tolist() == DM.draws(KEY, STREAM, 2**64 - 8, 8, 433).tolist()
    # a NULL handle
    k = (C.c_uint32 * 8)(*KEY)
    fn = engine.lib.sda_full_mask_keyed32_dev if mask32 else engine.lib.sda_full_mask_keyed_dev
    assert fn(None, 433, None, 0, k, 0, 0, None, None, None) == INV
