"""GPU: Additive share generation with in-kernel draws (sda_additive_generate_keyed_dev and its int32 form), the keyed
participant pipelines built on it, and the int32 Additive chain they open.

Every expected share comes from the CPU (tests/test_additive_keyed_model.py: the oracle's additive_generate over the
draws model), never from the engine; the pipeline tests compare the keyed calls with the unkeyed ones fed with
sda_draws_dev's draws, which tests/test_gpu_draws.py holds to the same model.  T = ADDITIVE_KEYED_TILE columns per
workgroup: dimensions stand on both sides of it.
"""
import ctypes as C

import numpy as np
import pytest

from sda_amd import Engine, SdaError, schemes as S
from sda_amd import engine as E
from tests import draws_model as DM
from tests import test_additive_keyed_model as AM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEY, STREAM, T = AM.KEY, AM.STREAM, AM.T
SENT64, SENT32 = -0x5DA5DA5DA5DA5DA, -0x5DA5DA5
PAD = 3                                                    # out_stride = dimension + PAD


def _device(a, dtype=torch.int64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _generate(engine, m, n, secrets, first=0, narrow=False, key=KEY, stream_id=STREAM):
    """The whole [n][dimension + PAD] out buffer of one call, pre-filled with a sentinel."""
    d = len(secrets)
    sec = _device(np.asarray(secrets, dtype=np.int64))
    out = torch.full((max(n, 1), d + PAD), SENT32 if narrow else SENT64,
                     dtype=torch.int32 if narrow else torch.int64, device="cuda")
    call = engine.additive_generate_keyed32_dev if narrow else engine.additive_generate_keyed_dev
    call(m, n, sec.data_ptr() if d else None, d, key, stream_id, out.data_ptr(), d + PAD, first_column=first)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(m, n, secrets, first=0, narrow=False):
    """The same buffer from the CPU model: the shares, then PAD sentinels per row."""
    d = len(secrets)
    full = np.full((n, d + PAD), SENT32 if narrow else SENT64, dtype=np.int64)
    full[:, :d] = AM.expected(m, n, secrets, first_column=first)
    return full.astype(np.int32) if narrow else full


def _dims(n):
    """The larger share counts stop at T + 1 columns (the CPU model costs a millisecond per block of 8 draws)."""
    return [0, 1, T - 1, T, T + 1] + ([2 * T + 5] if n <= 4 else [])


@pytest.mark.parametrize("m", [AM.M_SMALL, AM.M_PRIME])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 10, 17, 26])
def test_kernel_matrix(engine, n, m):
    for d in _dims(n):
        secrets = AM.matrix_secrets(m, d, 100 * n + d)
        want = _want(m, n, secrets)
        got = _generate(engine, m, n, secrets)
        assert np.array_equal(got, want), (n, m, d)
        got32 = _generate(engine, m, n, secrets, narrow=True)
        assert got32.dtype == np.int32 and np.array_equal(got32, _want(m, n, secrets, narrow=True)), (n, m, d, "int32")
        if d and n > 1:
            assert np.array_equal(got32[:, :d], got[:, :d].astype(np.int32))
            assert 0 <= got[:n - 1, :d].min() and got[:n - 1, :d].max() < m and np.abs(got[n - 1, :d]).max() < m


@pytest.mark.parametrize("n", [3, 4, 10])
def test_first_column_is_a_column_slice(engine, n):
    """A call that starts at first_column gives the matching columns of the whole job: the first block, the last
    block or both are partial (AM.test_first_column_cases_cover_partial_blocks_at_both_ends), and a slice wider
    than T cuts a block between two workgroups.  This is what the multi-device split relies on."""
    for m in (AM.M_SMALL, AM.M_PRIME):
        secrets = AM.matrix_secrets(m, AM.FIRST_TOTAL, n)
        whole = _generate(engine, m, n, secrets)[:, :AM.FIRST_TOTAL]
        assert np.array_equal(whole, AM.expected(m, n, secrets)), (n, m)
        for nn, f, w in AM.FIRST_CASES:
            if nn != n:
                continue
            for narrow in (False, True):
                got = _generate(engine, m, n, secrets[f:f + w], first=f, narrow=narrow)
                assert np.array_equal(got[:, :w], whole[:, f:f + w].astype(got.dtype)), (n, m, f, w, narrow)
                assert (got[:, w:] == (SENT32 if narrow else SENT64)).all(), (n, m, f, w, narrow)


@pytest.mark.parametrize("m,n", AM.RETRY_CASES, ids=[f"{'quarter' if m == DM.BOUND_QUARTER else 'third'}-n{n}"
                                                     for m, n in AM.RETRY_CASES])
def test_retried_draws_and_the_wrapping_fold(engine, m, n):
    """Bounds above 2^62: about one draw in four / three is retried (AM checks that), and last - x wraps."""
    secrets = np.random.default_rng(n).integers(-(m - 1), m, size=AM.RETRY_COLUMNS, dtype=np.int64)
    want = _want(m, n, secrets)
    assert (want[n - 1, :AM.RETRY_COLUMNS] < 0).any() and (want[n - 1, :AM.RETRY_COLUMNS] > 0).any()
    assert np.array_equal(_generate(engine, m, n, secrets), want)


def test_fold_order(engine):
    m, n = AM.M_SMALL, 3
    secrets = np.full(64, 5 * m + 3, dtype=np.int64)
    assert np.array_equal(_generate(engine, m, n, secrets), _want(m, n, secrets))


# ---------------------------------------------------------------------------------------------------------------
# the status matrix of the header, in its order; a refused call writes nothing
# ---------------------------------------------------------------------------------------------------------------
def _refused(engine, narrow, status, text, m=AM.M_SMALL, n=3, d=8, key=KEY, first=0, stride=None, no_secrets=False,
             no_out=False):
    sec = _device(np.arange(max(d, 1), dtype=np.int64))
    out = torch.full((4, d + PAD), SENT32 if narrow else SENT64, dtype=torch.int32 if narrow else torch.int64,
                     device="cuda")
    call = engine.additive_generate_keyed32_dev if narrow else engine.additive_generate_keyed_dev
    with pytest.raises(SdaError) as ei:
        call(m, n, None if no_secrets else sec.data_ptr(), d, key, STREAM, None if no_out else out.data_ptr(),
             d + PAD if stride is None else stride, first_column=first)
    torch.cuda.synchronize()
    assert ei.value.status == status and text in str(ei.value), str(ei.value)
    assert (out == (SENT32 if narrow else SENT64)).all()


@pytest.mark.parametrize("narrow", [False, True], ids=["i64", "int32"])
def test_status_matrix(engine, narrow):
    INV, PRE, UNS = E.ERR_INVALID_ARGUMENT, E.ERR_PRECONDITION, E.ERR_UNSUPPORTED
    big = (1 << 31) + 1
    # 1. NULL key / needed buffer (ahead of every later check)
    _refused(engine, narrow, INV, "NULL", key=None, n=0, m=0)
    _refused(engine, narrow, INV, "NULL", no_secrets=True, n=0)
    _refused(engine, narrow, INV, "NULL", no_out=True, m=0)
    # 2. share_count == 0, ahead of the modulus
    _refused(engine, narrow, PRE, "share_count - 1 underflows", n=0, m=0, stride=1)
    # 3. modulus <= 0, ahead of the stride
    for bad in (0, -7):
        _refused(engine, narrow, PRE, "gen_range", m=bad, stride=1)
    # 4. out_stride < dimension, ahead of the wrap
    _refused(engine, narrow, INV, "out_stride", stride=7, first=(1 << 64) - 1)
    # 5. (first_column + dimension) * (share_count - 1) wraps, ahead of the int32 bound
    _refused(engine, narrow, INV, "wraps", first=(1 << 64) - 8, m=big)
    _refused(engine, narrow, INV, "wraps", first=1 << 63, m=big)
    _refused(engine, narrow, INV, "wraps", first=(1 << 64) // 25, n=26)
    # 6. the int32 form's modulus bound, ahead of dimension == 0
    if narrow:
        _refused(engine, narrow, UNS, "2^31", m=big)
        _refused(engine, narrow, UNS, "2^31", m=big, d=0, no_secrets=True, no_out=True)
    # 7. dimension == 0: OK, nothing launched, no buffer needed; share_count 1 never wraps (no draws)
    call = engine.additive_generate_keyed32_dev if narrow else engine.additive_generate_keyed_dev
    call(AM.M_SMALL, 3, None, 0, KEY, STREAM, None, 0)
    # a NULL handle
    k = (C.c_uint32 * 8)(*KEY)
    fn = engine.lib.sda_additive_generate_keyed32_dev if narrow else engine.lib.sda_additive_generate_keyed_dev
    assert fn(None, 433, 3, None, 0, k, 0, 0, None, 0, None) == INV
    secrets = AM.matrix_secrets(AM.M_SMALL, 5, 9)
    assert np.array_equal(_generate(engine, AM.M_SMALL, 1, secrets, first=(1 << 64) - 5, narrow=narrow)[:, :5],
                          secrets.astype(np.int32 if narrow else np.int64).reshape(1, 5))


def test_int32_form_is_accepted_at_two_to_the_31(engine):
    m, n, d = 1 << 31, 3, T + 1
    secrets = AM.matrix_secrets(m, d, 31)
    want = _want(m, n, secrets)
    assert want[:2].max() >= 1 << 30                          # draws in the top half of the range
    assert np.array_equal(_generate(engine, m, n, secrets), want)
    assert np.array_equal(_generate(engine, m, n, secrets, narrow=True), _want(m, n, secrets, narrow=True))
    assert np.array_equal(want.astype(np.int32).astype(np.int64)[:, :d], want[:, :d])   # every share fits


# ---------------------------------------------------------------------------------------------------------------
# pipelines
# ---------------------------------------------------------------------------------------------------------------
D_PIPE = 4099
SHARINGS = {"additive3": S.Additive(3, AM.M_SMALL), "additive26": S.Additive(26, AM.M_PRIME),
            "packed": S.CONFIG_PACKED}
MASK_KINDS = ["none", "full", "chacha"]
SEED = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]


def _masking(kind, m):
    return {"none": S.NoMasking(), "full": S.FullMasking(m), "chacha": S.ChaChaMasking(m, D_PIPE, 128)}[kind]


def _plan(ss, d):
    """(number of share-generation draws, their bound, B) of a participant call"""
    if isinstance(ss, S.Additive):
        return d * (ss.share_count - 1), ss.modulus, d
    B = (d + ss.secret_count - 1) // ss.secret_count
    return B * ss.privacy_threshold(), ss.prime_modulus - 1, B


def _participant(engine, ms, ss, secrets, full, keyed, narrow, stream_id=STREAM):
    """(shares, payload_row_bytes, payload bytes) of one participant call; keyed=False feeds draws_dev's draws."""
    d = secrets.numel()
    n = ss.output_size()
    count, bound, B = _plan(ss, d)
    sh = torch.full((n, B), SENT32 if narrow else SENT64, dtype=torch.int32 if narrow else torch.int64, device="cuda")
    cap = n * B * 10 + 32
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    kw = dict(seed=SEED if isinstance(ms, S.ChaChaMasking) else None,
              full_masks_ptr=full.data_ptr() if full is not None else None, payload_ptr=pay.data_ptr(), payload_cap=cap)
    if keyed:
        call = engine.participant_share32_keyed_dev if narrow else engine.participant_share_keyed_dev
        rb = call(ms, ss, secrets.data_ptr(), d, KEY, stream_id, sh.data_ptr(), **kw)
    else:
        draws = torch.zeros(max(count, 1), dtype=torch.int64, device="cuda")
        engine.draws_dev(KEY, stream_id, 0, count, bound, draws.data_ptr())
        call = engine.participant_share32_dev if narrow else engine.participant_share_dev
        rb = call(ms, ss, secrets.data_ptr(), d, draws.data_ptr(), sh.data_ptr(), **kw)
    torch.cuda.synchronize()
    return sh.cpu().numpy(), rb.tolist(), pay.cpu().numpy()[:int(rb.sum())].tobytes()


@pytest.mark.parametrize("mask", MASK_KINDS)
@pytest.mark.parametrize("name", list(SHARINGS))
def test_keyed_pipelines_equal_the_unkeyed_ones_fed_with_draws_dev(engine, oracle, name, mask):
    ss = SHARINGS[name]
    m = ss.modulus
    ms = _masking(mask, m)
    secrets = _device(np.random.default_rng(7).integers(0, m, size=D_PIPE, dtype=np.int64))
    full = None
    if mask == "full":                                       # the caller's Full mask: draws under another stream_id
        full = torch.zeros(D_PIPE, dtype=torch.int64, device="cuda")
        engine.draws_dev(KEY, STREAM + 1, 0, D_PIPE, m, full.data_ptr())
    want = _participant(engine, ms, ss, secrets, full, keyed=False, narrow=False)
    got = _participant(engine, ms, ss, secrets, full, keyed=True, narrow=False)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    assert (want[0] != SENT64).all() and len(want[2]) > want[0].size
    got32 = _participant(engine, ms, ss, secrets, full, keyed=True, narrow=True)
    assert np.array_equal(got32[0], want[0].astype(np.int32)) and got32[1] == want[1] and got32[2] == want[2]
    if isinstance(ss, S.Additive):
        # the shares themselves, from the CPU: the model's draws of the masked secrets' generate
        masked = secrets.cpu().numpy()
        if mask == "full":
            masked = oracle.full_mask(m, full.cpu().numpy(), masked)
        elif mask == "chacha":
            masked = oracle.chacha_mask(m, np.array(SEED, dtype=np.uint32), masked)
        if ss.share_count == 3:
            assert np.array_equal(got[0], AM.expected(m, 3, masked))
        # the unkeyed int32 call still refuses Additive
        with pytest.raises(SdaError) as ei:
            _participant(engine, ms, ss, secrets, full, keyed=False, narrow=True)
        assert ei.value.status == E.ERR_UNSUPPORTED


def test_keyed_int32_pipeline_refuses_an_additive_modulus_above_two_to_the_31(engine):
    secrets = _device(np.arange(16, dtype=np.int64))
    sh = torch.full((3, 16), SENT32, dtype=torch.int32, device="cuda")
    with pytest.raises(SdaError) as ei:
        engine.participant_share32_keyed_dev(S.NoMasking(), S.Additive(3, (1 << 31) + 1), secrets.data_ptr(), 16, KEY,
                                             STREAM, sh.data_ptr())
    assert ei.value.status == E.ERR_UNSUPPORTED and "2^31" in str(ei.value)
    assert (sh == SENT32).all()
    engine.participant_share32_keyed_dev(S.NoMasking(), S.Additive(3, 1 << 31), secrets.data_ptr(), 16, KEY, STREAM,
                                         sh.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(sh.cpu().numpy(), AM.expected(1 << 31, 3, np.arange(16)).astype(np.int32))


@pytest.mark.parametrize("m", [AM.M_SMALL, AM.M_PRIME])
def test_end_to_end_in_int32(engine, oracle, m):
    """Participants with distinct stream_ids -> int32 rows / payloads -> each clerk's combine on both routes ->
    Additive reconstruct + positive() = the column sums mod m."""
    ss, ms = S.Additive(3, m), S.NoMasking()
    n, d, people = 3, 1500 + 37, 5
    inputs = np.random.default_rng(m % 1000).integers(0, min(m, 1 << 20), size=(people, d), dtype=np.int64)
    rows = torch.zeros((n, people, d), dtype=torch.int32, device="cuda")      # clerk-major
    payloads = []
    for i in range(people):
        sh, rb, pay = _participant(engine, ms, ss, _device(inputs[i]), None, keyed=True, narrow=True,
                                   stream_id=STREAM + i)
        assert sh.dtype == np.int32 and np.abs(sh.astype(np.int64)).max() < m
        rows[:, i, :] = torch.as_tensor(sh).cuda()
        off = np.concatenate([[0], np.cumsum(rb)]).astype(np.int64)
        payloads.append([pay[off[c]:off[c + 1]] for c in range(n)])
    assert not np.array_equal(rows[0, 0].cpu().numpy(), rows[0, 1].cpu().numpy())     # distinct streams
    by_rows = torch.zeros((n, d), dtype=torch.int64, device="cuda")
    by_payload = torch.zeros((n, d), dtype=torch.int64, device="cuda")
    for c in range(n):
        engine.combine32_dev(m, rows[c].data_ptr(), people, d, d, by_rows[c].data_ptr())
        blob = b"".join(payloads[i][c] for i in range(people))
        boff = np.concatenate([[0], np.cumsum([len(payloads[i][c]) for i in range(people)])]).astype(np.uint64)
        src = torch.frombuffer(bytearray(blob + bytes(64)), dtype=torch.uint8).cuda()
        assert engine.clerk_decode_combine_dev(m, src.data_ptr(), boff, by_payload[c].data_ptr(), d) == d
    torch.cuda.synchronize()
    sums = inputs.sum(axis=0) % m
    for clerk_rows in (by_rows.cpu().numpy(), by_payload.cpu().numpy()):
        rec = oracle.positive(m, oracle.combine(m, clerk_rows))                  # additive.rs:56-70 + receive.rs:14-20
        assert np.array_equal(rec, sums)


# ---------------------------------------------------------------------------------------------------------------
# the host call
# ---------------------------------------------------------------------------------------------------------------
def test_share_generate_keyed_host_call(engine):
    sch = S.Additive(26, AM.M_PRIME)
    d = 2 * T + 5
    secrets = AM.matrix_secrets(AM.M_PRIME, d, 26)
    want = AM.expected(AM.M_PRIME, 26, secrets)
    assert np.array_equal(engine.share_generate_keyed(sch, secrets, KEY, STREAM), want)
    multi = Engine(devices=[0, 0, 0])
    try:
        assert np.array_equal(multi.share_generate_keyed(sch, secrets, KEY, STREAM), want)
    finally:
        multi.close()
