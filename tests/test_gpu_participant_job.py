"""GPU: the participant job (sda_participant_job_dev, sda_participant_job): keyed Full mask, mask payload, shares and
every clerk payload in one call.

For every case, over guarded buffers compared whole:
  (a) the device form equals the existing sequence sda_draws_dev (the Full mask) + sda_participant_share_keyed_dev +
      sda_varint_encode_dev of the mask, byte for byte;
  (b) the host form equals the device form under SDA_PARTICIPANT_TILE_BATCHES unset, 1, 2, 3 and 2049;
  (c) the round trip through the oracle: every payload decoded, the shares reconstructed, the decoded mask taken off,
      gives secrets % m made positive;
and the record of sda_participant_job_last_launch is what the case's schemes and tiling say.

The matrix is a covering one, not the full product (which would take minutes): every scheme meets every dimension
(masking kind and mode rotating with the pair), and every scheme meets every masking kind and both modes at the
dimension k + 1 (two batches, the second ragged).  Every case runs all five tilings (up to 6149 tiles of one batch).
The workspace scheme (242 clerks) costs the oracle 5 ms per batch to reconstruct from all clerks, so
above 8 batches its round trip reconstructs from the first 27 clerks; every clerk's payload is still decoded and
compared in (a).
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from sda_amd import SdaError, schemes as S
from sda_amd import engine as E
from tests import draws_model as DM
from tests import pipeline_matrix_cases as PC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEY = DM.TEST_KEY
MASK_STREAM, SHARE_STREAM = 0x5DA, 0x5DB
GUARD = 16
POISON8 = 0xA5
M32 = 2147482801                             # int32 Additive rows
MBIG = 68719676673                           # above 2^31: i64 Additive rows (a fast-path ChaCha modulus)
EXACT, CANONICAL = E.REVEAL_EXACT, E.REVEAL_CANONICAL
TILE_ENV = "SDA_PARTICIPANT_TILE_BATCHES"

SCHEMES = {"fl": S.FULL_LOOP_PACKED, "cp": S.CONFIG_PACKED, "wide": PC.wide_scheme()}
for _n in (1, 2, 3):
    SCHEMES[f"add{_n}"] = S.Additive(_n, M32)
    SCHEMES[f"add{_n}big"] = S.Additive(_n, MBIG)
MASKINGS = ("none", "full", "chacha0", "chacha1", "chacha8", "chacha9")


def _packed(ss):
    return isinstance(ss, S.PackedShamir)


def _k(ss):
    return ss.secret_count if _packed(ss) else 1


def _dims(ss):
    k = _k(ss)
    return (0, 1, k - 1, k, k + 1, 2049, 3 * 2048 * k + 5)


def _masking(kind, m, d):
    if kind == "none":
        return S.NoMasking()
    if kind == "full":
        return S.FullMasking(m)
    return S.ChaChaMasking(m, d, 32 * int(kind[6:]))


def _cases():
    out = []
    for si, (name, ss) in enumerate(SCHEMES.items()):
        for di, d in enumerate(_dims(ss)):
            out.append((name, MASKINGS[(si + di) % len(MASKINGS)], d, (si + di) % 2 if _packed(ss) else EXACT))
        for mk in MASKINGS:
            for mode in ((EXACT, CANONICAL) if _packed(ss) else (EXACT,)):
                out.append((name, mk, _k(ss) + 1, mode))
    return sorted(set(out))


CASES = _cases()


def _secrets(case_id, m, d):
    rng = np.random.default_rng(zlib.crc32(case_id.encode()))
    return rng.integers(-(m - 1), m, size=d, dtype=np.int64)


def _seed(ms, case_id):
    if not isinstance(ms, S.ChaChaMasking):
        return None
    rng = np.random.default_rng(zlib.crc32(case_id.encode()) + 1)
    return [int(x) for x in rng.integers(0, 2**32, size=ms.seed_words(), dtype=np.uint64)]


def _guarded_u8(cap):
    return torch.full((cap + 2 * GUARD,), POISON8, dtype=torch.uint8, device="cuda")


def _whole(blob, cap):
    """The guarded buffer a call that wrote `blob` into a poisoned buffer of `cap` bytes leaves."""
    full = np.full(cap + 2 * GUARD, POISON8, dtype=np.uint8)
    full[GUARD:GUARD + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return full


def _existing(engine, ms, ss, sec, d, seed, mode):
    """(clerk payloads, mask payload) of the sequence the job replaces."""
    n = ss.output_size()
    B = (d + _k(ss) - 1) // _k(ss)
    full = None
    mask_payload = b""
    if isinstance(ms, S.FullMasking):
        full = torch.zeros(max(d, 1), dtype=torch.int64, device="cuda")
        engine.draws_dev(KEY, MASK_STREAM, 0, d, ms.modulus, full.data_ptr())
        dst = torch.zeros(d * 10 + 32, dtype=torch.uint8, device="cuda")
        rb = engine.varint_encode_dev(full.data_ptr(), 1, d, d, dst.data_ptr(), dst.numel())
        torch.cuda.synchronize()
        mask_payload = dst.cpu().numpy()[:int(rb[0])].tobytes()
    elif isinstance(ms, S.ChaChaMasking):
        mask_payload = engine.varint_encode(np.asarray(seed, dtype=np.int64)) if seed else b""
    sh = torch.zeros(max(n * B, 1), dtype=torch.int64, device="cuda")
    cap = n * B * 10 + 32
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    rb = engine.participant_share_keyed_dev(ms, ss, sec.data_ptr() if d else None, d, KEY, SHARE_STREAM, sh.data_ptr(),
                                            seed=seed, full_masks_ptr=full.data_ptr() if full is not None else None,
                                            payload_ptr=pay.data_ptr(), payload_cap=cap, mode=mode)
    torch.cuda.synchronize()
    host = pay.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(rb)]).astype(np.int64)
    return [host[off[c]:off[c + 1]].tobytes() for c in range(n)], mask_payload


def _job_dev(engine, ms, ss, sec, d, seed, mode, key=KEY, mask_stream=MASK_STREAM, share_stream=SHARE_STREAM,
             short=(0, 0)):
    """(payload buffer, row bytes, mask buffer, mask length, caps) of the device form, guards included; `short`
    takes bytes off the two capacities (the status tests)."""
    n = ss.output_size()
    row, mb = E.participant_job_payload_bound(ms, ss, d)
    cap, mcap = n * row - short[0], mb - short[1]
    pay, mpay = _guarded_u8(max(cap, 0)), _guarded_u8(max(mcap, 0))
    try:
        rb, mlen = engine.participant_job_dev(ms, ss, sec.data_ptr() if d else None, d, key, mask_stream, share_stream,
                                              pay.data_ptr() + GUARD, cap, mpay.data_ptr() + GUARD, mcap, seed=seed,
                                              mode=mode)
    except SdaError as e:
        torch.cuda.synchronize()
        e.buffers = (pay.cpu().numpy(), mpay.cpu().numpy())
        raise
    torch.cuda.synchronize()
    return pay.cpu().numpy(), rb, mpay.cpu().numpy(), mlen, (cap, mcap)


def _job_host(engine, ms, ss, secrets, seed, mode, key=KEY, mask_stream=MASK_STREAM, share_stream=SHARE_STREAM,
              short=(0, 0)):
    """(clerk buffers, clerk lengths, mask buffer, mask length, caps) of the host form, guards included."""
    n = ss.output_size()
    sec = np.ascontiguousarray(secrets, dtype=np.int64)
    row, mb = E.participant_job_payload_bound(ms, ss, sec.size)
    cap, mcap = row - short[0], mb - short[1]
    bufs = [np.full(max(cap, 0) + 2 * GUARD, POISON8, dtype=np.uint8) for _ in range(n)]
    mbuf = np.full(max(mcap, 0) + 2 * GUARD, POISON8, dtype=np.uint8)
    ptrs = (C.POINTER(C.c_uint8) * max(n, 1))(*[C.cast(b.ctypes.data + GUARD, C.POINTER(C.c_uint8)) for b in bufs])
    caps = (C.c_uint64 * max(n, 1))(*[cap] * n)
    lens = (C.c_uint64 * max(n, 1))()
    mlen = C.c_uint64(0)
    sd = np.asarray(seed if seed is not None else [], dtype=np.uint32)
    k = (C.c_uint32 * 8)(*key)
    msc, ssc = ms.c(), ss.c()
    st = engine.lib.sda_participant_job(engine.h, C.byref(msc), sd.ctypes.data_as(C.POINTER(C.c_uint32)), sd.size,
                                        C.byref(ssc), sec.ctypes.data_as(C.POINTER(C.c_int64)), sec.size, k, mask_stream,
                                        share_stream, mode, ptrs, caps, lens,
                                        C.cast(mbuf.ctypes.data + GUARD, C.POINTER(C.c_uint8)), mcap, C.byref(mlen))
    return st, bufs, [int(x) for x in lens[:n]], mbuf, int(mlen.value), (cap, mcap)


TILINGS = (None, 1, 2, 3, 2049)


def _route(ms, ss):
    mask = (E.PARTICIPANT_JOB_MASK_NONE if isinstance(ms, S.NoMasking) else
            E.PARTICIPANT_JOB_MASK_CHACHA if isinstance(ms, S.ChaChaMasking) else
            E.PARTICIPANT_JOB_MASK_FULL32 if ms.modulus <= 2**31 else E.PARTICIPANT_JOB_MASK_FULL64)
    share = E.PARTICIPANT_SHARE_PACKED_KEYED if _packed(ss) else E.PARTICIPANT_SHARE_ADDITIVE_KEYED
    return mask, share, 4 if _packed(ss) or ss.modulus <= 2**31 else 8


@pytest.mark.parametrize("name,mk,d,mode", CASES, ids=[f"{n}-{k}-D{d}-{'canon' if m else 'exact'}"
                                                      for n, k, d, m in CASES])
def test_job_forms_existing_sequence_and_round_trip(engine, oracle, monkeypatch, name, mk, d, mode):
    ss = SCHEMES[name]
    m = ss.modulus
    case_id = f"{name}-{mk}-{d}-{mode}"
    ms = _masking(mk, m, d)
    seed = _seed(ms, case_id)
    secrets = _secrets(case_id, m, d)
    sec = torch.as_tensor(secrets).cuda() if d else None
    n = ss.output_size()
    monkeypatch.delenv(TILE_ENV, raising=False)
    before = engine.participant_job_last_launch()

    # (a) the device form against the existing sequence
    want_rows, want_mask = _existing(engine, ms, ss, sec, d, seed, mode)
    pay, rb, mpay, mlen, (cap, mcap) = _job_dev(engine, ms, ss, sec, d, seed, mode)
    assert [int(x) for x in rb] == [len(r) for r in want_rows] and mlen == len(want_mask)
    assert np.array_equal(pay, _whole(b"".join(want_rows), cap)), "clerk payloads"
    assert np.array_equal(mpay, _whole(want_mask, mcap)), "mask payload"
    rec = engine.participant_job_last_launch()
    assert rec == (E.ParticipantJobLaunch(*_route(ms, ss), 1) if d else before)
    if d and isinstance(ms, S.FullMasking):
        assert engine.participant_last_launch().mask_route == E.PARTICIPANT_MASK_FULL_KEYED

    # (b) the host form under every tiling
    row_cap = cap // n
    for tile in TILINGS:
        if tile is None:
            monkeypatch.delenv(TILE_ENV, raising=False)
        else:
            monkeypatch.setenv(TILE_ENV, str(tile))
        st, bufs, lens, mbuf, hmlen, _ = _job_host(engine, ms, ss, secrets, seed, mode)
        assert st == E.OK, (tile, E.load_library().sda_last_error_message())
        assert lens == [len(r) for r in want_rows] and hmlen == len(want_mask), tile
        for c in range(n):
            assert np.array_equal(bufs[c], _whole(want_rows[c], row_cap)), (tile, c)
        assert np.array_equal(mbuf, _whole(want_mask, mcap)), tile
        if d:
            units = (d + _k(ss) - 1) // _k(ss)
            tiles = 1 if tile is None else (units + min(tile, units) - 1) // min(tile, units)
            assert engine.participant_job_last_launch() == E.ParticipantJobLaunch(*_route(ms, ss), tiles), tile
    monkeypatch.delenv(TILE_ENV, raising=False)

    # (c) the round trip through the oracle
    if d == 0:
        return
    rows = np.stack([oracle.varint_decode(r) for r in want_rows])
    if _packed(ss):
        B = (d + _k(ss) - 1) // _k(ss)
        assert rows.shape == (n, B)
        pp = oracle.packed_params(ss.secret_count, n, ss.privacy_threshold(), m, ss.omega_secrets, ss.omega_shares)
        idx = list(range(n if n <= 26 or B <= 8 else 27))
        rc, masked = oracle.packed_reconstruct(pp, d, idx, rows[idx])
        assert rc == 0
    else:
        assert rows.shape == (n, d)
        masked = oracle.combine(m, rows)                     # additive.rs:56-70
    mask = oracle.varint_decode(want_mask)
    if isinstance(ms, S.FullMasking):
        assert mask.size == d and 0 <= mask.min() and mask.max() < m
        masked = oracle.unmask(m, mask, masked)
    elif isinstance(ms, S.ChaChaMasking):
        assert mask.tolist() == seed
        masked = oracle.unmask(m, oracle.chacha_mask_combine(m, d, mask.reshape(1, -1)), masked)
    else:
        assert mask.size == 0
    assert np.array_equal(oracle.positive(m, masked), secrets % m)


# ---------------------------------------------------------------------------------------------------------------
# the status matrix: a failing call leaves buffers and records as they were
# ---------------------------------------------------------------------------------------------------------------
def _records(engine):
    """every *_last_launch record of the handle"""
    return (engine.participant_job_last_launch(), engine.participant_last_launch(), engine.chacha_last_launch(),
            engine.packed_keyed_last_launch(), engine.codec_last_launch(), tuple(engine.combine_last_launch()),
            engine.snapshot_last_launch(), engine.clerk_job_last_launch(), tuple(engine.recipient_last_launch()),
            tuple(engine.recipient_job_last_launch()))


def _untouched(bufs):
    return all((np.asarray(b) == POISON8).all() for b in bufs)


def _refused_both(engine, status, text, ms, ss, d=8, seed=None, mode=EXACT, lens_are_bounds=False, **kw):
    secrets = np.arange(d, dtype=np.int64)
    sec = torch.as_tensor(secrets).cuda() if d else None
    before = _records(engine)
    with pytest.raises(SdaError) as ei:
        _job_dev(engine, ms, ss, sec, d, seed, mode, **kw)
    assert ei.value.status == status and text in str(ei.value), str(ei.value)
    assert _untouched(ei.value.buffers) and _records(engine) == before
    row, mb = E.participant_job_payload_bound(ms, ss, d) if lens_are_bounds else (0, 0)
    if lens_are_bounds:
        assert [int(x) for x in ei.value.row_bytes] == [row] * ss.output_size() and ei.value.mask_len == mb
    st, bufs, lens, mbuf, mlen, _ = _job_host(engine, ms, ss, secrets, seed, mode, **kw)
    msg = E.load_library().sda_last_error_message().decode()
    assert st == status and text in msg, msg
    assert _untouched(bufs + [mbuf]) and _records(engine) == before
    if lens_are_bounds:
        assert lens == [row] * ss.output_size() and mlen == mb


def test_status_matrix(engine, monkeypatch):
    monkeypatch.delenv(TILE_ENV, raising=False)
    INV, PRE = E.ERR_INVALID_ARGUMENT, E.ERR_PRECONDITION
    add, cp = S.Additive(2, 433), S.CONFIG_PACKED
    full, none = S.FullMasking(433), S.NoMasking()
    seed4 = [1, 2, 3, 4]
    # a successful call first: the records every refusal has to leave
    sec = torch.arange(8, dtype=torch.int64, device="cuda")
    _job_dev(engine, S.ChaChaMasking(2147482801, 8, 128), cp, sec, 8, seed4, EXACT)
    assert engine.participant_job_last_launch().mask_route == E.PARTICIPANT_JOB_MASK_CHACHA
    # equal stream ids under Full masking (the key contract); without a mask nothing shares the stream
    _refused_both(engine, INV, "must differ", full, add, mask_stream=7, share_stream=7)
    _job_dev(engine, none, add, sec, 8, None, EXACT, mask_stream=7, share_stream=7)
    # capacities below the bound: refused before any work, the lengths set to the bounds
    _refused_both(engine, INV, "below the bound", full, add, short=(1, 0), lens_are_bounds=True)
    _refused_both(engine, INV, "below the bound", full, cp, short=(0, 1), lens_are_bounds=True)
    _refused_both(engine, INV, "below the bound", S.ChaChaMasking(433, 8, 128), add, seed=seed4, short=(0, 1),
                  lens_are_bounds=True)
    # modulus <= 0: gen_range's panic, for the mask and for the Additive draws
    for bad in (0, -433):
        _refused_both(engine, PRE, "Rng.gen_range called with low >= high", S.FullMasking(bad), add)
        _refused_both(engine, PRE, "Rng.gen_range called with low >= high", S.ChaChaMasking(bad, 8, 128), add,
                      seed=seed4)
        _refused_both(engine, PRE, "Rng.gen_range called with low >= high", none, S.Additive(2, bad))
    # chacha.rs:26: dimension == secrets.len(), for an empty vector too; the seed's word count
    _refused_both(engine, PRE, "dimension == secrets.len()", S.ChaChaMasking(433, 9, 128), add, seed=seed4)
    _refused_both(engine, PRE, "dimension == secrets.len()", S.ChaChaMasking(433, 9, 128), add, d=0, seed=seed4)
    _refused_both(engine, PRE, "seed words", S.ChaChaMasking(433, 8, 128), add, seed=seed4[:3])
    _refused_both(engine, PRE, "seed words", S.ChaChaMasking(433, 0, 160), add, d=0, seed=seed4)
    # scheme checks of the reused pipeline
    _refused_both(engine, INV, "bad mode", none, cp, mode=7)
    _refused_both(engine, PRE, "share_count - 1 underflows", none, S.Additive(0, 433))
    # NULLs
    lib = engine.lib
    k = (C.c_uint32 * 8)(*KEY)
    msc, ssc = full.c(), add.c()
    rb, mlen = (C.c_uint64 * 2)(), C.c_uint64()
    pay, mpay = _guarded_u8(64), _guarded_u8(64)
    before = _records(engine)

    def dev(h=engine.h, ms=C.byref(msc), ss=C.byref(ssc), secrets=sec.data_ptr(), key=k, rows=rb, payload=True,
            mask=True, mask_len=C.byref(mlen)):
        return lib.sda_participant_job_dev(h, ms, None, 0, ss, secrets, 8, key, 1, 2, EXACT,
                                           pay.data_ptr() + GUARD if payload else None, 64, rows,
                                           mpay.data_ptr() + GUARD if mask else None, 64, mask_len, None)

    for kw in (dict(h=None), dict(ms=None), dict(ss=None), dict(secrets=None), dict(key=None), dict(rows=None),
               dict(payload=False), dict(mask=False), dict(mask_len=None)):
        assert dev(**kw) == INV, kw
        assert b"NULL" in lib.sda_last_error_message()
    torch.cuda.synchronize()
    assert _untouched([pay.cpu().numpy(), mpay.cpu().numpy()]) and _records(engine) == before
    assert dev() == E.OK
    secrets = np.arange(8, dtype=np.int64)
    sp = secrets.ctypes.data_as(C.POINTER(C.c_int64))
    bufs = [np.full(64, POISON8, dtype=np.uint8) for _ in range(2)]
    ptrs = (C.POINTER(C.c_uint8) * 2)(*[C.cast(b.ctypes.data, C.POINTER(C.c_uint8)) for b in bufs])
    nullp = (C.POINTER(C.c_uint8) * 2)(ptrs[0], None)
    caps, lens = (C.c_uint64 * 2)(64, 64), (C.c_uint64 * 2)()
    mbuf = np.full(64, POISON8, dtype=np.uint8)
    mp = C.cast(mbuf.ctypes.data, C.POINTER(C.c_uint8))
    before = _records(engine)

    def host(h=engine.h, ms=C.byref(msc), ss=C.byref(ssc), secrets=sp, key=k, payloads=ptrs, caps=caps, lens=lens,
             mask=mp, mask_len=C.byref(mlen)):
        return lib.sda_participant_job(h, ms, None, 0, ss, secrets, 8, key, 1, 2, EXACT, payloads, caps, lens, mask, 64,
                                       mask_len)

    for kw in (dict(h=None), dict(ms=None), dict(ss=None), dict(secrets=None), dict(key=None), dict(payloads=None),
               dict(payloads=nullp), dict(caps=None), dict(lens=None), dict(mask=None), dict(mask_len=None)):
        assert host(**kw) == INV, kw
        assert b"NULL" in lib.sda_last_error_message()
    assert _untouched(bufs + [mbuf]) and _records(engine) == before
    assert host() == E.OK
    v = [C.c_uint32() for _ in range(3)]
    assert lib.sda_participant_job_last_launch(engine.h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), None) == INV
    assert lib.sda_participant_job_last_launch(None, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(mlen)) == INV


def test_multi_device_handle_runs_on_its_first_device(engine, monkeypatch):
    from sda_amd import Engine
    monkeypatch.setenv(TILE_ENV, "2")
    ss, ms = S.CONFIG_PACKED, S.FullMasking(S.CONFIG_PACKED.prime_modulus)
    secrets = _secrets("multi", ss.prime_modulus, 69)
    want = engine.participant_job(ms, ss, secrets, KEY, MASK_STREAM, SHARE_STREAM)
    multi = Engine(devices=[0, 0])
    try:
        assert multi.participant_job(ms, ss, secrets, KEY, MASK_STREAM, SHARE_STREAM) == want
        assert multi.participant_job_last_launch().tiles == 5
    finally:
        multi.close()
