"""GPU: the clerk's job as one device pipeline (sda_clerk_job_dev, sda_clerk_job, sda_clerk_job_last_launch).

Every case of tests/clerk_job_cases.py runs every split of its blobs into calls -- one call, 1 | rest, rest | 1,
three tiles -- with the payload asked from the last tile and from a trailing n_blobs == 0 finish call, and the
first and last split again under SDA_CODEC_GROUP=3 (read per call).  After each split the whole guarded state
buffer and the whole guarded payload buffer (payload_cap exactly the size needed) are compared with
sda_clerk_decode_combine_dev over all blobs on the same GPU, with oracle.combine and with oracle.varint_encode, and
every call's sda_clerk_job_last_launch and sda_codec_last_launch records are asserted, the expected ones computed
from the bytes (tests/codec_dispatch.py): field moduli must take the device-length encode (route 1), the moduli past
2^31, whose shares leave int32, the host-length one (route 2).  One field case leaves the slot path as well, 433 at
dimension 4097 (clerk_job_cases.takes_slots: 4097 two-byte shares in one region of 4096 slots), and is asserted so.
tests/test_clerk_job_plan.py holds the same tables against the oracle on the CPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import clerk_job_cases as CJ
from tests import codec_dispatch as CD
from tests import codec_matrix_cases as CM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0x5A5A5A5A5A5A5A5A
FILL = 0xA5
PAD = 64                       # guard words in front of and behind the state
CASES = CJ.cases()


def _clear(monkeypatch, **knobs):
    for k in CM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return knobs


def _chunks(n):
    return -(-n // CD.ENC_CHUNK)


def job_record(record, continued, pay, dim, bound):
    """sda_clerk_job_last_launch of a call over blobs whose sda_codec_last_launch record is `record`: the slot path
    encodes by route 1, its grid sized by the host's bound on the dimension (`bound`: blob 0's bytes, or prior_dim),
    every other path by route 2 over the dimension; `pay`: the call asked for the payload"""
    slots = record[0] in (CD.SLOTS, CD.SLOTS_GROUPED)
    route, chunks = ((1, _chunks(bound)) if slots else (2, _chunks(dim))) if pay else (0, 0)
    return (1 if continued else 0, route, chunks)


FINISH_CODEC_RECORD = (CD.NONE, 0, 0, 0)


def finish_record(dim):
    """sda_clerk_job_last_launch of the n_blobs == 0 finish call with a payload"""
    return (1, 2, _chunks(dim))


class Job:
    """blobs on the device, back to back behind 16 bytes of junk, with the host offsets"""

    def __init__(self, blobs):
        self.blobs = list(blobs)
        self.buf, off = CJ.layout(self.blobs)
        self.off = off.astype(np.uint64)
        self.dev = torch.frombuffer(bytearray(self.buf), dtype=torch.uint8).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self):
        return self.dev.data_ptr()

    def tile(self, b0, b1):
        return self.off[b0:b1 + 1]

    def predict(self, b0, b1, m, knobs):
        """the sda_codec_last_launch record of a call over blobs [b0, b1), from the bytes where they lie"""
        return CD.predict(CD.Job(self.buf, self.tile(b0, b1)), m, knobs)[0]


class Guarded:
    """a state of `cap` words and a payload of `pcap` bytes, each between guards, all poisoned"""

    def __init__(self, cap, pcap, lead=0):
        self.cap, self.pcap, self.lead = cap, pcap, PAD + lead
        self.state = torch.full((PAD + cap + PAD,), POISON, dtype=torch.int64, device="cuda")
        self.payload = torch.full((self.lead + pcap + PAD,), FILL, dtype=torch.uint8, device="cuda")

    def state_ptr(self):
        return self.state.data_ptr() + 8 * PAD

    def payload_ptr(self):
        return self.payload.data_ptr() + self.lead

    def host(self):
        torch.cuda.synchronize()
        return self.state.cpu().numpy(), self.payload.cpu().numpy()

    def expect(self, values, payload=b""):
        s = np.full(PAD + self.cap + PAD, POISON, np.int64)
        s[PAD:PAD + len(values)] = values
        p = np.full(self.lead + self.pcap + PAD, FILL, np.uint8)
        p[self.lead:self.lead + len(payload)] = np.frombuffer(payload, np.uint8)
        return s, p


@functools.lru_cache(maxsize=4)
def _case_job(case):
    from oracle import oracle as O
    m, n, dim = case
    x = CJ.rows(m, n, dim)
    want = O.combine(m, x)
    return Job([O.varint_encode(r) for r in x]), want, O.varint_encode(want)


@functools.lru_cache(maxsize=4)
def _one_call_reference(engine, case):
    """sda_clerk_decode_combine_dev over all blobs, on this GPU and with no knob set"""
    job, want, _ = _case_job(case)
    out = torch.full((len(want) + PAD,), POISON, dtype=torch.int64, device="cuda")
    assert engine.clerk_decode_combine_dev(case[0], job.ptr(), job.off, out.data_ptr(), len(want)) == len(want)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[len(want):] == POISON).all()
    return host[:len(want)]


def _run_split(engine, case, split, finish, knobs):
    """the job of `case` in the calls of `split`; the payload from the last tile, or from a finish call"""
    m, n, dim = case
    job, want, want_payload = _case_job(case)
    g = Guarded(dim, len(want_payload), lead=dim % 16)
    b0 = 0
    for i, k in enumerate(split):
        last = i == len(split) - 1
        pay = last and not finish
        got = engine.clerk_job_dev(m, job.ptr(), job.tile(b0, b0 + k), g.state_ptr(), dim,
                                   first_participation=b0, prior_dim=dim if b0 else dim + 5,   # fresh: ignored
                                   payload_ptr=g.payload_ptr() if pay else None,
                                   payload_cap=len(want_payload) if pay else 0)
        assert got == (dim, len(want_payload) if pay else 0), (split, i)
        record = job.predict(b0, b0 + k, m, knobs)
        assert engine.codec_last_launch() == record, (split, i, CD.PATH_NAMES[record[0]])
        slots = record[0] in (CD.SLOTS, CD.SLOTS_GROUPED)
        if len(split) == 1:
            assert slots == CJ.takes_slots(case), record
        assert slots or record[0] == (CD.MATRIX32 if CJ.is_field(m) else CD.MATRIX64), record
        # route 1 sizes its grid by the host's bound on the dimension: blob 0's bytes, or prior_dim
        bound = dim if b0 else len(job.blobs[0])
        assert engine.clerk_job_last_launch() == job_record(record, b0, pay, dim, bound), (split, i)
        b0 += k
    if finish:
        got = engine.clerk_job_dev(m, job.ptr(), [], g.state_ptr(), dim, first_participation=n, prior_dim=dim,
                                   payload_ptr=g.payload_ptr(), payload_cap=len(want_payload))
        assert got == (dim, len(want_payload))
        assert engine.clerk_job_last_launch() == finish_record(dim)
        assert engine.codec_last_launch() == FINISH_CODEC_RECORD
    state, payload = g.host()
    exp_state, exp_payload = g.expect(want, want_payload)
    assert np.array_equal(state[PAD:PAD + dim], _one_call_reference(engine, case)), (split, finish)
    assert np.array_equal(state, exp_state), (split, finish)
    assert np.array_equal(payload, exp_payload), (split, finish)


@pytest.mark.parametrize("case", CASES, ids=CJ.case_id)
def test_every_split_gives_the_one_call_state_and_payload(engine, monkeypatch, case):
    knobs = _clear(monkeypatch)
    _one_call_reference(engine, case)
    for split in CJ.splits(case[1]):
        for finish in (False, True):
            _run_split(engine, case, split, finish, knobs)


@pytest.mark.parametrize("case", [c for c in CASES if CJ.is_field(c[0])], ids=CJ.case_id)
def test_first_and_last_split_grouped(engine, monkeypatch, case):
    """SDA_CODEC_GROUP=3: the first group of a continuing call starts from the state"""
    _clear(monkeypatch)
    _one_call_reference(engine, case)
    knobs = _clear(monkeypatch, SDA_CODEC_GROUP="3")
    sp = CJ.splits(case[1])
    for split in (sp[0], sp[-1]):
        for finish in (False, True):
            _run_split(engine, case, split, finish, knobs)
    if case[1] > 3 and CJ.takes_slots(case):
        assert _case_job(case)[0].predict(0, case[1], case[0], knobs)[0] == CD.SLOTS_GROUPED


# ---------------------------------------------------------------- statuses
N4, D4 = 4, 700


@functools.lru_cache(maxsize=1)
def _small():
    from oracle import oracle as O
    rng = np.random.default_rng(0xC1E4)
    x = rng.integers(-(CJ.M31 - 1), CJ.M31, size=(N4, D4), dtype=np.int64)
    return x, [O.varint_encode(r) for r in x]


def _raises(status, fn, *a, **kw):
    with pytest.raises(E.SdaError) as ei:
        fn(*a, **kw)
    assert ei.value.status == status, str(ei.value)
    return ei.value


def test_null_arguments_and_the_record_getter(engine, monkeypatch):
    _clear(monkeypatch)
    _, blobs = _small()
    job, g = Job(blobs), Guarded(D4, 8 * D4)
    off = job.off
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    dim, plen = C.c_uint64(), C.c_uint64()
    call = engine.lib.sda_clerk_job_dev
    args = [engine.h, CJ.M31, job.ptr(), offp, N4, 0, 0, g.state_ptr(), D4, C.byref(dim), g.payload_ptr(), 8 * D4,
            C.byref(plen), None]
    for i in (0, 2, 3, 9, 12):          # handle, bytes, blob_off, dim_out, payload_len next to a payload
        bad = list(args)
        bad[i] = None
        assert call(*bad) == E.ERR_INVALID_ARGUMENT, i
    no_payload = list(args)
    no_payload[10], no_payload[12] = None, None                     # an intermediate tile: payload_len may be NULL
    assert call(*no_payload) == E.OK and dim.value == D4
    s, p = g.host()
    assert (p == FILL).all() and (s[:PAD] == POISON).all() and (s[PAD + D4:] == POISON).all()
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint64()
    rec = [C.byref(a), C.byref(b), C.byref(c)]
    for i in range(3):
        bad = list(rec)
        bad[i] = None
        assert engine.lib.sda_clerk_job_last_launch(engine.h, *bad) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_clerk_job_last_launch(None, *rec) == E.ERR_INVALID_ARGUMENT
    assert engine.clerk_job_last_launch() == (0, 0, 0)


def test_a_fresh_handle_reports_zeros():
    e = E.Engine(0)
    try:
        assert e.clerk_job_last_launch() == (0, 0, 0)
    finally:
        e.close()


def test_refused_arguments_leave_everything_alone(engine, monkeypatch):
    _clear(monkeypatch)
    x, blobs = _small()
    job, g = Job(blobs), Guarded(D4, 8 * D4)
    before = engine.clerk_job_last_launch()
    e = _raises(E.ERR_INVALID_ARGUMENT, engine.clerk_job_dev, CJ.M31, job.ptr() + 8, job.off, g.state_ptr(), D4,
                payload_ptr=g.payload_ptr(), payload_cap=8 * D4)
    assert "16-byte aligned" in str(e)
    dec = job.off.copy()
    dec[2] = dec[1] - 1
    e = _raises(E.ERR_INVALID_ARGUMENT, engine.clerk_job_dev, CJ.M31, job.ptr(), dec, g.state_ptr(), D4,
                payload_ptr=g.payload_ptr(), payload_cap=8 * D4)
    assert "non-decreasing" in str(e)
    e = _raises(E.ERR_INVALID_ARGUMENT, engine.clerk_job_dev, CJ.M31, job.ptr(), job.tile(1, 2), g.state_ptr(), D4,
                first_participation=1, prior_dim=D4 + 1)
    assert "prior_dim" in str(e)
    s, p = g.host()
    assert (s == POISON).all() and (p == FILL).all()
    assert engine.clerk_job_last_launch() == before
    assert engine.codec_last_launch() == (CD.NONE, 0, 0, 0)


def test_modulus_zero(engine, monkeypatch):
    """`% 0` needs an element: dim 0 passes, dim > 0 fails, fresh and continuing"""
    _clear(monkeypatch)
    _, blobs = _small()
    empty, job, g = Job([b"", b"", b""]), Job(blobs), Guarded(D4, 8 * D4)
    for m in (0, -(2**63)):
        assert engine.clerk_job_dev(m, empty.ptr(), empty.off, g.state_ptr(), D4, payload_ptr=g.payload_ptr(),
                                    payload_cap=8 * D4) == (0, 0)
        assert engine.clerk_job_dev(m, empty.ptr(), empty.tile(1, 3), g.state_ptr(), D4, first_participation=1,
                                    prior_dim=0, payload_ptr=g.payload_ptr(), payload_cap=8 * D4) == (0, 0)
        fresh = _raises(E.ERR_PRECONDITION if m == 0 else E.ERR_UNSUPPORTED, engine.clerk_job_dev, m,
                        job.ptr(), job.off, g.state_ptr(), D4, payload_ptr=g.payload_ptr(), payload_cap=8 * D4)
        with pytest.raises(E.SdaError) as ref:       # as the existing call fails it
            engine.clerk_decode_combine_dev(m, job.ptr(), job.off, g.state_ptr(), D4)
        assert (ref.value.status, str(ref.value)) == (fresh.status, str(fresh))
        # continuing: the modulus fails before any length is looked at (the blobs here are of the wrong dimension)
        cont = _raises(fresh.status, engine.clerk_job_dev, m, job.ptr(), job.tile(1, 4), g.state_ptr(), D4,
                       first_participation=1, prior_dim=D4 - 1)
        assert str(cont) == str(fresh)
    s, p = g.host()
    assert (s == POISON).all() and (p == FILL).all()


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("group", [None, "2"])
def test_a_continuing_tile_of_the_wrong_dimension(engine, oracle, monkeypatch, which, delta, group):
    _clear(monkeypatch, **({"SDA_CODEC_GROUP": group} if group else {}))
    x, blobs = _small()
    i = 0 if which == "first" else N4 - 2
    odd = x[1 + i][:D4 + delta] if delta < 0 else np.concatenate([x[1 + i], [7]])
    tile = list(blobs[1:])
    tile[i] = oracle.varint_encode(odd)
    job, g = Job(tile), Guarded(D4, 8 * D4)
    state0 = oracle.combine(CJ.M31, x[:1])
    g.state[PAD:PAD + D4] = torch.from_numpy(state0).cuda()
    e = _raises(E.ERR_WRONG_DIMENSION, engine.clerk_job_dev, CJ.M31, job.ptr(), job.off, g.state_ptr(), D4,
                first_participation=1, prior_dim=D4, payload_ptr=g.payload_ptr(), payload_cap=8 * D4)
    assert f"participation {1 + i} decodes to {D4 + delta} shares, expected {D4}" in str(e)
    assert (e.dim, e.payload_len) == (D4, 0)
    s, p = g.host()
    exp_s, exp_p = g.expect(state0)
    assert np.array_equal(s, exp_s) and np.array_equal(p, exp_p)
    assert engine.codec_last_launch() == (CD.NONE, 0, 0, 0)


def test_a_fresh_call_reports_row_zero_before_a_later_wrong_dimension(engine, oracle, monkeypatch):
    _clear(monkeypatch)
    x, blobs = _small()
    job, g = Job([blobs[0], oracle.varint_encode(x[1][:-1])]), Guarded(D4, 8 * D4)
    e0 = _raises(E.ERR_PRECONDITION, engine.clerk_job_dev, 0, job.ptr(), job.off, g.state_ptr(), D4)
    assert "Wrong dimension" not in str(e0)
    e = _raises(E.ERR_WRONG_DIMENSION, engine.clerk_job_dev, CJ.M31, job.ptr(), job.off, g.state_ptr(), D4,
                payload_ptr=g.payload_ptr(), payload_cap=8 * D4)
    assert f"participation 1 decodes to {D4 - 1} shares, expected {D4}" in str(e)
    s, p = g.host()
    assert (s == POISON).all() and (p == FILL).all()


@pytest.mark.parametrize("kind", ["irregular", "truncated"])
def test_malformed_blobs_in_a_continuing_tile(engine, oracle, monkeypatch, kind):
    """an 11-byte run of continuation bytes is one element (the sequential decoder); a truncated final varint
    yields its partial value"""
    knobs = _clear(monkeypatch)
    x, blobs = _small()
    tile = list(blobs[1:])
    if kind == "irregular":
        tile[1] = oracle.varint_encode(x[2][:-1]) + bytes([0xFF] * 11)
    else:
        tile[1] = oracle.varint_encode(np.concatenate([x[2][:-1], [2**30]]))[:-1]
        assert tile[1][-1] & 0x80
    rows = np.stack([x[0]] + [oracle.varint_decode(b) for b in tile])
    assert rows.shape == (N4, D4)
    want = oracle.combine(CJ.M31, rows)
    want_payload = oracle.varint_encode(want)
    head, job = Job(blobs[:1]), Job(tile)
    g = Guarded(D4, len(want_payload))
    assert engine.clerk_job_dev(CJ.M31, head.ptr(), head.off, g.state_ptr(), D4) == (D4, 0)
    got = engine.clerk_job_dev(CJ.M31, job.ptr(), job.off, g.state_ptr(), D4, first_participation=1, prior_dim=D4,
                               payload_ptr=g.payload_ptr(), payload_cap=len(want_payload))
    assert got == (D4, len(want_payload))
    record = job.predict(0, len(tile), CJ.M31, knobs)
    assert engine.codec_last_launch() == record
    route = 1 if record[0] == CD.SLOTS else 2
    assert route == (2 if kind == "irregular" else 1)
    assert (kind == "irregular") == bool(record[2] & CD.FB_SEQUENTIAL)
    assert engine.clerk_job_last_launch() == (1, route, _chunks(D4))
    s, p = g.host()
    exp_s, exp_p = g.expect(want, want_payload)
    assert np.array_equal(s, exp_s) and np.array_equal(p, exp_p)


@pytest.mark.parametrize("m", [CJ.M31, 2**62 + 1], ids=["route1", "route2"])
def test_a_payload_buffer_one_byte_short(engine, monkeypatch, m):
    _clear(monkeypatch)
    case = (m, 9, 2049)
    job, want, want_payload = _case_job(case)
    need = len(want_payload)
    g = Guarded(2049, need)
    assert engine.clerk_job_dev(m, job.ptr(), job.tile(0, 4), g.state_ptr(), 2049) == (2049, 0)
    before = engine.clerk_job_last_launch()
    e = _raises(E.ERR_INVALID_ARGUMENT, engine.clerk_job_dev, m, job.ptr(), job.tile(4, 9), g.state_ptr(), 2049,
                first_participation=4, prior_dim=2049, payload_ptr=g.payload_ptr(), payload_cap=need - 1)
    assert (e.dim, e.payload_len) == (2049, need)
    assert engine.clerk_job_last_launch() == before
    s, p = g.host()
    exp_s, exp_p = g.expect(want)
    assert np.array_equal(s, exp_s), "the state is the finished combine"
    assert np.array_equal(p, exp_p), "no payload byte is written"
    assert engine.clerk_job_dev(m, job.ptr(), [], g.state_ptr(), 2049, first_participation=9, prior_dim=2049,
                                payload_ptr=g.payload_ptr(), payload_cap=need) == (2049, need)
    assert engine.clerk_job_last_launch() == (1, 2, _chunks(2049))
    s, p = g.host()
    exp_s, exp_p = g.expect(want, want_payload)
    assert np.array_equal(s, exp_s) and np.array_equal(p, exp_p)


def test_fused_is_not_taken_by_a_continuing_call(engine, monkeypatch):
    _clear(monkeypatch)
    case = (CJ.M31, 9, 2049)
    job, want, want_payload = _case_job(case)
    g = Guarded(2049, len(want_payload))
    _clear(monkeypatch, SDA_CODEC_PATH="fused")
    assert engine.clerk_job_dev(CJ.M31, job.ptr(), job.tile(0, 4), g.state_ptr(), 2049) == (2049, 0)
    assert engine.codec_last_launch()[0] == CD.FUSED            # a fresh call still takes it
    assert engine.clerk_job_last_launch() == (0, 0, 0)
    got = engine.clerk_job_dev(CJ.M31, job.ptr(), job.tile(4, 9), g.state_ptr(), 2049, first_participation=4,
                               prior_dim=2049, payload_ptr=g.payload_ptr(), payload_cap=len(want_payload))
    assert got == (2049, len(want_payload))
    assert engine.codec_last_launch() == (CD.MATRIX32, 0, 0, 1)
    assert engine.clerk_job_last_launch() == (1, 2, _chunks(2049))
    assert engine.combine_last_launch().variant & E.COMBINE_ACC
    s, p = g.host()
    exp_s, exp_p = g.expect(want, want_payload)
    assert np.array_equal(s, exp_s) and np.array_equal(p, exp_p)


# ---------------------------------------------------------------- the host form
@pytest.mark.parametrize("n,dim,stage_mb", [(9, 2049, None), (3, 100_000, "1")], ids=["one-group", "two-groups"])
def test_host_form(engine, oracle, monkeypatch, n, dim, stage_mb):
    """sda_clerk_job: the payload of the device form and the oracle, the out of sda_clerk_decode_combine; the
    second size spans two streamed groups (SDA_HOST_STAGE_MB=1: 3 blobs of about 490 KB)"""
    _clear(monkeypatch)
    if stage_mb:
        monkeypatch.setenv("SDA_HOST_STAGE_MB", stage_mb)
    rng = np.random.default_rng([n, dim])
    x = rng.integers(-(CJ.M31 - 1), CJ.M31, size=(n, dim), dtype=np.int64)
    blobs = [oracle.varint_encode(r) for r in x]
    if stage_mb:
        assert len(blobs[0]) + len(blobs[1]) <= 2**20 < sum(len(b) for b in blobs)
    sch = S.Additive(3, CJ.M31)
    want = oracle.combine(CJ.M31, x)
    want_payload = oracle.varint_encode(want)
    out, payload = engine.clerk_job(sch, blobs)
    assert engine.clerk_job_last_launch() == (0, 2, _chunks(dim))
    assert engine.codec_last_launch() == (CD.NONE, 0, 0, 0)
    assert np.array_equal(out, engine.clerk_decode_combine(sch, blobs)) and np.array_equal(out, want)
    assert payload == want_payload
    none, payload2 = engine.clerk_job(sch, blobs, want_out=False)         # out == NULL
    assert none is None and payload2 == want_payload
    job, g = Job(blobs), Guarded(dim, len(want_payload))
    assert engine.clerk_job_dev(CJ.M31, job.ptr(), job.off, g.state_ptr(), dim, payload_ptr=g.payload_ptr(),
                                payload_cap=len(want_payload)) == (dim, len(want_payload))
    _, p = g.host()
    assert p[g.lead:g.lead + len(want_payload)].tobytes() == payload
    e = _raises(E.ERR_INVALID_ARGUMENT, engine.clerk_job, sch, blobs, payload_cap=len(want_payload) - 1)
    assert e.payload_len == len(want_payload)
    ragged = blobs[:-1] + [oracle.varint_encode(x[-1][:-1])]
    e = _raises(E.ERR_WRONG_DIMENSION, engine.clerk_job, sch, ragged)
    with pytest.raises(E.SdaError) as ref:
        engine.clerk_decode_combine(sch, ragged)
    assert str(e) == str(ref.value)
