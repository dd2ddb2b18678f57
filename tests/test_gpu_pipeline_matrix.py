"""GPU: the two role pipelines of the C ABI (sda_recipient_reveal / _dev, sda_participant_share{,32}{,_keyed}_dev) over
the case tables of tests/pipeline_matrix_cases.py -- steered inputs at the smallest shapes each thing can go wrong at.

Every case compares the whole output buffer (the `_dev` output, the participant's shares and payload sit between guard
words; the slack of an oversized buffer is compared too) with the big-integer model (tests/pipeline_model.py), and
the record the call left (sda_recipient_last_launch / sda_participant_last_launch) with tests/pipeline_dispatch.py.
Payloads are the oracle's varint encoding of the model's shares, byte for byte, with the row byte counts.  A
residue_only case runs a second time under SDA_RECIPIENT_EXACT=1: the record then says exact, the output is identical.
Every status row asserts its status and message, that the output buffer and its guards are untouched, and that the
record is unchanged.  tests/test_pipeline_matrix_plan.py holds the tables on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import packed_dispatch as KD
from tests import pipeline_dispatch as PD
from tests import pipeline_matrix_cases as PC
from tests import pipeline_model as PM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = PC.GUARD
_POISON = {np.dtype(np.int64): PC.POISON, np.dtype(np.int32): PC.POISON32, np.dtype(np.uint8): PC.POISON8}

# message fragments of tests/pipeline_dispatch.py's classes, as the library words them
MESSAGES = {"masks.iter().all": "masks.iter().all", "1..8 words": "1..8 words", "gen_range": "gen_range",
            "divisor of zero": "divisor of zero", "i64::MIN": "i64::MIN", "Mismatching dimension": "Mismatching dimension",
            "mask.len() == dimension": "mask.len() == dimension", "index out of bounds": "index out of bounds",
            "Not enough shares": "Not enough shares", "clerk shares per batch": "clerk shares per batch",
            "bad mode": "bad mode", "mask.len() == masked_secrets.len()": "mask.len() == masked_secrets.len()",
            "output buffer too small": "output buffer too small", "NULL argument": "NULL argument",
            "int32 shares need a PackedShamir scheme": "int32 shares need a PackedShamir scheme",
            "share_count - 1 underflows": "share_count - 1 underflows", "modulus <= 2^31": "modulus <= 2^31",
            "Full masking needs the drawn masks": "Full masking needs the drawn masks",
            "dimension == secrets.len()": "dimension == secrets.len()", "seed words": "seed words",
            "need the randomness draws": "need the randomness draws", "payload_cap": "payload_cap"}


# ---------------------------------------------------------------- guarded buffers
def guarded_host(n, slack, dtype):
    """GUARD poison words, n + slack poisoned body words, GUARD poison words."""
    dtype = np.dtype(dtype)
    return np.full(2 * GUARD + n + slack, _POISON[dtype], dtype=dtype)


def check_guarded(host, want, slack, label):
    """The whole buffer: both guards, every element of `want`, every word of the slack."""
    poison = _POISON[host.dtype]
    n = len(want)
    assert host.size == 2 * GUARD + n + slack, label
    assert (host[:GUARD] == poison).all(), f"{label}: wrote before the buffer"
    assert (host[GUARD + n:] == poison).all(), f"{label}: wrote past the {n} output elements"
    body = host[GUARD:GUARD + n]
    assert np.array_equal(body, np.asarray(want, host.dtype)), \
        f"{label}: {int((body != np.asarray(want, host.dtype)).sum())} of {n} elements differ"


class Guarded:
    def __init__(self, n, slack, dtype=np.int64, device=True):
        self.n, self.slack, self.device = n, slack, device
        self.buf = guarded_host(n, slack, dtype)
        if device:
            self.buf = torch.as_tensor(self.buf).cuda()
        self.ptr = (self.buf.data_ptr() if device else self.buf.ctypes.data) + GUARD * np.dtype(dtype).itemsize

    def host(self):
        if self.device:
            torch.cuda.synchronize()
            return self.buf.cpu().numpy()
        return self.buf

    def check(self, want, label):
        assert len(want) <= self.n + self.slack
        check_guarded(self.host(), want, self.n + self.slack - len(want), label)

    def untouched(self, label):
        self.check([], label)


def _dev(values, dtype=np.int64):
    """A device tensor of the values, never empty (a pointer the library may check against NULL)."""
    a = np.asarray(values, dtype=dtype).reshape(-1)
    if a.size == 0:
        a = np.zeros(1, dtype)
    return torch.as_tensor(a).cuda()


def _message(lib):
    return lib.sda_last_error_message().decode()


# ---------------------------------------------------------------- recipient calls
def _recipient_dev(eng, case, out, null=None):
    """sda_recipient_reveal_dev on the case's uniform rows -> (status, out_len)."""
    masks, indexed = PC.recipient_inputs(case)
    ms, ss = case.ms.c(), case.ss.c()
    if isinstance(case.ms, S.ChaChaMasking):
        width = case.seed_words if case.mask_width is None else case.mask_width
        dm = _dev(np.asarray([w for r in masks for w in r], np.uint64).astype(np.uint32).view(np.int32), np.int32)
    else:
        width = len(masks[0]) if masks else (case.mask_width or 0)
        dm = _dev([v for r in masks for v in r])
    idx = np.asarray([i for i, _ in indexed] or [0], np.uint64)
    share_len = len(indexed[0][1]) if indexed else 0
    dsh = _dev([v for _, r in indexed for v in r])
    olen = C.c_uint64(77)
    st = eng.lib.sda_recipient_reveal_dev(
        eng.h, None if null == "ms" else C.byref(ms), None if null == "masks" else dm.data_ptr(), len(masks), width,
        None if null == "ss" else C.byref(ss), case.dimension, None if null == "indices" else E._ptr(idx, E._u64p),
        None if null == "shares" else dsh.data_ptr(), len(indexed), share_len, case.m_out, case.mode, out.ptr,
        case.D + case.out_slack, None if null == "out_len" else C.byref(olen), None)
    torch.cuda.synchronize()
    return st, olen.value


def _recipient_host(eng, case, out, null=None):
    """sda_recipient_reveal on the case's (possibly ragged) host rows -> (status, out_len)."""
    masks, indexed = PC.host_rows(case)
    ms, ss = case.ms.c(), case.ss.c()
    marrs, mptrs, mlens, nm = E._rows(masks)
    sarrs, sptrs, slens, ns = E._rows([r for _, r in indexed])
    idx = np.asarray([i for i, _ in indexed] or [0], np.uint64)
    olen = C.c_uint64(77)
    st = eng.lib.sda_recipient_reveal(
        eng.h, None if null == "ms" else C.byref(ms), None if null == "masks" else mptrs, mlens, nm,
        None if null == "ss" else C.byref(ss), case.dimension, None if null == "indices" else E._ptr(idx, E._u64p),
        None if null == "shares" else sptrs, slens, ns, case.m_out, case.mode, C.cast(out.ptr, E._i64p),
        case.D + case.out_slack, None if null == "out_len" else C.byref(olen))
    return st, olen.value


def _recipient(eng, case, form, null=None):
    slack = max(case.out_slack, 0)
    out = Guarded(case.D, slack, device=(form == "dev"))
    st, olen = (_recipient_dev if form == "dev" else _recipient_host)(eng, case, out, null)
    return st, olen, out


def _recipient_want(case, form, env_exact=None):
    masks, indexed = PC.host_rows(case) if form == "host" else PC.recipient_inputs(case)
    want = PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, case.mode)
    share_len = min(len(r) for _, r in indexed) if indexed else 0
    record = PD.recipient_record(case.ms, case.ss, case.dimension, [i for i, _ in indexed], share_len, case.m_out,
                                 case.mode, env_exact, late_resolve="late" in case.tags)
    return want, record


def _check_recipient_chacha(eng, case):
    """sda_chacha_last_launch after a recipient call whose mask had seed rows."""
    if not isinstance(case.ms, S.ChaChaMasking) or case.n_masks == 0:
        return
    path, grid_y, fixups = eng.chacha_last_launch()
    if PD.chacha_fast_path(case.ms.modulus):
        assert path in (E.CHACHA_DIRECT, E.CHACHA_CHUNKED, E.CHACHA_STREAM_K) and grid_y >= 1
        assert fixups == (case.n_masks if "late" in case.tags else 0)
    else:
        assert (path, grid_y, fixups) == (E.CHACHA_STREAM, 0, 0)


@pytest.mark.parametrize("case", PC.RECIPIENT_CASES, ids=[c.id for c in PC.RECIPIENT_CASES])
def test_recipient_cases(engine, monkeypatch, case):
    monkeypatch.delenv("SDA_RECIPIENT_EXACT", raising=False)
    monkeypatch.delenv("SDA_CHACHA_PATH", raising=False)
    for form in case.forms:
        want, record = _recipient_want(case, form)
        st, olen, out = _recipient(engine, case, form)
        assert st == E.OK, (form, _message(engine.lib))
        got = tuple(engine.recipient_last_launch())
        print(f"CASE {case.id} {form} record={got}")
        assert olen == case.D
        out.check(want, f"{case.id} {form}")
        assert got == record, form
        _check_recipient_chacha(engine, case)
        if "late" in case.tags:
            assert got[4] == 2
        if PD.has_duplicates(case.subset) and "residue_only" in case.tags:
            assert got[2] == 1
        if "residue_only" in case.tags:
            assert got[1] == PD.REVEAL_EXACT if got[2] else got[1] == PD.REVEAL_CANONICAL
            monkeypatch.setenv("SDA_RECIPIENT_EXACT", "1")
            st, olen, forced = _recipient(engine, case, form)
            monkeypatch.delenv("SDA_RECIPIENT_EXACT")
            assert st == E.OK and olen == case.D
            forced.check(want, f"{case.id} {form} forced exact")
            again = tuple(engine.recipient_last_launch())
            assert again == _recipient_want(case, form, env_exact="1")[1]
            assert again[1] == PD.REVEAL_EXACT and again[2] == 0


@pytest.mark.parametrize("case", PC.RECIPIENT_ZERO, ids=[c.id for c in PC.RECIPIENT_ZERO])
def test_recipient_zero_length(engine, case):
    before = tuple(engine.recipient_last_launch())
    for form in case.forms:
        st, olen, out = _recipient(engine, case, form)
        print(f"CASE {case.id} {form} record={tuple(engine.recipient_last_launch())}")
        assert st == E.OK and olen == 0, (form, _message(engine.lib))
        out.untouched(f"{case.id} {form}")
        assert tuple(engine.recipient_last_launch()) == before


@pytest.mark.parametrize("case", PC.RECIPIENT_STATUS, ids=[c.id for c in PC.RECIPIENT_STATUS])
def test_recipient_status_matrix(engine, case):
    before = tuple(engine.recipient_last_launch())
    for form in case.forms:
        status, cls = PC.recipient_expected_status(case, form)
        st, olen, out = _recipient(engine, case, form, null=case.null)
        message = _message(engine.lib)              # (the getters below clear it)
        print(f"CASE {case.id} {form} status={st} record={tuple(engine.recipient_last_launch())}")
        assert st == status, (form, st, message)
        assert MESSAGES[cls] in message, (form, message)
        if case.null != "out_len":
            assert olen == (77 if case.null else 0)     # a NULL argument is refused before anything is written
        out.untouched(f"{case.id} {form}")
        assert tuple(engine.recipient_last_launch()) == before, form


def _multi_cases():
    """A few host-form cases whose ChaCha mask a multi-device handle combines first: one per group, and one modulus
    of each ChaCha path."""
    able = [c for c in PC.RECIPIENT_CASES if "host" in c.forms and PD.multi_mask(c.ms, c.n_masks)]
    picks = [next(c for c in able if c.group == g) for g in ("kinds", "nmasks", "seeds", "wide")]
    picks += [next(c for c in able if c.ms.modulus == m)
              for m in (PC.CHACHA_FAST, PC.CHACHA_HIGH_REJECTION, PC.CHACHA_ABOVE_2_62)]
    picks.append(next(c for c in able if c.packed and "representative" in c.tags))
    return picks


MULTI_CASES = _multi_cases()
from tests.test_gpu_host_path import multi3  # noqa: E402,F401  (that file's multi-device handle fixture)


def test_recipient_on_a_multi_device_handle(multi3):  # noqa: F811
    """The host form on a handle from sda_engine_create_multi combines the ChaCha mask over its devices first and
    runs the pipeline with the combined row: mask_kind 4, the same output as the single-device handle's
    (test_recipient_cases holds that one to the same model)."""
    multi = multi3
    for case in MULTI_CASES:
        masks, indexed = PC.host_rows(case)
        want = PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, case.mode)
        st, olen, out = _recipient(multi, case, "host")
        assert st == E.OK and olen == case.D, _message(multi.lib)
        out.check(want, f"{case.id} multi")
        record = PD.recipient_record(case.ms, case.ss, case.dimension, case.subset, case.share_len, case.m_out,
                                     case.mode, multi_mask=True)
        got = tuple(multi.recipient_last_launch())
        print(f"CASE {case.id} multi record={got}")
        assert got == record and got[0] == E.RECIPIENT_MASK_COMBINED_ROW
    # no seed row: nothing to split, the pipeline's own ChaCha step runs
    zero = next(c for c in PC.RECIPIENT_CASES if c.id == "nmasks-chacha-0-negative-add-D257")
    st, olen, out = _recipient(multi, zero, "host")
    assert st == E.OK and tuple(multi.recipient_last_launch())[0] == E.RECIPIENT_MASK_CHACHA
    out.check(_recipient_want(zero, "host")[0], "zero rows, multi")


# ---------------------------------------------------------------- participant calls
class _Participant:
    """One call of the case's entry point into guarded share and payload buffers."""

    def __init__(self, eng, case, null=None):
        secrets, seed, full, draws = PC.participant_inputs(case)
        n = case.ss.output_size()
        B = case.B
        self.n, self.B = n, B
        width = np.int32 if case.narrow else np.int64
        self.shares = Guarded(n * B, 0, width)
        self.cap = n * B * 10 + 8
        self.pay = Guarded(self.cap, 0, np.uint8) if case.payload else None
        self.rb = np.full(max(n, 1), 0xEE, np.uint64)
        ms, ss = case.ms.c(), case.ss.c()
        sd = np.asarray(seed if seed is not None else [], np.uint64).astype(np.uint32)
        words = sd.size if case.seed_words is None else case.seed_words
        self.keep = (_dev(secrets), _dev(full if full is not None else []), _dev(draws))
        key = np.asarray(PC.KEY, np.uint32)
        fn = {"dev": eng.lib.sda_participant_share_dev, "dev32": eng.lib.sda_participant_share32_dev,
              "keyed": eng.lib.sda_participant_share_keyed_dev,
              "keyed32": eng.lib.sda_participant_share32_keyed_dev}[case.entry]
        head = (eng.h, C.byref(ms), None if null == "seed" else E._ptr(sd, E._u32p), words,
                None if (full is None or null == "full_masks") else self.keep[1].data_ptr(), C.byref(ss),
                None if null == "secrets" else self.keep[0].data_ptr(), case.D)
        src = ((None if null == "key" else E._ptr(key, E._u32p), PC.STREAM) if case.keyed
               else (None if null == "draws" else self.keep[2].data_ptr(),))
        cap = 0 if case.payload_short else self.cap
        tail = (case.mode, None if null == "shares" else self.shares.ptr, self.pay.ptr if self.pay else None,
                cap if self.pay else 0, None if null == "payload_row_bytes" else E._ptr(self.rb, E._u64p), None)
        self.status = fn(*head, *src, *tail)
        torch.cuda.synchronize()


def _participant_want(case):
    secrets, seed, full, draws = PC.participant_inputs(case)
    _, shares = PM.participant(case.ms, case.ss, secrets, draws, seed=seed, full_masks=full, mode=case.mode)
    flat = np.asarray([v for row in shares for v in row], np.int64)
    if case.narrow:
        flat = flat.astype(np.int32)              # the int32 rows are (int32_t) of the i64 form's
    rows = flat.reshape(len(shares), -1).astype(np.int64) if flat.size else [[] for _ in shares]
    payload, row_bytes = PM.payloads(rows)
    return flat, payload, row_bytes


def _check_participant_launches(eng, case):
    route = PD.mask_route(case.ms)
    if route == PD.ROUTE_CHACHA_FUSED:
        assert eng.chacha_last_launch() == (E.CHACHA_MASK_ADD, 1, 1 if "late" in case.tags else 0)
    elif route == PD.ROUTE_CHACHA_COMBINE_ADD:
        assert eng.chacha_last_launch() == (E.CHACHA_STREAM, 0, 0)
    if case.keyed and PD.is_packed(case.ss):
        ss = case.ss
        in_kernel = ss.share_count + 1 <= 27 and KD.gen_kernel(ss, case.B, 0, case.mode) != "wide"
        staged = 0 if in_kernel else case.B * ss.privacy_threshold() * 8
        assert eng.packed_keyed_last_launch() == (1 if in_kernel else 2, staged)


@pytest.mark.parametrize("case", PC.PARTICIPANT_CASES, ids=[c.id for c in PC.PARTICIPANT_CASES])
def test_participant_cases(engine, monkeypatch, case):
    monkeypatch.delenv("SDA_CHACHA_PATH", raising=False)
    flat, payload, row_bytes = _participant_want(case)
    run = _Participant(engine, case)
    assert run.status == E.OK, _message(engine.lib)
    got = tuple(engine.participant_last_launch())
    print(f"CASE {case.id} record={got}")
    run.shares.check(flat, f"{case.id} shares")
    if case.payload:
        assert run.rb[:run.n].tolist() == row_bytes
        run.pay.check(np.frombuffer(payload, np.uint8), f"{case.id} payload")
    else:
        assert run.rb[:run.n].tolist() == [0xEE] * run.n          # no payload: the row byte counts are not written
    assert got == PD.participant_record(case.ms, case.ss, case.entry, late_resolve="late" in case.tags)
    _check_participant_launches(engine, case)


@pytest.mark.parametrize("case", PC.PARTICIPANT_ZERO, ids=[c.id for c in PC.PARTICIPANT_ZERO])
def test_participant_zero_length(engine, case):
    before = tuple(engine.participant_last_launch())
    run = _Participant(engine, case)
    print(f"CASE {case.id} record={tuple(engine.participant_last_launch())}")
    assert run.status == E.OK, _message(engine.lib)
    run.shares.untouched(f"{case.id} shares")
    run.pay.untouched(f"{case.id} payload")
    assert run.rb[:run.n].tolist() == [0] * run.n
    assert tuple(engine.participant_last_launch()) == before


@pytest.mark.parametrize("case", PC.PARTICIPANT_STATUS, ids=[c.id for c in PC.PARTICIPANT_STATUS])
def test_participant_status_matrix(engine, case):
    before = tuple(engine.participant_last_launch())
    status, cls = PC.participant_expected_status(case)
    run = _Participant(engine, case, null=case.null)
    message = _message(engine.lib)                  # (the getters below clear it)
    print(f"CASE {case.id} status={run.status} record={tuple(engine.participant_last_launch())}")
    assert run.status == status, (run.status, message)
    assert MESSAGES[cls] in message, message
    if not case.payload_short:
        run.shares.untouched(f"{case.id} shares")      # a short payload buffer is found after the shares were made
    run.pay.untouched(f"{case.id} payload")
    assert tuple(engine.participant_last_launch()) == before


# ---------------------------------------------------------------- the records themselves
def test_last_launch_getters(engine):
    """A fresh handle reports zeros; a NULL out-pointer or handle is an invalid argument."""
    fresh = E.Engine(0)
    try:
        assert tuple(fresh.recipient_last_launch()) == (0, 0, 0, 0, 0)
        assert tuple(fresh.participant_last_launch()) == (0, 0, 0)
    finally:
        fresh.close()
    v = [C.c_uint32() for _ in range(5)]
    for i in range(5):
        args = [C.byref(x) for x in v]
        args[i] = None
        assert engine.lib.sda_recipient_last_launch(engine.h, *args) == E.ERR_INVALID_ARGUMENT
    for i in range(3):
        args = [C.byref(x) for x in v[:3]]
        args[i] = None
        assert engine.lib.sda_participant_last_launch(engine.h, *args) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_recipient_last_launch(None, *[C.byref(x) for x in v]) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_participant_last_launch(None, *[C.byref(x) for x in v[:3]]) == E.ERR_INVALID_ARGUMENT


def test_zero_row_chacha_combine_agrees_everywhere(engine):
    """chacha.rs:57-76 with no seed row: `dimension` zeros for any modulus -- the step-wise calls (host and device),
    the pipeline and the model agree; a modulus <= 0 with a row keeps its PRECONDITION."""
    D = 257
    for m in (433, -PC.P, -(2**62 + 1), 0, PD.I64_MIN):
        ms = S.ChaChaMasking(m, D, 128)
        assert PM.mask_combine(ms, []) == [0] * D
        assert engine.mask_combine(ms, []).tolist() == [0] * D
        out = Guarded(D, 0)
        engine.chacha_mask_combine_dev(m, D, None, 4, 0, out.ptr)
        out.check([0] * D, f"m = {m}")
        if m <= 0:
            with pytest.raises(E.SdaError) as ei:
                engine.mask_combine(ms, [[1, 2, 3, 4]])
            assert ei.value.status == E.ERR_PRECONDITION
            seeds = _dev([1, 2, 3, 4], np.int32)
            with pytest.raises(E.SdaError) as ei:
                engine.chacha_mask_combine_dev(m, D, seeds.data_ptr(), 4, 1, out.ptr)
            assert ei.value.status == E.ERR_PRECONDITION
            out.check([0] * D, f"m = {m}, refused")
    multi = E.Engine(devices=[0, 0])
    try:
        assert multi.mask_combine(S.ChaChaMasking(-PC.P, D, 128), []).tolist() == [0] * D
    finally:
        multi.close()


GROUPS = {"test_recipient_cases": PC.RECIPIENT_CASES, "test_recipient_zero_length": PC.RECIPIENT_ZERO,
          "test_recipient_status_matrix": PC.RECIPIENT_STATUS, "test_participant_cases": PC.PARTICIPANT_CASES,
          "test_participant_zero_length": PC.PARTICIPANT_ZERO, "test_participant_status_matrix": PC.PARTICIPANT_STATUS}
