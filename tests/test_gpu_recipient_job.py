"""GPU: the recipient job (sda_recipient_job, sda_recipient_job_dev, sda_recipient_job_last_launch) over the case
tables of tests/recipient_job_cases.py.

The contract: the job returns what sda_recipient_reveal returns on the rows each blob decodes to.  Every case runs
both forms into guarded buffers and compares the whole buffer (guards and slack included) with the big-integer model
on the oracle-decoded rows, and runs sda_recipient_reveal on those rows in the same test (and sda_recipient_reveal_dev
where the rows are uniform enough for it): same status, same message class, same length, same bytes.  The new record
and sda_recipient_last_launch are asserted.  With Full masking the `_dev` form takes the mask that sda_clerk_job_dev
folded from the mask payloads; test_full_mask_folded_in_every_split folds it over every split of the blobs into
calls.  A status row also asserts that the output, its guards, the folded mask and every record are untouched.
tests/test_recipient_job_plan.py holds the tables on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import clerk_job_cases as CJ
from tests import pipeline_dispatch as PD
from tests import recipient_job_cases as RJ
from tests.test_gpu_pipeline_matrix import MESSAGES, Guarded, _dev, _message

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0x5A5A5A5A5A5A5A5A
PAD = 16
JOB_MESSAGES = dict(MESSAGES)
JOB_MESSAGES.update({RJ.ALIGN: "16-byte aligned", RJ.OFFSETS: "non-decreasing", "Wrong dimension": "Wrong dimension"})


def _records(eng):
    """every *_last_launch record of the handle"""
    return (tuple(eng.recipient_job_last_launch()), tuple(eng.recipient_last_launch()), eng.codec_last_launch(),
            tuple(eng.combine_last_launch()), eng.chacha_last_launch(), eng.clerk_job_last_launch(),
            eng.snapshot_last_launch(), tuple(eng.participant_last_launch()), tuple(eng.participant_job_last_launch()),
            eng.packed_keyed_last_launch())


class DevBlobs:
    """blobs on the device, back to back behind LEAD junk bytes, with the host offsets"""

    def __init__(self, blobs):
        buf, off = RJ.layout(list(blobs))
        self.off = off.astype(np.uint64)
        self.dev = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self):
        return self.dev.data_ptr()


class FoldedMask:
    """the Full mask payloads folded by sda_clerk_job_dev in the calls of `split` (blob counts): the state, between
    guards, that sda_recipient_job_dev takes as its mask"""

    def __init__(self, eng, case, split=None):
        mask_blobs, _ = RJ.blobs(case)
        n = len(mask_blobs)
        self.cap = max(len(mask_blobs[0]) if n else 0, 1)           # a value takes a byte at least
        self.state = torch.full((PAD + self.cap + PAD,), POISON, dtype=torch.int64, device="cuda")
        self.ptr = self.state.data_ptr() + 8 * PAD
        self.len = 0
        self.before = self.state.cpu().numpy().copy()
        job = DevBlobs(mask_blobs)
        b0 = 0
        for k in (split or (n,)) if n else ():
            self.len, _ = eng.clerk_job_dev(case.ms.modulus, job.ptr(), job.off[b0:b0 + k + 1], self.ptr, self.cap,
                                            first_participation=b0, prior_dim=self.len)
            b0 += k
        torch.cuda.synchronize()
        self.before = self.state.cpu().numpy().copy()

    def untouched(self):
        torch.cuda.synchronize()
        return np.array_equal(self.state.cpu().numpy(), self.before)


def _job_dev(eng, case, out, mask=None, fault=None):
    """sda_recipient_job_dev -> (status, out_len); `mask`: the FoldedMask of a Full case"""
    mask_blobs, indexed = RJ.blobs(case)
    ms, ss = case.ms.c(), case.ss.c()
    full = isinstance(case.ms, S.FullMasking)
    seeds = DevBlobs([] if full else mask_blobs)
    clerk = DevBlobs([b for _, b in indexed])
    idx = np.asarray([i for i, _ in indexed] or [0], np.uint64)
    soff, coff = seeds.off.copy(), clerk.off.copy()
    if fault == "seed_off-decreasing":
        soff[2] = soff[1] - 1
    if fault == "clerk_off-decreasing":
        coff[2] = coff[1] - 1
    args = {"ms": C.byref(ms), "mask": mask.ptr if mask else None, "seed_bytes": seeds.ptr(),
            "seed_off": E._ptr(soff, E._u64p), "ss": C.byref(ss), "indices": E._ptr(idx, E._u64p),
            "clerk_bytes": clerk.ptr(), "clerk_off": E._ptr(coff, E._u64p)}
    olen = C.c_uint64(77)
    args["out_len"] = C.byref(olen)
    if fault in args:
        args[fault] = None
    if fault in ("seed_bytes+8", "clerk_bytes+8"):
        args[fault[:-2]] += 8
    st = eng.lib.sda_recipient_job_dev(
        eng.h, args["ms"], args["mask"], mask.len if mask else 0, args["seed_bytes"], args["seed_off"],
        0 if full else len(mask_blobs), args["ss"], case.dimension, args["indices"], args["clerk_bytes"],
        args["clerk_off"], len(indexed), case.m_out, case.mode, out.ptr, RJ.out_len(case) + case.out_slack,
        args["out_len"], None)
    torch.cuda.synchronize()
    return st, olen.value


def _job_host(eng, case, out, fault=None):
    """sda_recipient_job -> (status, out_len)"""
    mask_blobs, indexed = RJ.blobs(case)
    ms, ss = case.ms.c(), case.ss.c()
    mbufs, mptrs, mlens, nm = E.Engine._blobs(mask_blobs)
    sbufs, sptrs, slens, ns = E.Engine._blobs([b for _, b in indexed])
    idx = np.asarray([i for i, _ in indexed] or [0], np.uint64)
    if fault == "mask_blob_0":
        mptrs[0] = None
    if fault == "clerk_blob_1":
        sptrs[1] = None
    args = {"ms": C.byref(ms), "mask_blobs": mptrs, "mask_lens": mlens, "ss": C.byref(ss),
            "indices": E._ptr(idx, E._u64p), "clerk_blobs": sptrs, "clerk_lens": slens}
    olen = C.c_uint64(77)
    args["out_len"] = C.byref(olen)
    if fault in args:
        args[fault] = None
    st = eng.lib.sda_recipient_job(eng.h, args["ms"], args["mask_blobs"], args["mask_lens"], nm, args["ss"],
                                   case.dimension, args["indices"], args["clerk_blobs"], args["clerk_lens"], ns,
                                   case.m_out, case.mode, C.cast(out.ptr, E._i64p),
                                   RJ.out_len(case) + case.out_slack, args["out_len"])
    return st, olen.value


def _reveal_host(eng, case, out):
    """sda_recipient_reveal on the decoded rows -> (status, out_len)"""
    masks, indexed = RJ.rows(case)
    ms, ss = case.ms.c(), case.ss.c()
    marrs, mptrs, mlens, nm = E._rows(masks)
    sarrs, sptrs, slens, ns = E._rows([r for _, r in indexed])
    idx = np.asarray([i for i, _ in indexed] or [0], np.uint64)
    olen = C.c_uint64(77)
    st = eng.lib.sda_recipient_reveal(eng.h, C.byref(ms), mptrs, mlens, nm, C.byref(ss), case.dimension,
                                      E._ptr(idx, E._u64p), sptrs, slens, ns, case.m_out, case.mode,
                                      C.cast(out.ptr, E._i64p), RJ.out_len(case) + case.out_slack, C.byref(olen))
    return st, olen.value


def _reveal_dev(eng, case, out):
    """sda_recipient_reveal_dev on the decoded rows, where they are uniform (else None)"""
    masks, indexed = RJ.rows(case)
    if len({len(r) for _, r in indexed}) > 1:
        return None
    if isinstance(case.ms, S.ChaChaMasking):
        if not masks:
            return None
        width = 8
        words = np.zeros((len(masks), 8), np.uint32)
        for i, r in enumerate(masks):
            words[i, :min(len(r), 8)] = [v & 0xFFFFFFFF for v in r[:8]]
        dm = _dev(words.view(np.int32), np.int32)
    else:
        if len({len(r) for r in masks}) > 1:
            return None
        width = len(masks[0]) if masks else 0
        dm = _dev([v for r in masks for v in r])
    idx = np.asarray([i for i, _ in indexed] or [0], np.uint64)
    share_len = len(indexed[0][1]) if indexed else 0
    dsh = _dev([v for _, r in indexed for v in r])
    ms, ss = case.ms.c(), case.ss.c()
    olen = C.c_uint64(77)
    st = eng.lib.sda_recipient_reveal_dev(eng.h, C.byref(ms), dm.data_ptr(), len(masks), width, C.byref(ss),
                                          case.dimension, E._ptr(idx, E._u64p), dsh.data_ptr(), len(indexed),
                                          share_len, case.m_out, case.mode, out.ptr,
                                          RJ.out_len(case) + case.out_slack, C.byref(olen), None)
    torch.cuda.synchronize()
    return st, olen.value


def _out(case, device):
    return Guarded(RJ.out_len(case), max(case.out_slack, 0), device=device)


def _check_ok(eng, case, form, st, olen, out, multi=False):
    assert st == E.OK, (form, _message(eng.lib))
    D = RJ.out_len(case)
    assert olen == D
    out.check(RJ.expected_output(case), f"{case.id} {form}")
    if D:
        job, rec = RJ.expected_records(case, form, multi=multi)
        got = (tuple(eng.recipient_job_last_launch()), tuple(eng.recipient_last_launch()))
        print(f"CASE {case.id} {form} records={got}")
        assert got == (job, rec), form


def _check_status(eng, case, form, want, st, olen, out, before, message):
    status, cls = want
    assert st == status, (form, st, message)
    assert JOB_MESSAGES[cls] in message, (form, message)
    assert olen == 0
    out.untouched(f"{case.id} {form}")
    assert _records(eng) == before, form


@pytest.mark.parametrize("case", RJ.CASES, ids=[c.id for c in RJ.CASES])
def test_recipient_job_cases(engine, monkeypatch, case):
    monkeypatch.delenv("SDA_RECIPIENT_EXACT", raising=False)
    monkeypatch.delenv("SDA_CHACHA_PATH", raising=False)
    want = RJ.expected_status(case)
    full = isinstance(case.ms, S.FullMasking)
    # ---- what a caller does today, on the decoded rows: the job must do the same
    ref = _out(case, device=False)
    rst, rlen = _reveal_host(engine, case, ref)
    rmsg = _message(engine.lib)
    assert rst == (want[0] if want else E.OK), rmsg
    # ---- host form
    before = _records(engine)
    out = _out(case, device=False)
    st, olen = _job_host(engine, case, out)
    message = _message(engine.lib)
    assert (st, olen) == (rst, rlen), (message, rmsg)
    if want is None:
        _check_ok(engine, case, "host", st, olen, out)
        assert np.array_equal(out.host(), ref.host())
    else:
        _check_status(engine, case, "host", want, st, olen, out, before, message)
        assert JOB_MESSAGES[want[1]] in rmsg
    # ---- device form
    mask = None
    if full:
        try:
            mask = FoldedMask(engine, case)
        except E.SdaError as e:
            # the fold's own failures: a modulus the recurrence cannot divide by, and status 3 for full.rs:43
            assert want is not None
            cls = "Wrong dimension" if want[1] == "mask.len() == dimension" else want[1]
            assert e.status == (E.ERR_WRONG_DIMENSION if cls == "Wrong dimension" else want[0]), str(e)
            assert JOB_MESSAGES[cls] in str(e)
            return
    before = _records(engine)
    out = _out(case, device=True)
    st, olen = _job_dev(engine, case, out, mask=mask)
    message = _message(engine.lib)
    if want is None:
        _check_ok(engine, case, "dev", st, olen, out)
        assert np.array_equal(out.host(), ref.host())
        dref = _out(case, device=True)
        got = _reveal_dev(engine, case, dref)
        if got is not None:
            assert got == (E.OK, olen), _message(engine.lib)
            assert np.array_equal(out.host(), dref.host())
    else:
        _check_status(engine, case, "dev", want, st, olen, out, before, message)
    if mask is not None:
        assert mask.untouched()


FULL_SPLIT_CASES = [c for c in RJ.CASES if isinstance(c.ms, S.FullMasking) and RJ.expected_status(c) is None
                    and RJ.out_len(c) and len(RJ.blobs(c)[0]) >= 2]


@pytest.mark.parametrize("case", FULL_SPLIT_CASES, ids=[c.id for c in FULL_SPLIT_CASES])
def test_full_mask_folded_in_every_split(engine, case):
    """the state sda_clerk_job_dev leaves over the mask payloads gives the same output however they were tiled"""
    n = len(RJ.blobs(case)[0])
    want = RJ.expected_output(case)
    assert len(CJ.splits(n)) >= 3
    for split in CJ.splits(n):
        mask = FoldedMask(engine, case, split)
        assert mask.len == RJ.out_len(case)
        out = _out(case, device=True)
        st, olen = _job_dev(engine, case, out, mask=mask)
        assert st == E.OK and olen == len(want), (split, _message(engine.lib))
        out.check(want, f"{case.id} split {split}")
        assert mask.untouched()
        assert tuple(engine.recipient_job_last_launch())[0] == RJ.MASK_FULL_COMBINED


MULTI_CASES = [c for c in RJ.ADDED if isinstance(c.ms, S.ChaChaMasking) and RJ.expected_status(c) is None]


def test_host_form_on_a_multi_device_handle():
    """ChaCha masking on a handle over two devices: the decoded key words are read back, the mask combine is split,
    the output is identical and the records say so (mask_route 4, mask_kind 4)"""
    assert len(MULTI_CASES) >= 8
    multi = E.Engine(devices=[0, 0])
    try:
        for case in MULTI_CASES:
            out = _out(case, device=False)
            st, olen = _job_host(multi, case, out)
            _check_ok(multi, case, "host", st, olen, out, multi=True)
            job = tuple(multi.recipient_job_last_launch())
            assert job[0] == RJ.MASK_CHACHA_SPLIT and job[2] == len(RJ.blobs(case)[0])
            assert tuple(multi.recipient_last_launch())[0] == E.RECIPIENT_MASK_COMBINED_ROW
    finally:
        multi.close()


@pytest.mark.parametrize("fault", RJ.FAULTS, ids=[f"{f[1]}-{f[0]}" for f in RJ.FAULTS])
def test_engine_argument_checks(engine, fault):
    name, form, kind, arg, cls = fault
    case = RJ.fault_case(kind)
    mask = FoldedMask(engine, case) if kind == "full" else None
    before = _records(engine)
    out = _out(case, device=(form == "dev"))
    st, olen = (_job_dev(engine, case, out, mask=mask, fault=arg) if form == "dev"
                else _job_host(engine, case, out, fault=arg))
    message = _message(engine.lib)
    assert st == E.ERR_INVALID_ARGUMENT, (st, message)
    assert JOB_MESSAGES[cls] in message, message
    if arg != "out_len":
        assert olen == 77                           # refused before anything is written
    out.untouched(f"{name} {form}")
    assert _records(engine) == before
    if mask is not None:
        assert mask.untouched()
    # the same payloads, nothing made faulty: the call succeeds
    st, olen = (_job_dev(engine, case, out, mask=mask) if form == "dev" else _job_host(engine, case, out))
    assert st == E.OK and olen == RJ.out_len(case), _message(engine.lib)
    out.check(RJ.expected_output(case), f"{name} {form} clean")


def test_last_launch_getter(engine):
    fresh = E.Engine(0)
    try:
        assert tuple(fresh.recipient_job_last_launch()) == (0, 0, 0)
    finally:
        fresh.close()
    v = [C.c_uint32() for _ in range(3)]
    for i in range(3):
        args = [C.byref(x) for x in v]
        args[i] = None
        assert engine.lib.sda_recipient_job_last_launch(engine.h, *args) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_recipient_job_last_launch(None, *[C.byref(x) for x in v]) == E.ERR_INVALID_ARGUMENT


def test_binding_methods(engine):
    """Engine.recipient_job / recipient_job_dev give the model's output"""
    case = next(c for c in RJ.CASES if c.id == "seeds-lens-0-1-4-8-9-D256")
    mask_blobs, indexed = RJ.blobs(case)
    want = RJ.expected_output(case)
    got = engine.recipient_job(case.ms, mask_blobs, case.ss, case.dimension, indexed, case.m_out)
    assert got.tolist() == want
    seeds, clerk = DevBlobs(mask_blobs), DevBlobs([b for _, b in indexed])
    out = Guarded(len(want), 0)
    n = engine.recipient_job_dev(case.ms, case.ss, case.dimension, [i for i, _ in indexed], clerk.ptr(), clerk.off,
                                 case.m_out, out.ptr, len(want), seed_ptr=seeds.ptr(), seed_off=seeds.off)
    assert n == len(want)
    out.check(want, "binding")
    assert tuple(engine.recipient_job_last_launch()) == (RJ.MASK_CHACHA, RJ.SHARE_ADDITIVE, len(mask_blobs))
