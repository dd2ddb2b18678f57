"""GPU: the share payload codec's dispatch matrix (codec_decode.hip, codec_encode.hip) against the oracle, with the kernel that ran asserted.

Every case of tests/codec_matrix_cases.py runs bit-exactly against oracle.combine, oracle.varint_decode or
oracle.varint_encode, writes into a poisoned buffer, and -- for sda_clerk_decode_combine_dev -- must report through
sda_codec_last_launch exactly the (path, width, fell_back, passes) record the case states: all of the codec's paths
are exact, so a case that silently reached another kernel than it names would pass on its numbers alone.
tests/test_codec_matrix_plan.py holds the same cases against their payload bytes and the built library on the CPU.

  a  slot_combine_kernel<CPL, 8, SMALL_M>: SDA_SLOT_CPL 1/2/4, seven moduli, 1..17 blobs (the 8-blob unroll and
     its tail), dimensions around one tile of 256 CPL columns and past two regions, the grouped path.  The shares
     fit int32, so for m > 2^62 (SMALL_M = false) no sum ever reaches m: those cases check that instantiation's
     indexing and loads, not its `%`.  The small moduli (|v| >> m) are what drive add_trem's trem64 branch.
  b  every fall-back of decode_combine() with the bit that names it.
  c  varint_decode_combine_kernel<DEPTH, MULTI>: SDA_DC_DEPTH 2/4/8 with fewer blobs than the ring, whole rings and
     a ring and a tail; 10-byte elements for the multi-round variant.
  d  65,538 payloads: every per-blob grid is sliced in steps of 65,535.
  e  more than 256 regions per blob, more than 256 encode chunks per row, more than 256 rows: the scans' carries.
  f  SDA_DEC_NT 0/1 on each of the three decodes.
  g  payload boundaries and elements at every offset around region and sub-region edges.
"""
import functools

import numpy as np
import pytest

from sda_amd import engine as E
from tests import codec_dispatch as CD
from tests import codec_matrix_cases as CM
from tests.util import assert_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0x5A5A5A5A5A5A5A5A
PAD = 64


def _env(monkeypatch, case):
    for k in CM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env().items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=2)
def _device_job(builder, args):
    """the job's bytes on the device (shared by the cases over one payload set)"""
    buf, off, rows = CM.BUILDERS[builder](*args)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, off, rows


@functools.lru_cache(maxsize=2)
def _expected(builder, args, m):
    from oracle import oracle as O
    return O.combine(m, CM.BUILDERS[builder](*args)[2])


@pytest.mark.parametrize("case", CM.COMBINE_CASES, ids=lambda c: c.id)
def test_decode_combine(engine, monkeypatch, case):
    _env(monkeypatch, case)
    t, off, rows = _device_job(case.builder, case.args)
    dim = rows.shape[1]
    out = torch.full((dim + PAD,), POISON, dtype=torch.int64, device="cuda")
    n = engine.clerk_decode_combine_dev(case.m, t.data_ptr(), off, out.data_ptr(), dim)
    torch.cuda.synchronize()
    record = engine.codec_last_launch()
    host = out.cpu().numpy()
    assert n == dim
    assert_same(host[:dim], _expected(case.builder, case.args, case.m), case.id)
    assert (host[dim:] == POISON).all(), "wrote past the dimension"
    assert record == case.record, (f"ran {CD.PATH_NAMES[record[0]]} {record[1:]}, the case names "
                                   f"{CD.PATH_NAMES[case.record[0]]} {case.record[1:]}")


@pytest.mark.parametrize("case", CM.DECODE_CASES, ids=lambda c: c.id)
def test_decode_dev(engine, monkeypatch, case):
    _env(monkeypatch, case)
    t, off, rows = _device_job(case.builder, ())
    n = len(off) - 1
    if isinstance(rows, dict):                       # section d: the picked blobs
        check, counts_exp = rows, np.full(n, CM.BIG_DIM)
        counts_exp[65_537] = CM.BIG_DIM + 1
    else:
        check = dict(enumerate(rows))
        counts_exp = np.array([len(r) for r in rows])
    stride = int(counts_exp.max()) + 3
    out = torch.full((n, stride), POISON, dtype=torch.int64, device="cuda")
    counts = engine.varint_decode_dev(t.data_ptr(), off, out.data_ptr(), stride)
    torch.cuda.synchronize()
    assert counts.tolist() == counts_exp.tolist()
    if len(check) < n:
        host = {b: out[b].cpu().numpy() for b in check}
    else:
        host = dict(enumerate(out.cpu().numpy()))
    for b, r in check.items():
        assert_same(host[b][:len(r)], np.asarray(r), f"{case.id} blob {b}")
        assert (host[b][len(r):] == POISON).all(), f"blob {b}: wrote past its count"


@pytest.mark.parametrize("case", CM.ENCODE_CASES, ids=lambda c: c.id)
def test_encode_dev(engine, oracle, monkeypatch, case):
    _env(monkeypatch, case)
    v = CM.encode_values(case.seed, case.rows, case.length, case.stride)
    exp_rows = [oracle.varint_encode(v[r, :case.length]) for r in range(case.rows)]
    exp = b"".join(exp_rows)
    x = torch.from_numpy(v).cuda()
    assert x.data_ptr() % 16 == 0 and x.is_contiguous()
    buf = torch.full((len(exp) + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    row_bytes = engine.varint_encode_dev(x.data_ptr(), case.rows, case.length, case.stride, buf.data_ptr(), len(exp))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert row_bytes.tolist() == [len(b) for b in exp_rows]
    assert host[:len(exp)].tobytes() == exp
    assert (host[len(exp):] == 0xA5).all(), "wrote past the rows' total"


def test_last_launch_refuses_null(engine):
    import ctypes as C
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    args = [C.byref(a), C.byref(b), C.byref(c), C.byref(d)]
    for i in range(4):
        bad = list(args)
        bad[i] = None
        assert engine.lib.sda_codec_last_launch(engine.h, *bad) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_codec_last_launch(None, *args) == E.ERR_INVALID_ARGUMENT


def test_record_is_none_after_a_failed_call_and_after_the_host_path(engine, oracle, monkeypatch):
    for k in CM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(5)
    x = rng.integers(-(CM.M31 - 1), CM.M31, size=(4, 700), dtype=np.int64)
    blobs = [oracle.varint_encode(r) for r in x]
    buf, off, _ = CM._job(blobs, x)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    out = torch.full((700,), POISON, dtype=torch.int64, device="cuda")

    def good():
        assert engine.clerk_decode_combine_dev(CM.M31, t.data_ptr(), off, out.data_ptr(), 700) == 700
        assert engine.codec_last_launch() == (CD.SLOTS, 4, 0, 1)

    good()
    ragged = [blobs[0], blobs[1], oracle.varint_encode(x[2][:-1]), blobs[3]]
    rbuf, roff, _ = CM._job(ragged, None)
    rt = torch.frombuffer(bytearray(rbuf), dtype=torch.uint8).cuda()
    with pytest.raises(E.SdaError):
        engine.clerk_decode_combine_dev(CM.M31, rt.data_ptr(), roff, out.data_ptr(), 700)
    assert engine.codec_last_launch() == (CD.NONE, 0, 0, 0)
    good()
    with pytest.raises(E.SdaError):                  # an output too small: the record stays NONE
        engine.clerk_decode_combine_dev(CM.M31, t.data_ptr(), off, out.data_ptr(), 699)
    assert engine.codec_last_launch() == (CD.NONE, 0, 0, 0)
    good()
    from sda_amd import schemes as S
    got = engine.clerk_decode_combine(S.Additive(3, CM.M31), blobs)
    assert_same(np.asarray(got), oracle.combine(CM.M31, x), "host path")
    assert engine.codec_last_launch() == (CD.NONE, 0, 0, 0)
