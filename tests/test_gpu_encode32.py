"""GPU: sda_varint_encode32_dev (varint_size32_kernel + varint_write32_kernel) over the plan of
tests/encode32_cases.py, bit-exact against oracle.varint_encode of the widened rows.

dst is a poisoned buffer: the bytes in front of the payload and behind its last byte must be untouched (the
write kernel's 16-byte interior stores and byte-wise end words must stay inside the chunk's bytes).  Every case
asserts on the oracle's output that the byte-size classes it is meant to hold occur, before it compares.
"""
import numpy as np
import pytest

from sda_amd import SdaError
from sda_amd import engine as E
from tests import codec_dispatch as CD
from tests import codec_matrix_cases as CM
from tests import encode32_cases as EC
from tests.util import assert_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FRONT = 32                 # poisoned bytes in front of dst (a multiple of 16, plus the case's dst_off)
BACK = 64


def _device_vals(v, off):
    """v [rows][stride] int32 on the device, its first element `off` int32 elements past a 16-byte boundary"""
    t = torch.empty(v.size + 8, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 16 == 0
    x = t[off:off + v.size]
    x.copy_(torch.from_numpy(np.array(v).reshape(-1)))          # a copy: the plan's arrays are read-only
    return t, x


def _dst(total, dst_off):
    buf = torch.full((FRONT + dst_off + total + BACK,), EC.POISON, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + FRONT + dst_off


def _check(buf, dst_off, payload):
    host = buf.cpu().numpy()
    a = FRONT + dst_off
    assert (host[:a] == EC.POISON).all(), "wrote in front of dst"
    assert (host[a + len(payload):] == EC.POISON).all(), "wrote past the rows' total"
    assert host[a:a + len(payload)].tobytes() == payload


def _encode(engine, case, fn=None, widen=False):
    v = EC.case_values(case)
    payload, row_bytes = EC.case_expected(case)
    EC.check_classes(case, payload)
    if widen:
        keep = torch.from_numpy(v.astype(np.int64)).cuda()
        ptr = keep.data_ptr()
    else:
        keep, x = _device_vals(v, case.vals_off)
        ptr = x.data_ptr()
        assert ptr % 16 == 4 * case.vals_off
    buf, dst = _dst(len(payload), case.dst_off)
    assert dst % 16 == case.dst_off
    rb = (fn or engine.varint_encode32_dev)(ptr, case.rows, case.length, case.stride, dst, len(payload))
    torch.cuda.synchronize()
    assert rb.tolist() == row_bytes.tolist()
    _check(buf, case.dst_off, payload)
    return rb


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.id)
def test_encode32_dev(engine, monkeypatch, case):
    if case.nt0:
        monkeypatch.setenv("SDA_ENC_NT", "0")
    else:
        monkeypatch.delenv("SDA_ENC_NT", raising=False)
    _encode(engine, case)


def test_capacity(engine, monkeypatch):
    """One byte short: INVALID_ARGUMENT and nothing written; the exact capacity succeeds (every other case)."""
    monkeypatch.delenv("SDA_ENC_NT", raising=False)
    case = EC.CASE3
    payload, _ = EC.case_expected(case)
    keep, x = _device_vals(EC.case_values(case), 0)
    buf, dst = _dst(len(payload), 0)
    with pytest.raises(SdaError) as ei:
        engine.varint_encode32_dev(x.data_ptr(), case.rows, case.length, case.stride, dst, len(payload) - 1)
    torch.cuda.synchronize()
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    assert (buf.cpu().numpy() == EC.POISON).all(), "a refused call wrote"
    engine.varint_encode32_dev(x.data_ptr(), case.rows, case.length, case.stride, dst, len(payload))
    torch.cuda.synchronize()
    _check(buf, 0, payload)


def test_arguments(engine):
    x = torch.zeros(64, dtype=torch.int32, device="cuda")
    buf, dst = _dst(64, 0)
    with pytest.raises(SdaError) as ei:
        engine.varint_encode32_dev(x.data_ptr(), 65536, 1, 1, dst, 64)
    assert ei.value.status == E.ERR_UNSUPPORTED
    with pytest.raises(SdaError) as ei:
        engine.varint_encode32_dev(x.data_ptr(), 2, 8, 7, dst, 64)
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    rb = engine.varint_encode32_dev(x.data_ptr(), 3, 0, 8, dst, 64)
    torch.cuda.synchronize()
    assert rb.tolist() == [0, 0, 0]
    assert (buf.cpu().numpy() == EC.POISON).all(), "len == 0 wrote"


def test_twin_i64_encoder_gives_the_same_bytes(engine, monkeypatch):
    monkeypatch.delenv("SDA_ENC_NT", raising=False)
    a = _encode(engine, EC.CASE3)
    b = _encode(engine, EC.CASE3, fn=engine.varint_encode_dev, widen=True)
    assert a.tolist() == b.tolist()


def test_chain_into_the_clerks_slot_decode(engine, oracle, monkeypatch):
    """int32 rows -> sda_varint_encode32_dev -> sda_clerk_decode_combine_dev: an int32 never needs more than 5
    bytes, so the clerk's int32 slot path takes the payload without falling back."""
    for k in CM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    v = EC.chain_values()
    rows, length = v.shape
    keep, x = _device_vals(v.astype(np.int32), 0)
    cap = rows * length * 5
    pay = torch.zeros(cap + 32, dtype=torch.uint8, device="cuda")
    assert pay.data_ptr() % 16 == 0
    rb = engine.varint_encode32_dev(x.data_ptr(), rows, length, length, pay.data_ptr(), cap)
    off = np.concatenate([[0], np.cumsum(rb)]).astype(np.uint64)
    out = torch.full((length + 8,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    n = engine.clerk_decode_combine_dev(EC.CHAIN_M, pay.data_ptr(), off, out.data_ptr(), length)
    torch.cuda.synchronize()
    path, _, fell_back, _ = engine.codec_last_launch()
    assert n == length
    host = out.cpu().numpy()
    assert_same(host[:length], oracle.combine(EC.CHAIN_M, v))
    assert (host[length:] == 0x5A5A5A5A).all()
    assert (path, fell_back) == (CD.SLOTS, 0)
