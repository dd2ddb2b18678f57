"""GPU: the snapshot transposition's steered copy matrix (snapshot.hip) against its model and the oracle, with the
plan that ran asserted.

Every case of tests/snapshot_matrix_cases.py goes through sda_snapshot_transpose_dev into a dst buffer 256 bytes
longer than the sizing query asks for, filled with a fixed pattern.  Afterwards the ENTIRE buffer must equal
tests/snapshot_dispatch.py's transpose_model byte for byte: the blobs' bytes, every byte of alignment padding after
a clerk's job and the 256 bytes past dst_len untouched.  The per-clerk slices must equal oracle.snapshot_transpose,
the source must be unchanged, and sda_snapshot_last_launch must report exactly the record the plan predicts.
tests/test_snapshot_matrix_plan.py holds the same cases on the CPU: model == oracle, the coverage sets, and the
named index-arithmetic faults each of which some case's buffer notices.

  Q  16 shifts x 16 dst starts x the one-chunk lengths        L  body quad counts around the lane guards
  C  lengths around C, 2C, 4C at every shift                  W  the workgroup walk and its binary search
  Z  empty blobs, empty clerks, the empty snapshot            R  one handle: small plan, larger plan, small plan

The chunk size C is the one the record reports; the cases are built from it.
"""
import ctypes as C_

import numpy as np
import pytest

from sda_amd import Engine, SdaError
from sda_amd import engine as E
from tests import snapshot_dispatch as SD
from tests import snapshot_matrix_cases as CM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ZERO = (0, 0, 0, 0, 0)


def _all_empty_call(eng):
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    dlen, base, _ = eng.snapshot_transpose_dev(src.data_ptr(), [9, 9, 9], 1, 2, dst.data_ptr(), 64)
    assert dlen == 32 and base.tolist() == [0, 16]
    torch.cuda.synchronize()
    assert (dst == 0xA5).all()


@pytest.fixture(scope="module")
def chunk(engine):
    """C as sda_snapshot_last_launch reports it (a snapshot of empty blobs writes (0, 0, 0, C, 0)); the model
    restates the kernel that ships, so it must be the model's"""
    _all_empty_call(engine)
    rec = engine.snapshot_last_launch()
    assert rec[:3] == (0, 0, 0) and rec[4] == 0 and rec[3] > 0
    assert rec[3] == SD.CHUNK, "snapshot.hip's chunk changed: update tests/snapshot_dispatch.py's model of it"
    return rec[3]


def _first_difference(got, exp, pl):
    i = int(np.flatnonzero(got != exp)[0])
    where = "past dst_len" if i >= pl.dst_len else "padding"
    for b, (s, d, ln) in enumerate(pl.blobs):
        if d <= i < d + ln:
            where = f"blob {b} (src {s}, dst {d}, len {ln}, shift {(s - d) & 15}) byte {i - d}"
    return f"{int((got != exp).sum())} bytes differ, the first at dst[{i}]: {where}: {got[i]:#x}, expected {exp[i]:#x}"


def _run(eng, oracle, case, C, stream=None):
    pl, exp = CM.model(case.id, C)
    off, P, n = case.part_off(), case.P, case.n
    host_src = case.src()
    src = torch.from_numpy(host_src.copy()).cuda()
    need, _, _ = eng.snapshot_transpose_dev(src.data_ptr(), off, P, n)                 # sizing query
    assert need == pl.dst_len
    dst = torch.from_numpy(SD.fill_pattern(need + SD.GUARD)).cuda()
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    dlen, base, coff = eng.snapshot_transpose_dev(src.data_ptr(), off, P, n, dst.data_ptr(), need, stream)
    rec = eng.snapshot_last_launch()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert dlen == pl.dst_len
    assert base.tolist() == pl.clerk_base and all(int(b) % 16 == 0 for b in base)
    assert coff.tolist() == pl.clerk_off
    assert np.array_equal(got, exp), f"{case.id}: {_first_difference(got, exp, pl)}"
    assert SD.clerk_slices(got, pl) == oracle.snapshot_transpose(case.blobs())
    assert np.array_equal(src.cpu().numpy(), host_src), "the source changed"
    assert rec == pl.record, f"{case.id}: the record {rec}, the plan {pl.record}"
    return rec


@pytest.mark.parametrize("cid", CM.IDS)
def test_case(engine, oracle, chunk, cid):
    case = CM.build(chunk)[cid]
    rec = _run(engine, oracle, case, chunk)
    if case.family in "QC":
        assert rec[4] >> case.shift & 1, f"shift {case.shift} is not among the planned shifts {rec[4]:#06x}"


# ---------------------------------------------------------------- R: plan buffer reuse
@pytest.mark.parametrize("own_stream", [False, True], ids=["default-stream", "caller-stream"])
def test_plan_buffer_reuse(oracle, chunk, own_stream):
    """one fresh handle: a 1-blob plan, a plan of ~900 blobs that makes the handle's plan buffer grow, the 1-blob
    plan again; all three exact"""
    cases = CM.build(chunk)
    small, large = cases[CM.R_SMALL], cases[CM.R_LARGE]
    n_small, n_large = CM.model(small.id, chunk)[0].record[0], CM.model(large.id, chunk)[0].record[0]

    def plan_bytes(nb):                                         # 24-byte entries + the chunk prefix, each 256-aligned
        return (nb * 24 + 255) // 256 * 256 + ((nb + 1) * 8 + 255) // 256 * 256
    first = plan_bytes(n_small) + plan_bytes(n_small) // 4 + 4096       # what the first call allocates (ensure)
    assert n_small == 1 and plan_bytes(n_large) > first         # the second plan outgrows it
    eng = Engine(0)
    try:
        stream = torch.cuda.Stream() if own_stream else None
        handle = stream.cuda_stream if own_stream else None
        for case in (small, large, small):
            _run(eng, oracle, case, chunk, handle)
        if own_stream:
            stream.synchronize()
    finally:
        eng.close()


# ---------------------------------------------------------------- the record's life cycle
def _args():
    v = [C_.c_uint64() for _ in range(4)] + [C_.c_uint32()]
    return [C_.byref(x) for x in v]


def test_last_launch_refuses_null(engine):
    args = _args()
    for i in range(len(args)):
        bad = list(args)
        bad[i] = None
        assert engine.lib.sda_snapshot_last_launch(engine.h, *bad) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_snapshot_last_launch(None, *args) == E.ERR_INVALID_ARGUMENT


def test_record_is_zero_on_a_fresh_handle_and_written_by_the_empty_snapshot(chunk):
    eng = Engine(0)
    try:
        assert eng.snapshot_last_launch() == ZERO
        src = torch.zeros(64, dtype=torch.uint8, device="cuda")
        need, _, _ = eng.snapshot_transpose_dev(src.data_ptr(), [0, 8, 16], 1, 2)      # a sizing query
        assert need == 64 and eng.snapshot_last_launch() == ZERO
        _all_empty_call(eng)
        assert eng.snapshot_last_launch() == (0, 0, 0, chunk, 0)
    finally:
        eng.close()


def test_all_empty_case_writes_the_empty_record(engine, oracle, chunk):
    cases = CM.build(chunk)
    assert _run(engine, oracle, cases["Z-one"], chunk) == (1, 1, 1, chunk, 1 << 3)
    assert _run(engine, oracle, cases[CM.ALL_EMPTY], chunk) == (0, 0, 0, chunk, 0)


def test_record_is_left_by_sizing_queries_and_failed_calls(engine, oracle, chunk):
    """the three failing calls of tests/test_snapshot.py::test_gpu_transpose_rejects_bad_args, and a sizing query"""
    rec = _run(engine, oracle, CM.build(chunk)["W-9"], chunk)
    assert rec[0] == 4 and rec[1] == 9 and rec[2] == 3
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    engine.snapshot_transpose_dev(src.data_ptr(), [0, 8, 16], 1, 2)                    # sizing
    assert engine.snapshot_last_launch() == rec
    with pytest.raises(SdaError):        # decreasing offsets
        engine.snapshot_transpose_dev(src.data_ptr(), [0, 8, 4], 1, 2)
    assert engine.snapshot_last_launch() == rec
    with pytest.raises(SdaError):        # decreasing offsets with a dst
        engine.snapshot_transpose_dev(src.data_ptr(), [0, 8, 4], 1, 2, dst.data_ptr(), 64)
    assert engine.snapshot_last_launch() == rec
    with pytest.raises(SdaError):        # dst too small
        engine.snapshot_transpose_dev(src.data_ptr(), [0, 8, 16], 1, 2, dst.data_ptr(), 8)
    assert engine.snapshot_last_launch() == rec
    with pytest.raises(SdaError):        # misaligned src
        engine.snapshot_transpose_dev(src.data_ptr() + 1, [0, 8, 16], 1, 2, dst.data_ptr(), 64)
    assert engine.snapshot_last_launch() == rec
    torch.cuda.synchronize()
    assert not dst.any(), "a refused call wrote to dst"
