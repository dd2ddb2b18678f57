"""GPU: the share-combine's dispatch matrix (combine.hip) against the oracle, the kernel and grid that ran asserted.

Every case of tests/combine_matrix_cases.py runs bit-exactly against oracle.combine (int32 rows: the oracle of the
widened rows), writes into a poisoned buffer between guard words, and must report through sda_combine_last_launch
the record tests/combine_dispatch.py predicts from the actual device pointers: all of the combine's kernels are
exact, so a case that silently reached another instantiation or grid than it names would pass on its numbers alone.
tests/test_combine_matrix_plan.py holds the same cases against the built library, the oracle and the events their
steered columns must hit, on the CPU.

  a  all 34 combine_exact_kernel instantiations at two workgroups (the second of 3 lanes), every row count around
     the batch of each (no whole batch; 1-4 batches: the pipeline's peeled last batch on both buffers; tails of 0, 1
     and U - 1 rows; 0 rows), at the first, last and a middle modulus of their SMALL_M class, on steered columns that
     put r + v and v on the edges of add_trem's adjust, selector and i64 wrap; every alignment fall-back.
  b  the split's flags: all four outcomes and a word already 1, computed from the inputs.
  c  the 4 combine_replay_kernel instantiations against a Python-integer model of the replay step.
  d  the balanced grid of the ten pipelined instantiations: the shapes are derived from the occupancy the record
     reports and the device's CU count, and the grid the record reports must be combine_dispatch.grid()'s; steered
     columns sit on both sides of every kind of workgroup boundary.
  e  the record's own semantics.
"""
import ctypes as C

import numpy as np
import pytest

from sda_amd import Engine
from sda_amd import engine as E
from sda_amd import schemes as S
from tests import combine_dispatch as CB
from tests import combine_matrix_cases as CM
from tests.util import assert_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = CM.POISON
NO_LAUNCH = (CB.NONE, 0, 0, 0, 0, 0, 0, 0, 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _env(monkeypatch, env):
    for k in CB.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _rows_on_device(elem_bytes, rows, stride, in_off):
    """rows [n][dim] in a buffer of row stride `stride`, `in_off` elements into the allocation, the row padding
    and the lead poisoned; returns (tensor, pointer to row 0)"""
    n, dim = rows.shape
    dt = np.int64 if elem_bytes == 8 else np.int32
    host = np.full(in_off + max(n, 1) * stride, POISON if elem_bytes == 8 else CM.POISON32, dt)
    host[in_off:in_off + n * stride].reshape(n, stride)[:, :dim] = rows
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + in_off * elem_bytes


def _out_on_device(dim, out_off, acc0):
    """GUARD poisoned words, out_off more, `out` (poison, or the initial accumulator), GUARD poisoned words"""
    host = np.full(CM.GUARD + out_off + dim + CM.GUARD, POISON, np.int64)
    if acc0 is not None:
        host[CM.GUARD + out_off:CM.GUARD + out_off + dim] = acc0
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + (CM.GUARD + out_off) * 8


def _split_out(t, dim, out_off, what):
    host = t.cpu().numpy()
    lo = CM.GUARD + out_off
    assert (host[:lo] == POISON).all(), f"{what}: wrote in front of out"
    assert (host[lo + dim:] == POISON).all(), f"{what}: wrote past out"
    return host[lo:lo + dim]


def _check_record(rec, pred, n_lanes, what, geom=None):
    """the instantiation, and the grid: the plain one of 256-lane workgroups unless `geom`"""
    got = (rec.kind, rec.elem_bytes, rec.vec, rec.rows, rec.variant)
    assert got == tuple(pred[:5]), f"{what}: ran {got}, the case names {pred.kernel} {tuple(pred[:5])}"
    if geom is None:
        assert (rec.grid, rec.wlo, rec.nwide) == (CB.plain_grid(n_lanes), 0, 0), (what, rec)
    else:
        assert (rec.grid, rec.wlo, rec.nwide) == geom, (what, rec, geom)
    if pred.variant & CB.PIPE:
        assert 1 <= rec.per_cu <= 8, (what, rec)
    else:
        assert rec.per_cu == 0, (what, rec)


def _call(engine, case, n, in_ptr, out_ptr, flags_ptr=None):
    s = case.shape
    args = (case.m, in_ptr, n, s.dim, s.stride, out_ptr)
    if case.flag:
        engine.combine_split_dev(*args, flags_ptr, _stream())
    else:
        getattr(engine, case.entry)(*args, _stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- a, b: every instantiation, small shapes
@pytest.mark.parametrize("case", CM.EXACT_CASES, ids=lambda c: c.id)
def test_exact_kernel(engine, oracle, monkeypatch, case):
    _env(monkeypatch, case.env())
    s, elem = case.shape, case.inst.elem_bytes
    for n in case.ns:
        what = f"{case.id} n={n}"
        inp = case.inputs(n)
        xd, in_ptr = _rows_on_device(elem, inp.rows, s.stride, s.in_off)
        od, out_ptr = _out_on_device(s.dim, s.out_off, inp.acc0)
        flags0 = [1, 1] if case.flag_mode.endswith("+1") else [0, 0]
        fd = torch.tensor([POISON] + flags0 + [POISON], dtype=torch.int64, device="cuda") if case.flag else None
        before = engine.combine_last_launch()
        _call(engine, case, n, in_ptr, out_ptr, fd.data_ptr() + 8 if case.flag else None)
        rec = engine.combine_last_launch()
        got = _split_out(od, s.dim, s.out_off, what)
        if n == 0 and case.acc:                      # nothing launched: inout and the record are left
            assert_same(got, inp.acc0, what)
            assert rec == before, what
            if case.flag:
                assert fd.tolist() == [POISON] + flags0 + [POISON]
            continue
        full = inp.rows if inp.acc0 is None else np.vstack([inp.acc0[None, :], inp.rows])
        exp = oracle.combine(case.m, full) if n or case.acc else np.zeros(s.dim, np.int64)
        bad = np.nonzero(got != exp)[0]
        steered = {h[0]: h[2] for h in inp.hits}
        assert bad.size == 0, (f"{what}: {bad.size} columns differ, first {bad[:8].tolist()} "
                               f"(steered events there: {[steered.get(int(c)) for c in bad[:8]]})")
        _check_record(rec, case.predicted(n, xd.data_ptr(), od.data_ptr()), s.dim // case.inst.vec, what)
        if case.flag:
            want = CM.expected_flags(case.m, inp.rows)
            assert fd.tolist() == [POISON] + [max(a, b) for a, b in zip(flags0, want)] + [POISON], what


# ---------------------------------------------------------------- c: the replay kernel
@pytest.mark.parametrize("case", CM.REPLAY_CASES, ids=lambda c: c.id)
def test_replay_kernel(engine, monkeypatch, case):
    _env(monkeypatch, {})
    s, rank = case.shape, 3
    for n in case.ns:
        what = f"{case.id} n={n}"
        rows, state0, code0 = CM.replay_inputs(case.m, n, s.dim, n)
        xd, in_ptr = _rows_on_device(8, rows, s.stride, s.in_off)
        sd, st_ptr = _out_on_device(s.dim, 0, state0)
        code_host = np.full(CM.GUARD + s.code_off + s.dim + CM.GUARD, CM.POISON32, np.int32)
        lo = CM.GUARD + s.code_off
        code_host[lo:lo + s.dim] = code0
        cd = torch.from_numpy(code_host).cuda()
        before = engine.combine_last_launch()
        engine.combine_split_replay_dev(case.m, in_ptr, n, s.dim, s.stride, rank, st_ptr, cd.data_ptr() + lo * 4,
                                        _stream())
        torch.cuda.synchronize()
        rec = engine.combine_last_launch()
        got_state = _split_out(sd, s.dim, 0, what)
        got_code = cd.cpu().numpy()
        assert (got_code[:lo] == CM.POISON32).all() and (got_code[lo + s.dim:] == CM.POISON32).all(), what
        exp_state, exp_code = CM.model_replay(case.m, rows, state0, code0, 2 * rank + 1)
        assert got_state.tolist() == exp_state, what
        assert got_code[lo:lo + s.dim].tolist() == exp_code, what
        if n == 0:
            assert rec == before, what
            continue
        pred = case.predicted(n, xd.data_ptr(), sd.data_ptr(), cd.data_ptr())
        _check_record(rec, pred, s.dim // case.vec, what)


# ---------------------------------------------------------------- d: the balanced grid
_per_cu = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _entry(inst, acc, flag):
    if inst.elem_bytes == 4:
        return "combine32_accumulate_dev" if acc else "combine32_dev"
    return "combine_split_dev" if flag else ("combine_accumulate_dev" if acc else "combine_dev")


def _run(engine, inst, acc, flag, m, n, dim, stride, in_ptr, out_ptr, flags_ptr):
    args = (m, in_ptr, n, dim, stride, out_ptr)
    if flag:
        engine.combine_split_dev(*args, flags_ptr, _stream())
    else:
        getattr(engine, _entry(inst, acc, flag))(*args, _stream())
    torch.cuda.synchronize()
    return engine.combine_last_launch()


def _occupancy(engine, key):
    """per_cu of a pipelined instantiation, read from the record of one launch large enough to fill a round at any
    per_cu <= 8 (64 lanes on each of 8 * 256 slots; one row of zeros)"""
    if key not in _per_cu:
        inst, small, acc, flag = key
        m = CM.P if small else 2**63 - 25
        n_lanes = 64 * 256 * 8
        dim = n_lanes * inst.vec
        x = torch.zeros(dim, dtype=torch.int64 if inst.elem_bytes == 8 else torch.int32, device="cuda")
        out = torch.zeros(dim, dtype=torch.int64, device="cuda")
        fl = torch.zeros(2, dtype=torch.int64, device="cuda")
        rec = _run(engine, inst, acc, flag, m, 1, dim, dim, x.data_ptr(), out.data_ptr(), fl.data_ptr())
        want = CB.predict(inst.elem_bytes, dim, dim, x.data_ptr(), out.data_ptr(), m, acc, flag, {})
        assert 1 <= rec.per_cu <= 8, rec
        _check_record(rec, want, n_lanes, f"occupancy probe {want.kernel}", CB.grid(rec.per_cu, _cus(), n_lanes))
        assert int(out.abs().max()) == 0 and fl.tolist() == [0, 0]
        _per_cu[key] = rec.per_cu
    return _per_cu[key]


def _balanced_job(inst, small, acc, m, n_lanes, stride_pad, geom, seed):
    """random rows (inside (-m, m) for SMALL_M, else over the whole element type) with steered columns in the
    lanes around every kind of workgroup boundary; returns (rows [R][stride], acc0, dim, steered columns)"""
    R = CM.BALANCED_ROWS[2 * inst.rows]
    dim = n_lanes * inst.vec
    stride = dim + stride_pad
    tmin, tmax = CM.limits(inst.elem_bytes)
    rng = np.random.default_rng(seed)
    lo, hi = (max(-(m - 1), tmin), min(m - 1, tmax)) if small else (tmin, tmax)
    rows = rng.integers(lo, hi, size=(R, stride), dtype=np.int64, endpoint=True)
    acc0 = rng.integers(-(m - 1), m - 1, size=dim, dtype=np.int64, endpoint=True) if acc else None
    cols = [lane * inst.vec + e for lane in CM.boundary_lanes(n_lanes, geom) for e in range(inst.vec)]
    st = CM.steered(inst.elem_bytes, m, R, len(cols), acc, seed)
    rows[:, cols] = st.rows
    if acc:
        acc0[cols] = st.acc0
    return rows, acc0, dim, cols


def _balanced_run(engine, oracle, inst, small, acc, flag, m, geo, padded, what, expect_balanced=True):
    per_cu = _occupancy(engine, (inst, small, acc, flag))
    cus = _cus()
    n_lanes = CM.balanced_lanes(cus * per_cu, per_cu)[geo]
    geom = CB.grid(per_cu, cus, n_lanes)
    assert (geom is None) == (geo == "below"), (what, per_cu, cus, n_lanes, geom)
    pad = 4 * inst.vec if padded else 0
    rows, acc0, dim, cols = _balanced_job(inst, small, acc, m, n_lanes, pad, geom, n_lanes % 9973 + 31 * acc + flag)
    dt = torch.int64 if inst.elem_bytes == 8 else torch.int32
    xd = torch.from_numpy(rows).to(dt).cuda() if inst.elem_bytes == 4 else torch.from_numpy(rows).cuda()
    od, out_ptr = _out_on_device(dim, 0, acc0)
    fd = torch.zeros(2, dtype=torch.int64, device="cuda")
    rec = _run(engine, inst, acc, flag, m, rows.shape[0], dim, dim + pad, xd.data_ptr(), out_ptr, fd.data_ptr())
    got = _split_out(od, dim, 0, what)
    full = rows[:, :dim] if acc0 is None else np.vstack([acc0[None, :], rows[:, :dim]])
    exp = oracle.combine(m, full)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} columns differ, first {bad[:8].tolist()} (steered: {cols[:4]}...)"
    pred = CB.predict(inst.elem_bytes, dim, dim + pad, xd.data_ptr(), out_ptr, m, acc, flag, {})
    assert pred.variant & CB.PIPE
    if expect_balanced:
        _check_record(rec, pred, n_lanes, what, geom)
        assert rec.per_cu == per_cu
        assert (rec.wlo > 0) == (geo != "below"), (what, rec)
        assert not padded or rec.wlo > 0, (what, rec)            # row stride > dim runs on the balanced grid
    else:
        assert (rec.grid, rec.wlo, rec.nwide, rec.per_cu) == (CB.plain_grid(n_lanes), 0, 0, 0), (what, rec)
        assert (rec.kind, rec.elem_bytes, rec.vec, rec.rows, rec.variant) == tuple(pred[:5]), (what, rec)
    if flag:
        assert fd.tolist() == CM.expected_flags(m, rows[:, :dim]), what
    return rec, per_cu, n_lanes


def _balanced_id(p):
    (inst, small, acc, flag), geo, m, padded = p
    v = "split" if flag else ("acc" if acc else "plain")
    return f"{inst.tag}-{'S' if small else 'B'}-{v}-{geo}-m{m}{'-padded' if padded else ''}"


@pytest.mark.parametrize("p", CM.balanced_plan(), ids=_balanced_id)
def test_balanced_grid(engine, oracle, monkeypatch, p):
    _env(monkeypatch, {})
    (inst, small, acc, flag), geo, m, padded = p
    _balanced_run(engine, oracle, inst, small, acc, flag, m, geo, padded, _balanced_id(p))


@pytest.mark.parametrize("fam", ["i64", "i64_flag", "int32"])
def test_balance_knob_off_gives_the_plain_grid(engine, oracle, monkeypatch, fam):
    inst, small, acc, flag = next(p for p in CM.PIPELINED if CM.family(p[0], p[3]) == fam and p[1] and p[2])
    _env(monkeypatch, {})
    _occupancy(engine, (inst, small, acc, flag))                 # read with the balanced grid on
    _env(monkeypatch, {"SDA_COMBINE_BALANCE": "0"})
    _balanced_run(engine, oracle, inst, small, acc, flag, CM.P, "mixed", False, f"{fam} SDA_COMBINE_BALANCE=0",
                  expect_balanced=False)


def test_pipelined_kernels_run_8_workgroups_per_cu(engine, monkeypatch):
    """DESIGN.md §4.1 and tests/test_kernel_resources*.py: at most 64 VGPRs, "occupancy 8" -- as the runtime
    reports it for each of the ten pipelined instantiations."""
    _env(monkeypatch, {})
    got = {CB.exact_name(i.elem_bytes, i.vec, i.rows, s, a, f, True): _occupancy(engine, (i, s, a, f))
           for i, s, a, f in CM.PIPELINED}
    assert len(got) == 10
    assert all(v == 8 for v in got.values()), got


# ---------------------------------------------------------------- e: the record
def _args():
    v = [C.c_uint32() for _ in range(5)] + [C.c_uint64()] + [C.c_uint32() for _ in range(3)]
    return [C.byref(x) for x in v]


def test_last_launch_refuses_null(engine):
    args = _args()
    for i in range(len(args)):
        bad = list(args)
        bad[i] = None
        assert engine.lib.sda_combine_last_launch(engine.h, *bad) == E.ERR_INVALID_ARGUMENT
    assert engine.lib.sda_combine_last_launch(None, *args) == E.ERR_INVALID_ARGUMENT


def test_record_of_a_fresh_handle_and_of_calls_that_launch_nothing(monkeypatch):
    _env(monkeypatch, {})
    eng = Engine(0)
    try:
        assert eng.combine_last_launch() == NO_LAUNCH
        x = torch.ones(3 * 518, dtype=torch.int64, device="cuda")
        out = torch.zeros(518, dtype=torch.int64, device="cuda")
        eng.combine_dev(CM.P, x.data_ptr(), 3, 0, 0, None, _stream())              # dim == 0
        eng.combine_accumulate_dev(CM.P, x.data_ptr(), 0, 518, 518, out.data_ptr(), _stream())
        assert eng.combine_last_launch() == NO_LAUNCH
        eng.combine_dev(CM.P, x.data_ptr(), 3, 518, 518, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        rec = eng.combine_last_launch()
        assert rec[:5] == tuple(CB.predict(8, 518, 518, x.data_ptr(), out.data_ptr(), CM.P, False, False, {})[:5])
        assert (rec.grid, rec.wlo, rec.nwide) == (2, 0, 0) and out.tolist() == [3] * 518
        eng.combine_dev(CM.P, x.data_ptr(), 3, 0, 0, None, _stream())
        eng.combine32_dev(CM.P, x.data_ptr(), 3, 0, 0, None, _stream())
        eng.combine_accumulate_dev(CM.P, x.data_ptr(), 0, 518, 518, out.data_ptr(), _stream())
        eng.combine32_accumulate_dev(CM.P, x.data_ptr(), 0, 518, 518, out.data_ptr(), _stream())
        fl = torch.zeros(2, dtype=torch.int64, device="cuda")
        eng.combine_split_dev(CM.P, x.data_ptr(), 0, 518, 518, out.data_ptr(), fl.data_ptr(), _stream())
        assert eng.combine_last_launch() == rec
    finally:
        eng.close()


def test_record_after_the_codec_matrix_combine(engine, oracle, monkeypatch):
    """sda_clerk_decode_combine_dev on its int32 matrix path ends in launch_combine_exact32: 2 columns per lane."""
    from tests import codec_matrix_cases as XM
    _env(monkeypatch, {})
    monkeypatch.setenv("SDA_CODEC_PATH", "matrix")
    dim = 700
    x = np.random.default_rng(11).integers(-(CM.P - 1), CM.P, size=(5, dim), dtype=np.int64)
    buf, off, _ = XM._job([oracle.varint_encode(r) for r in x], x)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    out = torch.full((dim,), POISON, dtype=torch.int64, device="cuda")
    assert engine.clerk_decode_combine_dev(CM.P, t.data_ptr(), off, out.data_ptr(), dim) == dim
    torch.cuda.synchronize()
    assert engine.codec_last_launch()[0] == E.CODEC_MATRIX32
    assert_same(out.cpu().numpy(), oracle.combine(CM.P, x), "matrix32")
    rec = engine.combine_last_launch()
    pred = CB.predict(4, dim, dim, 0, out.data_ptr(), CM.P, False, False, {}, codec=True)
    assert pred.kernel == "combine_exact_kernel<int, 2, 8, true, false, false, false>"
    _check_record(rec, pred, dim // 2, "matrix32")


def test_record_after_the_host_stream_is_its_last_tile(oracle, monkeypatch):
    """40 rows of 4,096 columns through 1 MiB tiles: 32 rows, then 8 rows continuing the accumulator."""
    _env(monkeypatch, {})
    monkeypatch.setenv("SDA_HOST_STAGE_MB", "1")
    eng = Engine(0)
    try:
        x = np.random.default_rng(12).integers(-(CM.P - 1), CM.P, size=(40, 4096), dtype=np.int64)
        got = eng.share_combine(S.Additive(3, CM.P), list(x))
        assert_same(np.asarray(got), oracle.combine(CM.P, x), "host stream")
        t32, t64, _ = eng.host_stream_stats()
        assert t32 + t64 == 2
        rec = eng.combine_last_launch()
        pred = CB.predict(4 if t32 else 8, 4096, 4096, 0, 0, CM.P, True, False, {})
        _check_record(rec, pred, 4096 // pred.vec, "last tile")
    finally:
        eng.close()


def test_multi_device_handle_reports_its_first_slice(oracle, monkeypatch):
    """1,537 columns over three sub-handles: slices of 514, 512 and 511 columns (column_slice: even-aligned), which
    take three different launches -- 257 lanes of 2 columns on two workgroups, one workgroup, and 511 lanes of 1
    column.  The handle reports the first slice's."""
    _env(monkeypatch, {})
    eng = Engine(devices=[0, 0, 0])
    try:
        x = np.random.default_rng(13).integers(-(CM.P - 1), CM.P, size=(7, 1537), dtype=np.int64)
        got = eng.share_combine(S.Additive(3, CM.P), list(x))
        assert_same(np.asarray(got), oracle.combine(CM.P, x), "multi-device")
        rec = eng.combine_last_launch()
        assert rec.elem_bytes in (4, 8)
        preds = [CB.predict(rec.elem_bytes, w, w, 0, 0, CM.P, False, False, {}) for w in (514, 512, 511)]
        shapes = [(p.vec, CB.plain_grid(w // p.vec)) for p, w in zip(preds, (514, 512, 511))]
        assert len(set(shapes)) == 3 and shapes[0] == (2, 2), shapes
        _check_record(rec, preds[0], 257, "first slice")
    finally:
        eng.close()
