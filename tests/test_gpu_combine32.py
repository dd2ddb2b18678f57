"""GPU: int32 share rows as an input type of the combine (include/sda_engine.h: sda_combine32_dev,
sda_combine32_accumulate_dev, sda_narrow32_dev, sda_host_stream_stats) and the half-width host stream
(engine_host.cpp, SDA_HOST_NARROW).

The oracle is combiner.rs:16-28 over the rows widened to i64 (oracle.combine): the int32 kernels sign-extend and
run the same recurrence, so every comparison is bit for bit, for every modulus."""
import numpy as np
import pytest

from sda_amd import Engine, SdaError, schemes as S
from sda_amd import engine as E
from tests.util import assert_same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = S.CONFIG_PACKED.prime_modulus
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MODULI = [7, 1, P, (1 << 31) - 1, (1 << 63) - 25]            # the last one: SMALL_M = false
STAGE = 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows32(N, D, seed):
    """Signed int32 rows over the whole range, the limits included."""
    x = np.random.default_rng(seed).integers(I32_MIN, I32_MAX + 1, size=(N, D), dtype=np.int64)
    flat = x.reshape(-1)
    if flat.size:
        flat[0] = I32_MIN
        flat[-1] = I32_MAX
        flat[flat.size // 2] = I32_MAX
        flat[flat.size // 3] = I32_MIN
    return x.astype(np.int32)


def _combine32(engine, m, xd, n, dim, stride, ptr=None):
    out = torch.full((max(dim, 1),), -12345, dtype=torch.int64, device="cuda")
    engine.combine32_dev(m, xd.data_ptr() if ptr is None else ptr, n, dim, stride, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()[:dim]


# ---------------- sda_combine32_dev ----------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 8, 1027, 1028])
def test_combine32_dev_matches_oracle(engine, oracle, D):
    """Every row count 1..13 and 21 (the pipeline's peeled last batch, odd and even batch counts, tails of 1-3
    rows) at widths that take the 4-, 2- and 1-column kernels, every modulus class."""
    x = _rows32(21, D, 100 + D)
    xd = torch.from_numpy(x).cuda()
    wide = x.astype(np.int64)
    for N in list(range(1, 14)) + [21]:
        for m in MODULI:
            assert_same(_combine32(engine, m, xd, N, D, D), oracle.combine(m, wide[:N]), f"N={N} D={D} m={m}")


@pytest.mark.parametrize("m", MODULI)
def test_combine32_dev_offset_pointer_and_strides(engine, oracle, m):
    D, N = 1028, 11
    x = _rows32(N, D, 7)
    wide = x.astype(np.int64)
    exp = oracle.combine(m, wide)
    # rows that start one element into the buffer: only the 1-column kernel's alignment holds
    buf = torch.zeros(N * D + 1, dtype=torch.int32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    assert_same(_combine32(engine, m, buf, N, D, D, ptr=buf.data_ptr() + 4), exp, "offset by one element")
    # row_stride > dim: stride % 4 == 2 (8-byte aligned rows: the 2-column kernel), stride % 4 == 0 (16-byte loads)
    for stride in (D + 2, D + 4):
        pad = torch.full((N, stride), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        pad[:, :D] = torch.from_numpy(x).cuda()
        assert_same(_combine32(engine, m, pad, N, D, stride), exp, f"stride {stride}")


def test_combine32_dev_empty(engine):
    x = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert_same(_combine32(engine, P, x, 0, 8, 8), np.zeros(8, np.int64), "n == 0 gives zeros")
    engine.combine32_dev(P, x.data_ptr(), 3, 0, 0, None, _stream())               # dim == 0: nothing to do
    engine.combine32_dev(P, None, 0, 0, 0, None, _stream())
    with pytest.raises(SdaError) as ei:
        engine.combine32_dev(0, x.data_ptr(), 1, 8, 8, x.data_ptr(), _stream())
    assert ei.value.status == E.ERR_PRECONDITION
    with pytest.raises(SdaError) as ei:
        engine.combine32_dev(P, x.data_ptr(), 2, 8, 4, x.data_ptr(), _stream())
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [1_048_588, 100_003], ids=["above_fill_threshold", "below_fill_threshold"])
def test_combine32_balanced_grid_and_pipe_knobs(engine, oracle, monkeypatch, D):
    """The balanced grid (whole rounds of resident workgroups; taken from 131,072 lanes up at 8 workgroups per
    CU: 1,048,588 / 4 lanes is above that for any residency up to 8, and no multiple of the workgroup width)
    and its knobs: SDA_COMBINE_BALANCE=0 and SDA_COMBINE_PIPE=0 give the default's result, the oracle's."""
    N = 9
    x = _rows32(N, D, D)
    xd = torch.from_numpy(x).cuda()
    exp = oracle.combine(P, x.astype(np.int64))
    assert_same(_combine32(engine, P, xd, N, D, D), exp, "default")
    # the kernel and grid the ids name (sda_combine_last_launch): 1,048,588 columns line up for the pipelined
    # 4-column kernel on the balanced grid; 100,003 is odd, which the 1-column kernel on the plain grid takes
    wide = D % 4 == 0
    rec = engine.combine_last_launch()
    assert (rec.elem_bytes, rec.vec, rec.rows) == ((4, 4, 2) if wide else (4, 1, 8)), rec
    assert bool(rec.variant & E.COMBINE_PIPE) == wide and (rec.wlo > 0) == wide and (rec.per_cu > 0) == wide, rec
    monkeypatch.setenv("SDA_COMBINE_BALANCE", "0")
    assert_same(_combine32(engine, P, xd, N, D, D), exp, "SDA_COMBINE_BALANCE=0")
    rec = engine.combine_last_launch()
    assert (rec.vec, rec.rows, rec.wlo, rec.nwide, rec.per_cu) == ((4, 2, 0, 0, 0) if wide else (1, 8, 0, 0, 0)), rec
    monkeypatch.delenv("SDA_COMBINE_BALANCE")
    monkeypatch.setenv("SDA_COMBINE_PIPE", "0")
    assert_same(_combine32(engine, P, xd, N, D, D), exp, "SDA_COMBINE_PIPE=0")
    rec = engine.combine_last_launch()
    assert (rec.vec, rec.rows, rec.wlo, rec.per_cu) == ((4, 8, 0, 0) if wide else (1, 8, 0, 0)), rec
    assert not rec.variant & E.COMBINE_PIPE, rec


# ---------------- sda_combine32_accumulate_dev ----------------
def test_combine32_accumulate_alternates_with_i64_tiles(engine, oracle):
    """A 40 x 4,100 signed job at m = 7 (a sign event almost every step) in row tiles of 1, 4, 7, ... rows,
    alternately int32 and i64, on one accumulator that starts at zeros == one pass of the oracle."""
    m, N, D = 7, 40, 4100
    x = np.random.default_rng(40).integers(-6, 7, size=(N, D), dtype=np.int64)
    x[3, 5], x[17, 9], x[17, 10], x[39, D - 1] = I32_MIN, I32_MAX, I32_MIN, I32_MAX
    x64 = torch.from_numpy(x).cuda()
    x32 = torch.from_numpy(x.astype(np.int32)).cuda()
    acc = torch.zeros(D, dtype=torch.int64, device="cuda")
    r0, n, narrow = 0, 1, True
    while r0 < N:
        n = min(n, N - r0)
        if narrow:
            engine.combine32_accumulate_dev(m, x32[r0].data_ptr(), n, D, D, acc.data_ptr(), _stream())
        else:
            engine.combine_accumulate_dev(m, x64[r0].data_ptr(), n, D, D, acc.data_ptr(), _stream())
        r0, n, narrow = r0 + n, n + 3, not narrow
    torch.cuda.synchronize()
    exp = oracle.combine(m, x)
    assert_same(acc.cpu().numpy(), exp, "alternating tiles")
    engine.combine32_accumulate_dev(m, x32.data_ptr(), 0, D, D, acc.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(acc.cpu().numpy(), exp, "n == 0 leaves inout unchanged")


# ---------------- sda_narrow32_dev ----------------
def _narrow(engine, src, n, dim, sstride, dstride, flag0=0):
    dst = torch.full((n, dstride), 0x55555555, dtype=torch.int32, device="cuda")
    flag = torch.full((1,), flag0, dtype=torch.int64, device="cuda")
    engine.narrow32_dev(src.data_ptr(), n, dim, sstride, dst.data_ptr(), dstride, flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dst.cpu().numpy(), int(flag.item())


@pytest.mark.parametrize("sstride,dstride", [(1006, 1004), (1005, 1007), (1003, 1003)],
                         ids=["16_byte_path", "scalar_path", "dense"])
def test_narrow32_dev(engine, sstride, dstride):
    N, D = 17, 1003
    x = np.full((N, sstride), 1 << 40, dtype=np.int64)                         # padding: must not be read
    x[:, :D] = _rows32(N, D, 5).astype(np.int64)
    src = torch.from_numpy(x).cuda()
    got, flag = _narrow(engine, src, N, D, sstride, dstride)
    assert_same(got[:, :D], x[:, :D].astype(np.int32), "narrowed")
    assert (got[:, D:] == 0x55555555).all(), "destination padding was written"
    assert flag == 0
    assert _narrow(engine, src, N, D, sstride, dstride, flag0=1)[1] == 1, "a flag already 1 stays 1"
    for (r, c, v) in ((0, 0, 1 << 31), (N - 1, D - 1, -(1 << 31) - 1)):
        y = x.copy()
        y[r, c] = v
        assert _narrow(engine, torch.from_numpy(y).cuda(), N, D, sstride, dstride)[1] == 1, (r, c, v)


@pytest.mark.parametrize("sstride,dstride", [(8, 8), (7, 7)], ids=["16_byte_path", "scalar_path"])
def test_narrow32_dev_rows_past_the_grid_limit(engine, sstride, dstride):
    """launch_narrow32 clamps grid.y at 65,535 and the kernel reaches the rows past it with r += gridDim.y: 65,541
    rows (six of them a lane's second row) of 6 columns -- one 16-byte quad and a 2-column tail, or 6 scalars."""
    N, D = 65_541, 6
    x = np.full((N, sstride), 1 << 40, dtype=np.int64)                         # padding: must not be read
    x[:, :D] = _rows32(N, D, 6).astype(np.int64)
    got, flag = _narrow(engine, torch.from_numpy(x).cuda(), N, D, sstride, dstride)
    assert_same(got[:, :D], x[:, :D].astype(np.int32), "narrowed")
    assert (got[:, D:] == 0x55555555).all(), "destination padding was written"
    assert flag == 0
    x[65_540, D - 1] = 1 << 31                                                 # only a second-pass row sees it
    assert _narrow(engine, torch.from_numpy(x).cuda(), N, D, sstride, dstride)[1] == 1


def test_combine32_of_narrowed_equals_combine(engine):
    N, D = 33, 2052
    x = torch.empty((N, D), dtype=torch.int64, device="cuda")
    engine.synth_fill_dev(x.data_ptr(), N, D, 0x5DA + 32, -(P - 1), P, _stream())
    x32 = torch.empty((N, D), dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int64, device="cuda")
    engine.narrow32_dev(x.data_ptr(), N, D, D, x32.data_ptr(), D, flag.data_ptr(), _stream())
    a = torch.empty(D, dtype=torch.int64, device="cuda")
    b = torch.empty(D, dtype=torch.int64, device="cuda")
    engine.combine_dev(P, x.data_ptr(), N, D, D, a.data_ptr(), _stream())
    engine.combine32_dev(P, x32.data_ptr(), N, D, D, b.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert_same(b.cpu().numpy(), a.cpu().numpy(), "combine32(narrow32(x)) vs combine(x)")


# ---------------- half-width host stream ----------------
@pytest.fixture
def host_env(monkeypatch):
    monkeypatch.setenv("SDA_HOST_STAGE_MB", "1")
    monkeypatch.setenv("SDA_HOST_NARROW", "1")
    return monkeypatch


def _delta(eng, fn):
    before = eng.host_stream_stats()
    got = fn()
    after = eng.host_stream_stats()
    return got, tuple(a - b for a, b in zip(after, before))


def _host_rows(N, D, seed, m=P):
    rng = np.random.default_rng(seed)
    return [rng.integers(-(m - 1), m, size=D, dtype=np.int64) for _ in range(N)]


@pytest.mark.parametrize("N,D", [(37, 100_003), (5, 300_001)])
def test_host_stream_ships_fitting_rows_as_int32(engine, oracle, host_env, N, D):
    rows = _host_rows(N, D, N + D)
    exp = oracle.combine(P, np.stack(rows))
    got, (t32, t64, by) = _delta(engine, lambda: engine.share_combine(S.Additive(3, P), rows))
    assert_same(got, exp, "narrow")
    assert t32 > 0 and t64 == 0 and by == 4 * N * D, (t32, t64, by)
    host_env.setenv("SDA_HOST_NARROW", "0")
    got, (t32, t64, by) = _delta(engine, lambda: engine.share_combine(S.Additive(3, P), rows))
    assert_same(got, exp, "wide")
    assert t32 == 0 and t64 > 0 and by == 8 * N * D, (t32, t64, by)


@pytest.fixture(scope="module")
def mixed_job():
    return np.random.default_rng(3).integers(-6, 7, size=(200, 131_081), dtype=np.int64)


@pytest.mark.parametrize("row", [100, 0, 199], ids=["middle_row", "row_0", "last_row"])
def test_host_stream_mixed_rows(engine, oracle, host_env, mixed_job, row):
    """One value of 2^31 in the first column chunk (a 1 MiB stage cuts the 131,081 columns into 131,072 + 9, one
    row per tile in the first chunk): the tile that holds it and the rest of its chunk ship as i64, the other
    chunk as int32; the value goes through the same `%`."""
    m, (N, D) = 7, mixed_job.shape
    x = mixed_job
    keep = x[row, 5]
    x[row, 5] = 1 << 31
    try:
        exp = oracle.combine(m, x)
        got, (t32, t64, by) = _delta(engine, lambda: engine.share_combine(S.Additive(3, m), list(x)))
    finally:
        x[row, 5] = keep
    assert_same(got, exp, f"row {row}")
    assert t32 > 0 and t64 > 0 and 4 * N * D < by < 8 * N * D, (t32, t64, by)
    if row == 0:
        wc0 = STAGE // 8                                     # the first chunk's columns
        assert by == 8 * N * wc0 + 4 * N * (D - wc0), (t32, t64, by)
        assert t64 == N, "one row per tile in the first chunk, all wide"


def test_host_stream_validation_stages_nothing(engine, host_env):
    rows = _host_rows(160, 20_001, 1)
    rows[150] = rows[150][:-1]
    before = engine.host_stream_stats()
    with pytest.raises(SdaError) as ei:
        engine.share_combine(S.Additive(3, P), rows)
    assert ei.value.status == E.ERR_WRONG_DIMENSION
    assert engine.host_stream_stats() == before


def test_host_stream_multi_device_handle(oracle, host_env):
    """Three column slices (ordinals repeat: one GPU): the stats are the sum over the slices."""
    eng = Engine(devices=[0, 0, 0])
    try:
        N, D = 23, 10_001
        rows = _host_rows(N, D, D)
        exp = oracle.combine(P, np.stack(rows))
        got, d = _delta(eng, lambda: eng.share_combine(S.Additive(3, P), rows))
        assert_same(got, exp, "share_combine")
        assert d[1] == 0 and d[2] == 4 * N * D, d
        got, d = _delta(eng, lambda: eng.secret_reconstruct(S.Additive(N, P), D, list(enumerate(rows))))
        assert_same(got, exp, "additive reconstruct")
        assert d[1] == 0 and d[2] == 4 * N * D, d
        masks = [np.abs(r) for r in rows[:9]]
        got, d = _delta(eng, lambda: eng.mask_combine(S.FullMasking(P), masks))
        assert_same(got, oracle.combine(P, np.stack(masks)), "full masks")
        assert d[1] == 0 and d[2] == 4 * 9 * D, d
    finally:
        eng.close()
