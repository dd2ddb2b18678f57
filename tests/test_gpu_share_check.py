"""GPU: the packed-Shamir share consistency check (sda_packed_check_dev, sda_packed_check32_dev, sda_secret_check)
against tests/share_check_model.py.

Shares come from the oracle's packed_generate (two participants per scheme, built once per scheme and shared).  A
case takes the rows of n_idx clerks, plants its errors on the residues, writes every value in one of the
representations a clerk may send -- exact signed, canonical, mixed, share - p and share + p, and for i64 raw values
far outside (-p, p), next to i64::MIN included -- and compares the whole guarded verdict buffer, the counts,
first_bad, blame and the launch record with the model.  The explicit expectations of the definitions (located at the
planted position for r >= 2, 0xFFFF for r = 1, for two errors with r >= 3 and for f(1) != 0) are asserted besides.

The shapes are the smallest that reach every guard: V = 3 vectors of B = 549 / 550 batches with an odd dimension (a
zero-padded tail batch, more than one tile, blockIdx.y > 0), and B = 1, 255, 256, 257 at V = 1.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import packed_matrix_cases as PM
from tests import share_check_model as M
from tests.test_share_check_model import SCHEMES

pytestmark = pytest.mark.gpu

GUARD = 8                      # uint16 words on each side of the verdict buffer
SENT = 0xBEEF
I64_MIN = -(1 << 63)
UNSUPPORTED, INVALID, NOT_ENOUGH = 66, 65, 6


def _kt(sch):
    return sch.secret_count + sch.privacy_threshold()


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, V, B):
    """[2 participants][V][n][B] exact signed shares from the oracle, and the dimension (odd, zero-padded tail)."""
    from oracle import oracle as O
    sch = SCHEMES[name]
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    D = PM.dimension(B, k)
    pp = O.packed_params(k, n, t, p, sch.omega_secrets, sch.omega_shares)
    rng = np.random.default_rng(1000 * V + B)
    out = np.empty((2, V, n, B), np.int64)
    for a in range(2):
        for v in range(V):
            out[a, v] = O.packed_generate(pp, rng.integers(0, p, D), rng.integers(0, p - 1, B * t))
    out.setflags(write=False)
    return out, D


def _plants(n_idx, V, B, p):
    """{(vec, b): [(position j0, error), ...]} and the special cells: single errors +1, -1, (p - 1) / 2 in the first
    and last lane of a tile, the last batch overall, vectors 0 and V - 1, the zero-padded tail batch of every vector,
    and every clerk position once; one batch with two errors; one with every share moved (f(1) != 0); one all zero."""
    errs = (1, -1, (p - 1) // 2)
    cells = {}

    def put(vec, b, j, e):
        if b < B and (vec, b) not in cells:
            cells[(vec, b)] = [(j % n_idx, e)]

    put(0, 0, 0, errs[0])
    put(0, 255, 1, errs[1])
    put(V - 1, 256, 2, errs[2])
    put(V - 1, 511, 3, errs[0])
    put(V - 1, 512, 4, errs[1])
    for v in range(V):
        put(v, B - 1, v + 1, errs[v % 3])                  # the tail batch; (V - 1, B - 1) is the last batch overall
    taken = {j for c in cells.values() for j, _ in c}
    for j in range(n_idx):                                 # every position once across the run
        if j in taken:
            continue
        for step in range(B * V):
            cell = ((j + step) % V, (7 * j + 3 + step) % B)
            if cell not in cells:
                cells[cell] = [(j, errs[j % 3])]
                break
    special = {}
    free = [(v, b) for b in range(min(B, 64)) for v in range(V) if (v, b) not in cells]
    if len(free) >= 3 and n_idx >= 2:
        special["double"], special["shift"], special["zero"] = free[0], free[1], free[2]
        cells[free[0]] = [(0, 1), (n_idx - 1, p - 1)]
    return cells, special


def _represent(canon, p, width, rng):
    """The residues [V][n_idx][B] in the representations that must not change a verdict: vector 0 exact signed,
    vector 1 (when there is one) canonical, the rest mixed; then share - p / share + p in some cells, and for i64 raw
    values far outside (-p, p)."""
    V = canon.shape[0]
    signed = np.where(canon > p // 2, canon - p, canon)
    out = canon.copy()
    out[0] = signed[0]
    for v in range(2, V):
        pick = rng.integers(0, 2, canon[v].shape).astype(bool)
        out[v] = np.where(pick, signed[v], canon[v])
    lim = (1 << 31) if width == 32 else (1 << 63)
    kind = rng.integers(0, 16, canon.shape)
    minus, plus = out - p, out + p
    out = np.where((kind == 1) & (minus >= -lim), minus, out)
    out = np.where((kind == 2) & (plus < lim), plus, out)
    if width == 64:
        q_far = (1 << 30) + 12345
        out = np.where(kind == 3, canon + q_far * p, out)
        out = np.where(kind == 4, canon - q_far * p, out)
        # the least value >= i64::MIN and the greatest <= i64::MAX of each residue class
        near_min = np.int64(I64_MIN) + (canon - (I64_MIN % p)) % p
        near_max = np.int64((1 << 63) - 1) - ((((1 << 63) - 1) % p) - canon) % p
        out = np.where(kind == 5, near_min, out)
        out = np.where(kind == 6, near_max, out)
    assert (out % p == canon).all()
    return out


def build_case(name, n_idx, V, B, width, seed=0):
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, D = _oracle_rows(name, V, B)
    rng = np.random.default_rng(seed + 17 * n_idx + B)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    canon = rows[0][:, idx, :] % p
    cells, special = _plants(n_idx, V, B, p)
    for (v, b), errs in cells.items():
        for j, e in errs:
            canon[v, j, b] = (canon[v, j, b] + e) % p
    if special:
        v, b = special["shift"]
        canon[v, :, b] = (canon[v, :, b] + 7) % p
        v, b = special["zero"]
        canon[v, :, b] = 0
    shares = _represent(canon, p, width, rng)
    return sch, idx, D, shares, cells, special


class Dev:
    """Device buffers of one call: shares, and the verdict between guard words."""

    def __init__(self, shares, width, V, B):
        import torch
        self.torch = torch
        dt = np.int32 if width == 32 else np.int64
        assert (shares >= np.iinfo(dt).min).all() and (shares <= np.iinfo(dt).max).all()
        self.shares = torch.from_numpy(np.ascontiguousarray(shares.astype(dt))).cuda()
        self.words = V * B
        self.buf = torch.from_numpy(np.full(self.words + 2 * GUARD, SENT, np.uint16).view(np.int16)).cuda()
        self.verdict_ptr = self.buf.data_ptr() + 2 * GUARD

    def whole(self):
        self.torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint16)

    def expect(self, verdict):
        return np.concatenate([np.full(GUARD, SENT, np.uint16), np.asarray(verdict, np.uint16).reshape(-1),
                               np.full(GUARD, SENT, np.uint16)])


def _call(engine, sch, D, idx, V, dev, width, verdict=True):
    fn = engine.packed_check32_dev if width == 32 else engine.packed_check_dev
    return fn(sch, D, idx, V, dev.shares.data_ptr(), dev.verdict_ptr if verdict else None)


def _expected_record(n_idx, bad, r):
    path = E.CHECK_PATH_REGISTERS if n_idx <= 32 else E.CHECK_PATH_LOOPED
    bucket = 0 if n_idx > 32 else 8 if n_idx <= 8 else 16 if n_idx <= 16 else 32
    return E.CheckLaunch(path, bucket, bad if r >= 2 else 0, 0)


def _matrix():
    cases = []
    for name, sch in SCHEMES.items():
        kt, n = _kt(sch), sch.share_count
        ns = sorted({x for x in (kt, kt + 1, kt + 2, kt + 3, 8, 9, 16, 17, 32, 33, n) if kt <= x <= n})
        for i, n_idx in enumerate(ns):
            cases.append((name, n_idx, PM.V, PM.B_ODD if i % 2 else PM.B_EVEN))
    for name, n_idx in (("config", 18), ("n80", 33), ("small_p", 9), ("full_loop", 8)):
        cases += [(name, n_idx, 1, B) for B in (1, 255, 256, 257)]
    return cases


MATRIX = _matrix()


def test_the_matrix_reaches_every_edge():
    seen = {(n_idx) for _, n_idx, _, _ in MATRIX}
    assert {8, 9, 16, 17, 32, 33, 26, 80} <= seen
    for name, sch in SCHEMES.items():
        kt = _kt(sch)
        mine = {n_idx for nm, n_idx, _, _ in MATRIX if nm == name}
        assert {kt, kt + 1, sch.share_count} <= mine
        if sch.share_count >= kt + 3:
            assert {kt + 2, kt + 3} <= mine


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx,V,B", MATRIX, ids=[f"{a}-from{b}-V{c}-B{d}" for a, b, c, d in MATRIX])
def test_check_matches_the_model(engine, name, n_idx, V, B, width):
    sch, idx, D, shares, cells, special = build_case(name, n_idx, V, B, width)
    want_v, r, bad, first, blame = M.summary(sch, idx, shares)
    # what the definitions say about the planted cells, independent of the model
    for (v, b), errs in cells.items():
        if r == 0:
            assert want_v[v, b] == 0
        elif r == 1:
            assert want_v[v, b] == M.UNLOCATED
        elif len(errs) == 1:
            assert want_v[v, b] == errs[0][0] + 1
        elif r >= 3:
            assert want_v[v, b] == M.UNLOCATED
    if special:
        assert want_v[special["zero"]] == 0
        assert want_v[special["shift"]] == (0 if r == 0 else M.UNLOCATED)
    planted = len(cells) + (1 if special else 0)
    # (with r == 1 the batch with two errors may be a codeword again: the model decides)
    assert bad == 0 if r == 0 else planted - 1 <= bad <= planted if r == 1 else bad == planted
    if r >= 2 and B >= 64:
        assert all(x >= 1 for x in blame), blame            # every clerk position is blamed once across the run

    dev = Dev(shares, width, V, B)
    before = engine.packed_check_last_launch()
    got = _call(engine, sch, D, idx, V, dev, width)
    assert np.array_equal(dev.whole(), dev.expect(want_v))
    assert got == E.ShareCheck(r, bad, first, blame)
    assert engine.packed_check_last_launch() == (before if r == 0 else _expected_record(n_idx, bad, r))
    # verdict == NULL: the same counts
    assert _call(engine, sch, D, idx, V, dev, width, verdict=False) == got
    assert np.array_equal(dev.whole(), dev.expect(want_v))


@pytest.mark.parametrize("width", (64, 32))
def test_clean_shares_are_consistent_in_every_representation(engine, width):
    name, n_idx, V, B = "config", 26, PM.V, PM.B_ODD
    sch = SCHEMES[name]
    rows, D = _oracle_rows(name, V, B)
    rng = np.random.default_rng(5)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    shares = _represent(rows[0][:, idx, :] % sch.prime_modulus, sch.prime_modulus, width, rng)
    dev = Dev(shares, width, V, B)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert got == E.ShareCheck(n_idx - _kt(sch), 0, E.CHECK_NO_BAD, [0] * n_idx)
    assert np.array_equal(dev.whole(), dev.expect(np.zeros(V * B, np.uint16)))
    assert engine.packed_check_last_launch() == E.CheckLaunch(E.CHECK_PATH_REGISTERS, 32, 0, 0)


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx", (("config", 18), ("n80", 40)))
def test_a_whole_wrong_row_is_blamed_with_and_without_log_overflow(engine, monkeypatch, name, n_idx, width):
    """One clerk's row replaced by the same clerk's row of another participant: every batch is bad and located."""
    V, B, pos = PM.V, 257, 5
    sch = SCHEMES[name]
    rows, D = _oracle_rows(name, V, B)
    idx = list(range(3, 3 + n_idx))
    shares = rows[0][:, idx, :].copy()
    shares[:, pos, :] = rows[1][:, idx[pos], :]
    want_v, r, bad, first, blame = M.summary(sch, idx, shares)
    assert bad == V * B and first == 0 and blame[pos] == V * B and (want_v == pos + 1).all()
    outs = []
    for cap in (None, "100"):
        if cap is None:
            monkeypatch.delenv("SDA_CHECK_LOG_CAP", raising=False)
        else:
            monkeypatch.setenv("SDA_CHECK_LOG_CAP", cap)
        dev = Dev(shares, width, V, B)
        got = _call(engine, sch, D, idx, V, dev, width)
        rec = engine.packed_check_last_launch()
        assert rec.overflowed == (0 if cap is None else 1) and rec.located == V * B
        assert _call(engine, sch, D, idx, V, dev, width, verdict=False) == got
        outs.append((got, dev.whole().copy()))
    assert outs[0][0] == outs[1][0] == E.ShareCheck(r, bad, first, blame)
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], dev.expect(want_v))


@pytest.mark.parametrize("width", (64, 32))
def test_overflow_with_few_bad_batches_walks_every_batch(engine, monkeypatch, width):
    """More bad batches than a shrunken log holds, most batches consistent: the full pass skips the consistent ones."""
    name, n_idx, V, B = "config", 17, PM.V, PM.B_EVEN
    sch, idx, D, shares, cells, special = build_case(name, n_idx, V, B, width, seed=3)
    want_v, r, bad, first, blame = M.summary(sch, idx, shares)
    assert r == 2 and bad > 4
    monkeypatch.setenv("SDA_CHECK_LOG_CAP", "4")
    dev = Dev(shares, width, V, B)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert got == E.ShareCheck(r, bad, first, blame)
    assert np.array_equal(dev.whole(), dev.expect(want_v))
    assert engine.packed_check_last_launch() == E.CheckLaunch(E.CHECK_PATH_REGISTERS, 32, V * B, 1)


def test_secret_check_equals_the_device_form_and_keeps_reconstructs_statuses(engine):
    name, n_idx, B = "config", 18, 257
    sch, idx, D, shares, cells, special = build_case(name, n_idx, 1, B, 64)
    want_v, r, bad, first, blame = M.summary(sch, idx, shares)
    got, verdict = engine.secret_check(sch, D, list(zip(idx, shares[0])))
    assert got == E.ShareCheck(r, bad, first, blame) and np.array_equal(verdict, want_v[0])
    assert engine.secret_check(sch, D, list(zip(idx, shares[0])), want_verdict=False) == (got, None)
    # ragged rows, too few rows, repeated indices: sda_secret_reconstruct's statuses
    ragged = [(i, row if j != 2 else row[: B - 1]) for j, (i, row) in enumerate(zip(idx, shares[0]))]
    few = list(zip(idx, shares[0]))[: _kt(sch) - 1]
    few_ragged = [(i, row if j else row[:0]) for j, (i, row) in enumerate(few)]
    for rows_ in (ragged, few, few_ragged):
        with pytest.raises(E.SdaError) as a:
            engine.secret_reconstruct(sch, D, rows_)
        with pytest.raises(E.SdaError) as b:
            engine.secret_check(sch, D, rows_)
        assert a.value.status == b.value.status
    with pytest.raises(E.SdaError) as e:
        engine.secret_check(sch, D, [(idx[0], row) for row in shares[0]])
    assert e.value.status == UNSUPPORTED
    # Additive: nothing to check
    add = S.Additive(3, 433)
    got, verdict = engine.secret_check(add, 4, [(i, np.arange(4)) for i in range(3)])
    assert got == E.ShareCheck(0, 0, E.CHECK_NO_BAD, [0, 0, 0]) and not verdict.any() and verdict.size == 4
    with pytest.raises(E.SdaError) as e:
        engine.secret_check(add, 4, [(0, np.arange(4)), (1, np.arange(3))])
    assert e.value.status == 4


def test_status_matrix_follows_the_reveal_and_a_failing_call_writes_nothing(engine):
    import torch
    name, V, B = "config", 2, 40
    sch = SCHEMES[name]
    rows, D = _oracle_rows(name, V, B)
    kt, n = _kt(sch), sch.share_count
    dev = Dev(rows[0][:, :18, :], 64, V, B)
    out = torch.zeros(V * D, dtype=torch.int64, device="cuda")
    good = list(range(18))
    first = engine.packed_check_dev(sch, D, good, V, dev.shares.data_ptr(), dev.verdict_ptr)
    assert first.bad_batches == 0
    clean, rec = dev.whole().copy(), engine.packed_check_last_launch()
    bad_root = S.PackedShamir(sch.secret_count, n, sch.privacy_threshold(), sch.prime_modulus, sch.omega_secrets, 1)
    even_p = S.PackedShamir(sch.secret_count, n, sch.privacy_threshold(), sch.prime_modulus - 1, sch.omega_secrets,
                            sch.omega_shares)
    failing = [  # (scheme, dimension, indices, n_vectors): single faults, then pairs that fix the order of the checks
        (sch, D, good[: kt - 1], V),                       # too few shares
        (sch, D, list(range(1024)), V),                    # more than 1023 shares
        (sch, D, good, 65536),                             # too many vectors
        (even_p, D, good, V), (bad_root, D, good, V),      # whatever check_packed refuses
        (even_p, D, good[: kt - 1], V),                    # scheme before share count
        (sch, D, good[: kt - 1], 65536),                   # share count before vector count
        (sch, D, list(range(1024)), 65536),
        (sch, D, [0] * 18, V),                             # repeated indices
        (sch, D, good[:16] + [3, 4], V),
    ]
    for s, d, idx, nv in failing:
        codes = []
        for call in (lambda: engine.packed_reconstruct_dev(s, d, idx, nv, dev.shares.data_ptr(), out.data_ptr(),
                                                           E.REVEAL_CANONICAL),
                     lambda: engine.packed_check_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.verdict_ptr),
                     lambda: engine.packed_check32_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.verdict_ptr)):
            try:
                call()
                codes.append(0)
            except E.SdaError as e:
                codes.append(e.status)
        assert codes[0] != 0 and codes[0] == codes[1] == codes[2], (codes, d, len(idx), nv)
        assert np.array_equal(dev.whole(), clean) and engine.packed_check_last_launch() == rec
    with pytest.raises(E.SdaError) as e:
        engine.packed_check_dev(sch, D, good[: kt - 1], V, dev.shares.data_ptr(), dev.verdict_ptr)
    assert e.value.status == NOT_ENOUGH
    with pytest.raises(E.SdaError) as e:
        engine.packed_check_dev(sch, D, [0] * 18, V, dev.shares.data_ptr(), dev.verdict_ptr)
    assert e.value.status == UNSUPPORTED
    # a failing call leaves the host outputs alone
    s = sch.c()
    idx = np.asarray(good[: kt - 1], np.uint64)
    vals = [C.c_uint64(111), C.c_uint64(222), C.c_uint64(333)]
    blame = np.full(18, 444, np.uint64)
    st = engine.lib.sda_packed_check_dev(engine.h, C.byref(s), D, idx.ctypes.data_as(C.POINTER(C.c_uint64)), idx.size,
                                         V, dev.shares.data_ptr(), dev.verdict_ptr, C.byref(vals[0]),
                                         C.byref(vals[1]), C.byref(vals[2]),
                                         blame.ctypes.data_as(C.POINTER(C.c_uint64)), None)
    assert st == NOT_ENOUGH and [v.value for v in vals] == [111, 222, 333] and (blame == 444).all()
    st = engine.lib.sda_packed_check_dev(engine.h, C.byref(s), D, idx.ctypes.data_as(C.POINTER(C.c_uint64)), 18, V,
                                         dev.shares.data_ptr(), dev.verdict_ptr, None, C.byref(vals[1]),
                                         C.byref(vals[2]), blame.ctypes.data_as(C.POINTER(C.c_uint64)), None)
    assert st == INVALID
    # SDA_OK with nothing launched: r == 0, dimension == 0, no vectors, an Additive scheme; verdict zero-filled
    assert np.array_equal(dev.whole(), clean) and engine.packed_check_last_launch() == rec
    dirty = Dev(rows[0][:, :kt, :], 64, V, B)
    assert engine.packed_check_dev(sch, D, good[:kt], V, dirty.shares.data_ptr(), dirty.verdict_ptr) == \
        E.ShareCheck(0, 0, E.CHECK_NO_BAD, [0] * kt)
    assert np.array_equal(dirty.whole(), dirty.expect(np.zeros(V * B, np.uint16)))
    dirty = Dev(rows[0][:, :18, :], 64, V, B)
    assert engine.packed_check_dev(sch, 0, good, V, dirty.shares.data_ptr(), dirty.verdict_ptr) == \
        E.ShareCheck(3, 0, E.CHECK_NO_BAD, [0] * 18)
    assert engine.packed_check_dev(sch, 0, good[:3], V, dirty.shares.data_ptr(), dirty.verdict_ptr).redundancy == 0
    assert engine.packed_check_dev(sch, D, good, 0, dirty.shares.data_ptr(), dirty.verdict_ptr) == \
        E.ShareCheck(3, 0, E.CHECK_NO_BAD, [0] * 18)
    assert (dirty.whole() == SENT).all()
    add = S.Additive(18, 433)
    small = Dev(rows[0][:1, :18, :], 64, 1, 18 * B)         # verdict [n_vectors][dimension] for an Additive scheme
    assert engine.packed_check_dev(add, 18 * B, good, 1, small.shares.data_ptr(), small.verdict_ptr) == \
        E.ShareCheck(0, 0, E.CHECK_NO_BAD, [0] * 18)
    assert np.array_equal(small.whole(), small.expect(np.zeros(18 * B, np.uint16)))
    assert engine.packed_check_last_launch() == rec


def test_record_is_all_zeros_before_the_first_check():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    e = E.Engine(0)
    try:
        assert e.packed_check_last_launch() == E.CheckLaunch(0, 0, 0, 0)
    finally:
        e.close()
