"""GPU: the checked reveal (sda_packed_reveal_checked_dev, sda_packed_reveal_checked32_dev,
sda_secret_reconstruct_checked) against tests/checked_reveal_model.py.

Shares come from the oracle's packed_generate (two participants per scheme and shape, built once and shared).  A case
takes the rows of n_idx clerks (shuffled, non-contiguous indices), plants its faults on the residues, writes every
value in one of the representations a clerk may send (tests/test_gpu_share_check.py: exact signed, canonical, mixed,
share - p and share + p, and for i64 raw values far outside (-p, p); _represent_for says what the composed path
leaves out) and compares the whole guarded `out` and verdict buffers, the counts, first_bad, blame and the launch
record with the model, and the verdict and counts with sda_packed_check_dev on the same arguments.  What the definitions promise without the model -- a single wrong share
with r >= 2 costs nothing: the batch's secrets are the fault-free ones -- is asserted besides.

Shapes: B in {1, 63, 64, 65, 257, 1030} (even and odd, one tile and several, lanes 0 and 63 of a wave), 1 and 3
vectors, an odd dimension that k does not divide (a cut tail batch; vector 1 then starts 8 bytes off a 16-byte
boundary), out 16-byte aligned and offset by 8.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import checked_reveal_model as R
from tests import packed_matrix_cases as PM
from tests import share_check_model as M
from tests.test_checked_reveal_model import SCHEMES, kt_of
from tests.test_gpu_share_check import GUARD, SENT, _represent

pytestmark = pytest.mark.gpu

OUT_GUARD = 2                  # i64 words on each side of `out`: 16 bytes, so the guard keeps the alignment
OUT_SENT = -0x0123456789ABCDEF
UNSUPPORTED, INVALID, NOT_ENOUGH = 66, 65, 6
BS = (1, 63, 64, 65, 257, 1030)


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, V, B):
    """([2 participants][V][n][B] exact signed shares, [2][V][D] canonical secrets, D) from the oracle."""
    from oracle import oracle as O
    sch = SCHEMES[name]
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    D = PM.dimension(B, k)
    rng = np.random.default_rng(7000 * V + B)
    rows, secrets = np.empty((2, V, n, B), np.int64), np.empty((2, V, D), np.int64)
    for a in range(2):
        for v in range(V):
            secrets[a, v] = rng.integers(0, p, D)
            rows[a, v] = O.packed_generate(R._params(O, sch), secrets[a, v], rng.integers(0, p - 1, B * t))
    rows.setflags(write=False)
    secrets.setflags(write=False)
    return rows, secrets, D


def _plant(canon, p, r):
    """Plants on canon [V][n_idx][B] in place: one wrong share at every position in turn, in scattered batches that
    start with batch 0, the last batch overall and lanes 0 / 63 of a wave; then (when cells are left) one batch with
    two wrong shares and one with every share moved (a polynomial with f(1) != 0).  Returns {(v, b): [positions]} of
    the single and double faults, and the moved cell or None."""
    V, n_idx, B = canon.shape
    errs = (1, p - 1, (p - 1) // 2)
    order = [(0, 0), (V - 1, B - 1), (0, 63), (V - 1, 64), (0, 127), (V - 1, 128), (V - 1, 0), (0, B - 1)]
    order += [((j + 1) % V, (7 * j + 3) % B) for j in range(4 * n_idx)]
    free = []
    for c in order:
        if c[1] < B and c not in free:
            free.append(c)
    cells = {}
    for j in range(n_idx):
        if not free:
            break
        v, b = free.pop(0)
        canon[v, j, b] = (canon[v, j, b] + errs[j % 3]) % p
        cells[(v, b)] = [j]
    shift = None
    if len(free) >= 2 and n_idx >= 2:
        v, b = free.pop(0)
        canon[v, 0, b] = (canon[v, 0, b] + 1) % p
        canon[v, n_idx - 1, b] = (canon[v, n_idx - 1, b] + p - 1) % p
        cells[(v, b)] = [0, n_idx - 1]
        shift = free.pop(0)
        canon[shift[0], :, shift[1]] = (canon[shift[0], :, shift[1]] + 7) % p
    return cells, shift


def _composed(sch, n_idx):
    return n_idx > 32 or sch.secret_count > 8


def _represent_for(sch, n_idx, canon, p, width, rng):
    """_represent, except that on the composed path raw values beyond 2^62 in magnitude go back to their residues:
    a consistent batch is there what sda_packed_reconstruct_dev CANONICAL returns, and past 32 shares that reveal runs
    tss' Newton steps in wrapping i64 arithmetic, whose differences of two such values wrap (the oracle's do too).
    Raw values up to 2^61 in magnitude, far outside (-p, p), stay."""
    out = _represent(canon, p, width, rng)
    if _composed(sch, n_idx):
        out = np.where(np.abs(out.astype(np.float64)) > float(1 << 62), canon, out)
        assert (out % p == canon).all() and (np.abs(out) > (1 << 60)).any() == (width == 64)
    return out


def _wrong_row(rows, clerk, p):
    """[V][B]: clerk's row of the other participant -- moved by one wherever it happens to be the first participant's
    share mod p (one batch in p: several at p = 433), so that it is wrong in every batch."""
    wrong, right = rows[1][:, clerk, :].copy(), rows[0][:, clerk, :]
    same = (wrong - right) % p == 0
    wrong[same] += np.where(wrong[same] < p - 1, 1, -1)
    assert ((wrong - right) % p != 0).all() and (np.abs(wrong) < p).all()
    return wrong


def _indices(sch, n_idx, seed):
    return np.random.default_rng(seed).permutation(sch.share_count)[:n_idx].tolist()


class Dev:
    """Device buffers of one call: the shares, and `out` and the verdict between guard words."""

    def __init__(self, shares, width, V, B, D, off=0):
        import torch
        self.torch = torch
        dt = np.int32 if width == 32 else np.int64
        assert (shares >= np.iinfo(dt).min).all() and (shares <= np.iinfo(dt).max).all()
        self.shares = torch.from_numpy(np.ascontiguousarray(shares.astype(dt))).cuda()
        self.vbuf = torch.from_numpy(np.full(V * B + 2 * GUARD, SENT, np.uint16).view(np.int16)).cuda()
        self.verdict_ptr = self.vbuf.data_ptr() + 2 * GUARD
        self.lead = OUT_GUARD + (1 if off else 0)
        self.obuf = torch.full((self.lead + V * D + OUT_GUARD,), OUT_SENT, dtype=torch.int64, device="cuda")
        self.out_ptr = self.obuf.data_ptr() + 8 * self.lead
        assert self.out_ptr % 16 == (8 if off else 0)

    def verdict(self):
        self.torch.cuda.synchronize()
        return self.vbuf.cpu().numpy().view(np.uint16)

    def out(self):
        self.torch.cuda.synchronize()
        return self.obuf.cpu().numpy()

    def expect_verdict(self, verdict):
        g = np.full(GUARD, SENT, np.uint16)
        return np.concatenate([g, np.asarray(verdict, np.uint16).reshape(-1), g])

    def expect_out(self, out):
        return np.concatenate([np.full(self.lead, OUT_SENT, np.int64), np.asarray(out, np.int64).reshape(-1),
                               np.full(OUT_GUARD, OUT_SENT, np.int64)])


def _call(engine, sch, D, idx, V, dev, width, verdict=True):
    fn = engine.packed_reveal_checked32_dev if width == 32 else engine.packed_reveal_checked_dev
    return fn(sch, D, idx, V, dev.shares.data_ptr(), dev.out_ptr, dev.verdict_ptr if verdict else None)


def _check_call(engine, sch, D, idx, V, dev, width):
    fn = engine.packed_check32_dev if width == 32 else engine.packed_check_dev
    return fn(sch, D, idx, V, dev.shares.data_ptr(), None)


def _record(sch, n_idx, verdict, bad, overflowed=0):
    k, kt = sch.secret_count, kt_of(sch)
    r = n_idx - kt
    if n_idx <= 32 and k <= 8:
        bucket = 8 if n_idx <= 8 else 16 if n_idx <= 16 else 32
        fixed = int(np.count_nonzero((verdict >= 1) & (verdict <= kt))) if r >= 2 else 0
        return E.RepairLaunch(E.REPAIR_PATH_FUSED, bucket, fixed, overflowed if r >= 2 else 0)
    return E.RepairLaunch(E.REPAIR_PATH_COMPOSED, 0, bad, overflowed)


def _matrix():
    """(scheme, n_idx, V, B, out offset): every clerk count of the issue's list, the shapes taken in turn."""
    pairs = [("b8", n) for n in (5, 6, 7, 8)] + [("b16", n) for n in range(10, 17)] + [("config", 17), ("config", 26)]
    pairs += [("b8", 3), ("b8", 4), ("full_loop", 7), ("full_loop", 8), ("config", 15), ("config", 16)]   # r = 0, 1
    cases = []
    for i, (name, n_idx) in enumerate(pairs):
        cases.append((name, n_idx, 3 if i % 2 else 1, BS[i % len(BS)], 8 * ((i // 2) % 2)))
    cases += [("config", 26, 3, 1030, 8), ("config", 17, 1, 1, 0), ("b8", 8, 3, 1030, 0), ("b16", 16, 1, 63, 8),
              ("n80", 40, 3, 257, 0), ("n80", 40, 1, 64, 8), ("n80", 16, 1, 65, 0)]
    return cases


MATRIX = _matrix()


def test_the_matrix_reaches_every_shape_and_path():
    assert {c[3] for c in MATRIX} == set(BS) and {c[2] for c in MATRIX} == {1, 3} and {c[4] for c in MATRIX} == {0, 8}
    assert {(c[0], c[1]) for c in MATRIX} >= {("b8", 5), ("b8", 8), ("b16", 10), ("b16", 16), ("config", 17),
                                               ("config", 26), ("n80", 40)}
    r_of = {c[1] - kt_of(SCHEMES[c[0]]) for c in MATRIX}
    assert {0, 1, 2, 3} <= r_of


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx,V,B,off", MATRIX, ids=[f"{a}-from{b}-V{c}-B{d}-off{e}" for a, b, c, d, e in MATRIX])
def test_checked_reveal_matches_the_model(engine, oracle, name, n_idx, V, B, off, width):
    sch = SCHEMES[name]
    p, k, kt = sch.prime_modulus, sch.secret_count, kt_of(sch)
    r = n_idx - kt
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 17 * n_idx + B)
    canon = rows[0][:, idx, :] % p
    cells, shift = _plant(canon, p, r)
    shares = _represent_for(sch, n_idx, canon, p, width, np.random.default_rng(n_idx + B))
    want, verdict, wr, bad, first, blame = R.reveal(oracle, sch, D, idx, shares)
    # what the definitions say about the planted cells, independent of the model
    assert wr == r
    for (v, b), pos in cells.items():
        lo, hi = b * k, min((b + 1) * k, D)
        if r >= 2 and len(pos) == 1:
            assert verdict[v, b] == pos[0] + 1 and np.array_equal(want[v, lo:hi], secrets[0, v, lo:hi])
        elif (r == 1 and len(pos) == 1) or (r >= 3 and len(pos) == 2):   # (r == 1, two faults: may be a codeword)
            assert verdict[v, b] == M.UNLOCATED
    if shift:
        assert verdict[shift] == (0 if r == 0 else M.UNLOCATED)
    untouched = np.ones((V, B), bool)
    for v, b in list(cells) + ([shift] if shift else []):
        untouched[v, b] = False
    assert not verdict[untouched].any()
    clean = np.repeat(untouched, k, axis=1)[:, :D]
    assert np.array_equal(want[clean], secrets[0][clean])

    dev = Dev(shares, width, V, B, D, off)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert np.array_equal(dev.verdict(), dev.expect_verdict(verdict))
    assert np.array_equal(dev.out(), dev.expect_out(want))
    assert got == E.ShareCheck(r, bad, first, blame)
    assert engine.packed_reveal_checked_last_launch() == _record(sch, n_idx, verdict, bad)
    # the share check on the same arguments: the same counts
    assert _check_call(engine, sch, D, idx, V, dev, width) == got
    # verdict == NULL: the same secrets and counts
    dev2 = Dev(shares, width, V, B, D, off)
    assert _call(engine, sch, D, idx, V, dev2, width, verdict=False) == got
    assert np.array_equal(dev2.out(), dev2.expect_out(want)) and (dev2.verdict() == SENT).all()


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx,V,B,off", [("b8", 7, 3, 257, 8), ("b16", 12, 1, 1030, 0), ("config", 26, 3, 65, 0),
                                                ("config", 15, 1, 64, 8), ("n80", 40, 1, 257, 0)])
def test_consistent_shares_give_the_canonical_reveal_byte_for_byte(engine, name, n_idx, V, B, off, width):
    import torch
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 5 + n_idx)
    shares = _represent_for(sch, n_idx, rows[0][:, idx, :] % p, p, width, np.random.default_rng(B))
    dev = Dev(shares, width, V, B, D, off)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert got == E.ShareCheck(n_idx - kt_of(sch), 0, E.CHECK_NO_BAD, [0] * n_idx)
    assert got == _check_call(engine, sch, D, idx, V, dev, width)
    plain = torch.full((V * D,), OUT_SENT, dtype=torch.int64, device="cuda")
    fn = engine.packed_reconstruct32_dev if width == 32 else engine.packed_reconstruct_dev
    fn(sch, D, idx, V, dev.shares.data_ptr(), plain.data_ptr(), E.REVEAL_CANONICAL)
    torch.cuda.synchronize()
    assert np.array_equal(dev.out(), dev.expect_out(plain.cpu().numpy()))
    assert np.array_equal(plain.cpu().numpy().reshape(V, D), secrets[0])
    assert np.array_equal(dev.verdict(), dev.expect_verdict(np.zeros(V * B, np.uint16)))
    assert engine.packed_reveal_checked_last_launch() == _record(sch, n_idx, np.zeros(1, np.uint16), 0)


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx,pos", (("config", 26, 5), ("config", 17, 16), ("b8", 6, 0), ("n80", 40, 9)))
def test_a_whole_wrong_row_costs_nothing_with_and_without_log_overflow(engine, monkeypatch, name, n_idx, pos, width):
    """One clerk's row replaced by the same clerk's row of another participant: every batch is bad, located at that
    clerk, and every secret is the fault-free one -- the same with SDA_CHECK_LOG_CAP=4."""
    V, B = 3, 257
    sch = SCHEMES[name]
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 3 + n_idx)
    shares = rows[0][:, idx, :].copy()
    shares[:, pos, :] = _wrong_row(rows, idx[pos], sch.prime_modulus)
    blame = [0] * n_idx
    blame[pos] = V * B
    verdict = np.full(V * B, pos + 1, np.uint16)
    for cap in (None, "4"):
        if cap is None:
            monkeypatch.delenv("SDA_CHECK_LOG_CAP", raising=False)
        else:
            monkeypatch.setenv("SDA_CHECK_LOG_CAP", cap)
        for with_verdict in (True, False):
            dev = Dev(shares, width, V, B, D)
            got = _call(engine, sch, D, idx, V, dev, width, verdict=with_verdict)
            assert got == E.ShareCheck(n_idx - kt_of(sch), V * B, 0, blame)
            assert np.array_equal(dev.out(), dev.expect_out(secrets[0]))
            if with_verdict:
                assert np.array_equal(dev.verdict(), dev.expect_verdict(verdict))
            rec = engine.packed_reveal_checked_last_launch()
            assert rec == _record(sch, n_idx, verdict, V * B, 0 if cap is None else 1)
            assert rec.overflowed == (0 if cap is None else 1)
        assert _check_call(engine, sch, D, idx, V, dev, width) == got


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx", (("config", 17), ("b8", 5), ("b16", 9)))
def test_two_flaky_clerks_in_disjoint_batches_at_r2_cost_nothing(engine, oracle, name, n_idx, width):
    """Two clerks each wrong in different batches, r = 2: every batch has one error and is located, so every secret
    is the fault-free one.  Dropping both clerks would leave no redundancy at all."""
    V, B = 3, 65
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    assert n_idx - kt == 2
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 9 + n_idx)
    a, b = 1, n_idx - 1                                      # a basis clerk and a check clerk
    shares = rows[0][:, idx, :].copy()
    shares[:, a, 0::3] = _wrong_row(rows, idx[a], p)[:, 0::3]
    shares[:, b, 1::3] = _wrong_row(rows, idx[b], p)[:, 1::3]
    verdict = np.zeros((V, B), np.uint16)
    verdict[:, 0::3], verdict[:, 1::3] = a + 1, b + 1
    changed = (shares != rows[0][:, idx, :]).any(axis=1)
    assert np.array_equal(changed, verdict != 0)
    want, mv, r, bad, first, blame = R.reveal(oracle, sch, D, idx, shares)
    assert np.array_equal(mv, verdict) and np.array_equal(want, secrets[0]) and r == 2
    dev = Dev(shares, width, V, B, D)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert got == E.ShareCheck(2, bad, 0, blame) and blame[a] == V * len(range(0, B, 3))
    assert np.array_equal(dev.out(), dev.expect_out(secrets[0]))
    assert np.array_equal(dev.verdict(), dev.expect_verdict(verdict))
    assert engine.packed_reveal_checked_last_launch() == _record(sch, n_idx, verdict, bad)


def test_host_form_equals_the_device_form_and_keeps_the_checks_statuses(engine, oracle):
    for name, n_idx, B in (("config", 18, 257), ("n80", 40, 65), ("full_loop", 8, 63)):
        sch = SCHEMES[name]
        p = sch.prime_modulus
        rows, secrets, D = _oracle_rows(name, 1, B)
        idx = _indices(sch, n_idx, 11)
        canon = rows[0][:, idx, :] % p
        _plant(canon, p, n_idx - kt_of(sch))
        shares = _represent_for(sch, n_idx, canon, p, 64, np.random.default_rng(2))
        want, verdict, r, bad, first, blame = R.reveal(oracle, sch, D, idx, shares)
        out, got, ver = engine.secret_reconstruct_checked(sch, D, list(zip(idx, shares[0])))
        assert np.array_equal(out, want[0]) and np.array_equal(ver, verdict[0])
        assert got == E.ShareCheck(r, bad, first, blame)
        assert engine.packed_reveal_checked_last_launch() == _record(sch, n_idx, verdict, bad)
        out2, got2, ver2 = engine.secret_reconstruct_checked(sch, D, list(zip(idx, shares[0])), want_verdict=False)
        assert np.array_equal(out2, out) and got2 == got and ver2 is None
    # ragged rows, too few rows, repeated indices: sda_secret_check's statuses
    sch, B = SCHEMES["config"], 257
    rows, secrets, D = _oracle_rows("config", 1, B)
    idx = list(range(18))
    full = list(zip(idx, rows[0][0, idx, :]))
    ragged = [(i, row if j != 2 else row[: B - 1]) for j, (i, row) in enumerate(full)]
    few = full[: kt_of(sch) - 1]
    few_ragged = [(i, row if j else row[:0]) for j, (i, row) in enumerate(few)]
    for rows_ in (ragged, few, few_ragged, [(idx[0], row) for _, row in full]):
        with pytest.raises(E.SdaError) as a:
            engine.secret_check(sch, D, rows_)
        with pytest.raises(E.SdaError) as b:
            engine.secret_reconstruct_checked(sch, D, rows_)
        assert a.value.status == b.value.status
    with pytest.raises(E.SdaError) as e:
        engine.secret_reconstruct_checked(S.Additive(3, 433), 4, [(i, np.arange(4)) for i in range(3)])
    assert e.value.status == UNSUPPORTED
    out, got, ver = engine.secret_reconstruct_checked(sch, 0, full)
    assert out.size == 0 and got == E.ShareCheck(3, 0, E.CHECK_NO_BAD, [0] * 18) and ver.size == 0


def test_status_matrix_follows_the_check_and_a_failing_call_writes_nothing(engine):
    name, V, B = "config", 2, 40
    sch = SCHEMES[name]
    rows, secrets, D = _oracle_rows(name, V, B)
    kt, n = kt_of(sch), sch.share_count
    good = list(range(18))
    dev = Dev(rows[0][:, :18, :], 64, V, B, D)
    first = _call(engine, sch, D, good, V, dev, 64)
    assert first == E.ShareCheck(3, 0, E.CHECK_NO_BAD, [0] * 18)
    assert np.array_equal(dev.out(), dev.expect_out(secrets[0]))
    clean_v, clean_o, rec = dev.verdict().copy(), dev.out().copy(), engine.packed_reveal_checked_last_launch()
    check_rec = engine.packed_check_last_launch()
    bad_root = S.PackedShamir(sch.secret_count, n, sch.privacy_threshold(), sch.prime_modulus, sch.omega_secrets, 1)
    even_p = S.PackedShamir(sch.secret_count, n, sch.privacy_threshold(), sch.prime_modulus - 1, sch.omega_secrets,
                            sch.omega_shares)
    failing = [  # (scheme, dimension, indices, n_vectors): single faults, then pairs that fix the order of the checks
        (sch, D, good[: kt - 1], V), (sch, D, list(range(1024)), V), (sch, D, good, 65536),
        (even_p, D, good, V), (bad_root, D, good, V), (even_p, D, good[: kt - 1], V),
        (sch, D, good[: kt - 1], 65536), (sch, D, list(range(1024)), 65536),
        (sch, D, [0] * 18, V), (sch, D, good[:16] + [3, 4], V),
    ]
    for s, d, idx, nv in failing:
        codes = []
        for call in (lambda: engine.packed_check_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.verdict_ptr),
                     lambda: engine.packed_reveal_checked_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.out_ptr,
                                                              dev.verdict_ptr),
                     lambda: engine.packed_reveal_checked32_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.out_ptr,
                                                                dev.verdict_ptr)):
            try:
                call()
                codes.append(0)
            except E.SdaError as e:
                codes.append(e.status)
        assert codes[0] != 0 and codes[0] == codes[1] == codes[2], (codes, d, len(idx), nv)
        assert np.array_equal(dev.verdict(), clean_v) and np.array_equal(dev.out(), clean_o)
        assert engine.packed_reveal_checked_last_launch() == rec
    for idx, status in ((good[: kt - 1], NOT_ENOUGH), ([0] * 18, UNSUPPORTED)):
        with pytest.raises(E.SdaError) as e:
            engine.packed_reveal_checked_dev(sch, D, idx, V, dev.shares.data_ptr(), dev.out_ptr, dev.verdict_ptr)
        assert e.value.status == status
    with pytest.raises(E.SdaError) as e:
        engine.packed_reveal_checked_dev(S.Additive(18, 433), D, good, V, dev.shares.data_ptr(), dev.out_ptr,
                                         dev.verdict_ptr)
    assert e.value.status == UNSUPPORTED
    # each NULL argument, through the C ABI; a failing call leaves the host outputs alone
    s = sch.c()
    idx = np.asarray(good, np.uint64)
    vals = [C.c_uint64(111), C.c_uint64(222), C.c_uint64(333)]
    blame = np.full(18, 444, np.uint64)
    u64p = C.POINTER(C.c_uint64)

    def raw(h=engine.h, sp=C.byref(s), ip=idx.ctypes.data_as(u64p), sh=dev.shares.data_ptr(), out=dev.out_ptr,
            r=C.byref(vals[0]), b=C.byref(vals[1]), f=C.byref(vals[2]), bl=blame.ctypes.data_as(u64p), n_idx=18):
        return engine.lib.sda_packed_reveal_checked_dev(h, sp, D, ip, n_idx, V, sh, out, dev.verdict_ptr, r, b, f, bl,
                                                        None)
    for kw in ({"h": None}, {"sp": None}, {"ip": None}, {"sh": None}, {"out": None}, {"r": None}, {"b": None},
               {"f": None}, {"bl": None}):
        assert raw(**kw) == INVALID, kw
    assert raw(n_idx=kt - 1) == NOT_ENOUGH
    assert [v.value for v in vals] == [111, 222, 333] and (blame == 444).all()
    assert np.array_equal(dev.verdict(), clean_v) and np.array_equal(dev.out(), clean_o)
    assert engine.packed_reveal_checked_last_launch() == rec and engine.packed_check_last_launch() == check_rec
    # SDA_OK with nothing launched: dimension == 0, no vectors
    dirty = Dev(rows[0][:, :18, :], 64, V, B, D)
    assert engine.packed_reveal_checked_dev(sch, 0, good, V, dirty.shares.data_ptr(), dirty.out_ptr,
                                            dirty.verdict_ptr) == E.ShareCheck(3, 0, E.CHECK_NO_BAD, [0] * 18)
    assert engine.packed_reveal_checked_dev(sch, 0, good[:3], V, dirty.shares.data_ptr(), dirty.out_ptr,
                                            dirty.verdict_ptr).redundancy == 0
    assert engine.packed_reveal_checked_dev(sch, D, good, 0, dirty.shares.data_ptr(), dirty.out_ptr,
                                            dirty.verdict_ptr) == E.ShareCheck(3, 0, E.CHECK_NO_BAD, [0] * 18)
    assert (dirty.verdict() == SENT).all() and (dirty.out() == OUT_SENT).all()
    assert engine.packed_reveal_checked_last_launch() == rec


def test_record_is_all_zeros_before_the_first_checked_reveal():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    e = E.Engine(0)
    try:
        assert e.packed_reveal_checked_last_launch() == E.RepairLaunch(0, 0, 0, 0)
    finally:
        e.close()


# ---- the one table of a (scheme, clerk set): shared by the share check and the checked reveal ----
def _new_engine():
    import torch
    torch.cuda.init()                                        # torch opens the device first (tests/conftest.py)
    return E.Engine(0)


def _run_on(eng, kind, sch, D, idx, shares, width):
    """One share check or checked reveal of `shares` [1][n_idx][B] on eng: everything the call hands back."""
    dev = Dev(shares, width, 1, shares.shape[2], D)
    if kind == "check":
        fn = eng.packed_check32_dev if width == 32 else eng.packed_check_dev
        got = fn(sch, D, idx, 1, dev.shares.data_ptr(), dev.verdict_ptr)
        return got, dev.verdict().copy(), dev.out().copy(), eng.packed_check_last_launch()
    got = _call(eng, sch, D, idx, 1, dev, width)
    return got, dev.verdict().copy(), dev.out().copy(), eng.packed_reveal_checked_last_launch()


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def _fresh(kind, sch, D, idx, shares, width):
    e = _new_engine()
    try:
        return _run_on(e, kind, sch, D, idx, shares, width)
    finally:
        e.close()


def _two_faults(name, n_idx, seed):
    """(indices, canonical shares [1][n_idx][65], D): a basis-position fault in batch 5 (position 2) and a
    check-position fault in the last batch (position n_idx - 1)."""
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, _, D = _oracle_rows(name, 1, 65)
    idx = _indices(sch, n_idx, seed)
    canon = rows[0][:, idx, :] % p
    canon[0, 1, 5] = (canon[0, 1, 5] + 1) % p
    canon[0, n_idx - 2, 64] = (canon[0, n_idx - 2, 64] + p - 1) % p
    return idx, canon, D


@pytest.mark.parametrize("name,n_idx,width", (("b8", 7, 64), ("n80", 40, 32), ("n80", 40, 64)))
def test_the_shared_table_serves_both_families_in_any_order(name, n_idx, width):
    sch = SCHEMES[name]
    assert n_idx - kt_of(sch) >= 2 and _composed(sch, n_idx) == (name == "n80")
    idx1, sh1, D = _two_faults(name, n_idx, 101)
    idx2, sh2, _ = _two_faults(name, n_idx, 202)
    assert idx1 != idx2
    eng = _new_engine()
    try:
        for kind, idx, sh in (("check", idx1, sh1), ("reveal", idx1, sh1), ("check", idx2, sh2), ("reveal", idx1, sh1)):
            got = _run_on(eng, kind, sch, D, idx, sh, width)
            assert _same(got, _fresh(kind, sch, D, idx, sh, width)), (kind, idx)
            blame = [0] * n_idx
            blame[1] = blame[n_idx - 2] = 1
            assert got[0] == E.ShareCheck(n_idx - kt_of(sch), 2, 5, blame)
            verdict = got[1][GUARD:-GUARD]
            assert verdict[5] == 2 and verdict[64] == n_idx - 1 and np.count_nonzero(verdict) == 2
    finally:
        eng.close()


def test_a_table_built_at_r0_carries_the_reveal_rows():
    import torch
    sch = SCHEMES["b8"]
    assert kt_of(sch) == 3
    rows, secrets, D = _oracle_rows("b8", 1, 65)
    idx = _indices(sch, 3, 303)
    shares = rows[0][:, idx, :]
    eng = _new_engine()
    try:
        dev = Dev(shares, 64, 1, 65, D)
        none = E.ShareCheck(0, 0, E.CHECK_NO_BAD, [0, 0, 0])
        assert eng.packed_check_dev(sch, D, idx, 1, dev.shares.data_ptr(), None) == none      # launches nothing
        assert eng.packed_check_last_launch() == E.CheckLaunch(0, 0, 0, 0)
        assert _call(eng, sch, D, idx, 1, dev, 64) == none
        plain = torch.full((D,), OUT_SENT, dtype=torch.int64, device="cuda")
        eng.packed_reconstruct_dev(sch, D, idx, 1, dev.shares.data_ptr(), plain.data_ptr(), E.REVEAL_CANONICAL)
        torch.cuda.synchronize()
        assert np.array_equal(dev.out(), dev.expect_out(plain.cpu().numpy()))
        assert np.array_equal(plain.cpu().numpy(), secrets[0, 0])
        assert eng.packed_reveal_checked_last_launch() == E.RepairLaunch(E.REPAIR_PATH_FUSED, 8, 0, 0)
    finally:
        eng.close()


def test_a_refused_call_leaves_the_cache_intact_across_families():
    sch = SCHEMES["b8"]
    idx, shares, D = _two_faults("b8", 7, 404)
    repeated = idx[:-1] + [idx[0]]
    eng = _new_engine()
    try:
        for valid, refused, message in (("check", "reveal", "the checked reveal needs distinct clerk indices"),
                                        ("reveal", "check", "the share check needs distinct clerk indices")):
            first = _run_on(eng, valid, sch, D, idx, shares, 64)
            assert first[0].bad_batches == 2
            dev = Dev(shares, 64, 1, 65, D)
            with pytest.raises(E.SdaError) as e:
                if refused == "reveal":
                    _call(eng, sch, D, repeated, 1, dev, 64)
                else:
                    eng.packed_check_dev(sch, D, repeated, 1, dev.shares.data_ptr(), dev.verdict_ptr)
            assert e.value.status == UNSUPPORTED and message in str(e.value)
            assert (dev.out() == OUT_SENT).all() and (dev.verdict() == SENT).all()
            assert _same(_run_on(eng, valid, sch, D, idx, shares, 64), first)
    finally:
        eng.close()
