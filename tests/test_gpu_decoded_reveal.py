"""GPU: the decoded reveal (sda_packed_reveal_decoded_dev, sda_packed_reveal_decoded32_dev,
sda_secret_reconstruct_decoded) against tests/decoded_reveal_model.py.

Shares, shapes, representations and guarded buffers are tests/test_gpu_checked_reveal.py's; a guarded `wrong` buffer
joins them.  A case plants, in batch 0, the last batch overall, lanes 0 / 63 / 64 of a wave and scattered cells, error
sets of every size 1 .. e_max + 1: only among the basis positions, only among the check positions and straddling
both, with positions 1, k + t, k + t + 1 and n_idx among them, error values 1, p - 1 and (p - 1) / 2, and one batch
with every share moved.  The whole guarded out, verdict and wrong buffers, every count and the launch record are
compared with the model; what the definitions promise without the model -- a planted set within the radius costs
nothing -- is asserted besides, and every batch the checked reveal answers with 0 or j has the same secrets here.
"""
import ctypes as C

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import checked_reveal_model as R
from tests import decoded_reveal_model as DM
from tests import packed_matrix_cases as PM
from tests import share_check_model as M
from tests.test_checked_reveal_model import SCHEMES, kt_of
from tests.test_gpu_checked_reveal import (BS, OUT_SENT, Dev, _indices, _oracle_rows, _represent_for, _wrong_row)
from tests.test_gpu_share_check import GUARD, SENT

pytestmark = pytest.mark.gpu

W_GUARD = 4                    # uint32 words on each side of `wrong`
W_SENT = 0xFEEDBEEF
UNSUPPORTED, INVALID, NOT_ENOUGH = 66, 65, 6
UND = DM.UNDECODABLE


class DDev(Dev):
    """Dev plus the `wrong` words between guard words."""

    def __init__(self, shares, width, V, B, D, off=0):
        super().__init__(shares, width, V, B, D, off)
        self.wbuf = self.torch.from_numpy(np.full(V * B + 2 * W_GUARD, W_SENT, np.uint32).view(np.int32)).cuda()
        self.wrong_ptr = self.wbuf.data_ptr() + 4 * W_GUARD

    def wrong(self):
        self.torch.cuda.synchronize()
        return self.wbuf.cpu().numpy().view(np.uint32)

    def expect_wrong(self, wrong):
        g = np.full(W_GUARD, W_SENT, np.uint32)
        return np.concatenate([g, np.asarray(wrong, np.uint32).reshape(-1), g])


def _call(engine, sch, D, idx, V, dev, width, verdict=True, wrong=True):
    fn = engine.packed_reveal_decoded32_dev if width == 32 else engine.packed_reveal_decoded_dev
    return fn(sch, D, idx, V, dev.shares.data_ptr(), dev.out_ptr, dev.verdict_ptr if verdict else None,
              dev.wrong_ptr if wrong else None)


def _checked(engine, sch, D, idx, V, dev, width):
    fn = engine.packed_reveal_checked32_dev if width == 32 else engine.packed_reveal_checked_dev
    return fn(sch, D, idx, V, dev.shares.data_ptr(), dev.out_ptr, dev.verdict_ptr)


def _bucket(n_idx):
    return 8 if n_idx <= 8 else 16 if n_idx <= 16 else 32


def _record(sch, n_idx, verdict, wrong, bad, decoded=None, overflowed=0):
    kt = kt_of(sch)
    r = n_idx - kt
    if r < 2 or not bad:
        return E.DecodeLaunch(E.DECODE_PATH_FIRST_PASS, _bucket(n_idx), 0, 0, 0, 0)
    ok = verdict.reshape(-1) != UND
    fixed = int(np.count_nonzero(wrong.reshape(-1)[ok] & np.uint32((1 << kt) - 1)))
    sizes = verdict.reshape(-1)[ok]
    return E.DecodeLaunch(E.DECODE_PATH_DECODED, _bucket(n_idx), bad if decoded is None else decoded, fixed,
                          int(sizes.max()) if sizes.size else 0, overflowed)


def _error_sets(n_idx, kt, e_max):
    """0-based position sets of every size 1 .. e_max + 1: basis only, check only, straddling; positions 1, kt,
    kt + 1 and n_idx (1-based) are among them."""
    r = n_idx - kt
    sets = []
    for size in range(1, e_max + 2):
        if size <= kt:
            sets.append(list(range(size)))                               # basis, from position 1
            sets.append(list(range(kt - size, kt)))                     # basis, up to position kt
        if size <= r:
            sets.append(list(range(kt, kt + size)))                     # check, from position kt + 1
            sets.append(list(range(n_idx - size, n_idx)))               # check, up to position n_idx
        if size >= 2:
            a = min(size // 2, kt)
            sets.append(list(range(kt - a, kt)) + list(range(n_idx - (size - a), n_idx)))     # straddling
            sets.append([0] + list(range(kt, kt + size - 1)))
    out = []
    for s in sets:
        s = sorted(set(s))
        if s not in out and all(0 <= j < n_idx for j in s):
            out.append(s)
    return out


def _plant(canon, p, kt):
    """Plants on canon [V][n_idx][B] in place.  Returns {(v, b): sorted 0-based positions} and the moved cell."""
    V, n_idx, B = canon.shape
    e_max = (n_idx - kt) // 2
    errs = (1, p - 1, (p - 1) // 2)
    order = [(0, 0), (V - 1, B - 1), (0, 63), (V - 1, 64), (0, 127), (V - 1, 128), (V - 1, 0), (0, B - 1)]
    order += [((j + 1) % V, (7 * j + 3) % B) for j in range(6 * n_idx)]
    free = []
    for c in order:
        if c[1] < B and c not in free:
            free.append(c)
    cells = {}
    for i, s in enumerate(_error_sets(n_idx, kt, e_max)):
        if not free:
            break
        v, b = free.pop(0)
        for j in s:
            canon[v, j, b] = (canon[v, j, b] + errs[(i + j) % 3]) % p
        cells[(v, b)] = s
    shift = None
    if free:
        shift = free.pop(0)
        canon[shift[0], :, shift[1]] = (canon[shift[0], :, shift[1]] + 7) % p
    return cells, shift


def _matrix():
    pairs = [("b8", 5), ("b8", 7), ("b8", 8), ("b16", 9), ("b16", 11), ("b16", 13), ("b16", 16), ("config", 17),
             ("config", 19), ("config", 23), ("config", 26)]
    pairs += [("b8", 3), ("b8", 4), ("full_loop", 7), ("full_loop", 8), ("config", 15), ("config", 16)]     # r = 0, 1
    cases = []
    for i, (name, n_idx) in enumerate(pairs):
        cases.append((name, n_idx, 3 if i % 2 else 1, BS[i % len(BS)], 8 * ((i // 2) % 2)))
    cases += [("config", 26, 3, 1030, 8), ("b8", 8, 1, 1, 0), ("b16", 16, 3, 65, 8)]
    return cases


MATRIX = _matrix()


def test_the_matrix_reaches_every_shape_and_radius():
    assert {c[3] for c in MATRIX} == set(BS) and {c[2] for c in MATRIX} == {1, 3} and {c[4] for c in MATRIX} == {0, 8}
    radii = {(c[0], (c[1] - kt_of(SCHEMES[c[0]])) // 2) for c in MATRIX}
    assert {("b8", 1), ("b8", 2), ("b16", 1), ("b16", 2), ("b16", 3), ("b16", 4), ("config", 1), ("config", 2),
            ("config", 4), ("config", 5), ("config", 0), ("b8", 0), ("full_loop", 0)} <= radii
    sets = _error_sets(26, 15, 5)
    assert {len(s) for s in sets} == {1, 2, 3, 4, 5, 6}
    assert [0] in sets and [14] in sets and [15] in sets and [25] in sets
    assert any(s[0] < 15 <= s[-1] for s in sets)


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx,V,B,off", MATRIX, ids=[f"{a}-from{b}-V{c}-B{d}-off{e}" for a, b, c, d, e in MATRIX])
def test_decoded_reveal_matches_the_model(engine, oracle, name, n_idx, V, B, off, width):
    sch = SCHEMES[name]
    p, k, kt = sch.prime_modulus, sch.secret_count, kt_of(sch)
    r = n_idx - kt
    e_max = r // 2
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 19 * n_idx + B)
    canon = rows[0][:, idx, :] % p
    cells, shift = _plant(canon, p, kt)
    shares = _represent_for(sch, n_idx, canon, p, width, np.random.default_rng(n_idx + B))
    want, verdict, wrong, wr, radius, bad, first, undecoded, blame = DM.reveal(oracle, sch, D, idx, shares)
    # what the definitions say about the planted cells, independent of the model
    assert (wr, radius) == (r, e_max)
    for (v, b), pos in cells.items():
        lo, hi = b * k, min((b + 1) * k, D)
        if len(pos) <= e_max:
            assert verdict[v, b] == len(pos) and wrong[v, b] == sum(1 << j for j in pos)
            assert np.array_equal(want[v, lo:hi], secrets[0, v, lo:hi])
        elif r >= 1 and len(pos) <= r:                       # past the radius, still inside the distance: detected
            assert verdict[v, b] != 0
    if shift:
        assert verdict[shift] == (0 if r == 0 else UND)
    untouched = np.ones((V, B), bool)
    for v, b in list(cells) + ([shift] if shift else []):
        untouched[v, b] = False
    assert not verdict[untouched].any() and not wrong[untouched].any()

    dev = DDev(shares, width, V, B, D, off)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert np.array_equal(dev.verdict(), dev.expect_verdict(verdict))
    assert np.array_equal(dev.wrong(), dev.expect_wrong(wrong))
    assert np.array_equal(dev.out(), dev.expect_out(want))
    assert got == E.ShareDecode(r, e_max, bad, first, undecoded, blame)
    assert sum(got.blame) == int(verdict[verdict != UND].sum())
    assert engine.packed_decode_last_launch() == _record(sch, n_idx, verdict, wrong, bad)
    # the checked reveal on the same buffers: every batch it answers 0 or j has the same secrets here
    dev2 = DDev(shares, width, V, B, D, off)
    chk = _checked(engine, sch, D, idx, V, dev2, width)
    cv = dev2.verdict()[GUARD:-GUARD].reshape(V, B)
    co = dev2.out()[dev2.lead:dev2.lead + V * D].reshape(V, D)
    same = np.repeat(cv != M.UNLOCATED, k, axis=1)[:, :D]
    assert np.array_equal(co[same], want[same])
    assert np.array_equal(verdict[(cv != 0) & (cv != M.UNLOCATED)], np.ones(int(sum(chk.blame)), np.uint16))
    assert (chk.redundancy, chk.bad_batches, chk.first_bad) == (got.redundancy, got.bad_batches, got.first_bad)
    if r < 2:                                                # everything both calls report is identical
        assert np.array_equal(dev2.out(), dev.out()) and np.array_equal(dev2.verdict(), dev.verdict())
        assert chk.blame == got.blame and got.undecoded == chk.bad_batches


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx,V,B", (("config", 26, 3, 257), ("config", 19, 3, 257), ("b16", 16, 3, 257),
                                            ("config", 26, 3, 1030)))
def test_whole_wrong_rows_within_the_radius_cost_nothing(engine, monkeypatch, name, n_idx, V, B, width):
    """e_max clerks' rows replaced by the other participant's: every batch is decoded with exactly those positions
    and every secret is the fault-free one -- the same with SDA_CHECK_LOG_CAP below the bad count."""
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    r = n_idx - kt
    e_max = r // 2
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 3 + n_idx)
    pos = sorted({0, kt - 1, kt, n_idx - 1, 2, n_idx - 3})[:e_max] if e_max > 2 else [1, n_idx - 1][:e_max]
    shares = rows[0][:, idx, :].copy()
    for j in pos:
        shares[:, j, :] = _wrong_row(rows, idx[j], p)
    blame = [V * B if j in pos else 0 for j in range(n_idx)]
    mask = sum(1 << j for j in pos)
    fixed = V * B if any(j < kt for j in pos) else 0
    for cap in (None, "4") if B == 257 else (None,):
        if cap is None:
            monkeypatch.delenv("SDA_CHECK_LOG_CAP", raising=False)
        else:
            monkeypatch.setenv("SDA_CHECK_LOG_CAP", cap)
        dev = DDev(shares, width, V, B, D)
        got = _call(engine, sch, D, idx, V, dev, width)
        assert got == E.ShareDecode(r, e_max, V * B, 0, 0, blame)
        assert np.array_equal(dev.out(), dev.expect_out(secrets[0]))
        assert np.array_equal(dev.verdict(), dev.expect_verdict(np.full(V * B, e_max, np.uint16)))
        assert np.array_equal(dev.wrong(), dev.expect_wrong(np.full(V * B, mask, np.uint32)))
        over = 0 if cap is None else 1
        assert engine.packed_decode_last_launch() == E.DecodeLaunch(E.DECODE_PATH_DECODED, _bucket(n_idx), V * B,
                                                                    fixed, e_max, over)


@pytest.mark.parametrize("width", (64, 32))
@pytest.mark.parametrize("name,n_idx", (("config", 26), ("config", 19), ("b16", 16)))
def test_one_wrong_row_past_the_radius_flags_every_batch(engine, oracle, name, n_idx, width):
    V, B = 3, 257
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    r = n_idx - kt
    e_max = r // 2
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 3 + n_idx)
    pos = sorted({0, kt - 1, kt, n_idx - 1, 2, n_idx - 3, 4})[:e_max + 1]
    shares = rows[0][:, idx, :].copy()
    for j in pos:
        shares[:, j, :] = _wrong_row(rows, idx[j], p)
    dev = DDev(shares, width, V, B, D)
    got = _call(engine, sch, D, idx, V, dev, width)
    assert got == E.ShareDecode(r, e_max, V * B, 0, V * B, [0] * n_idx)
    first = np.stack([R._reveal(oracle, sch, D, idx[:kt], shares[v, :kt] % p) for v in range(V)])
    assert np.array_equal(dev.out(), dev.expect_out(first))
    assert np.array_equal(dev.verdict(), dev.expect_verdict(np.full(V * B, UND, np.uint16)))
    assert np.array_equal(dev.wrong(), dev.expect_wrong(np.zeros(V * B, np.uint32)))
    assert engine.packed_decode_last_launch() == E.DecodeLaunch(E.DECODE_PATH_DECODED, _bucket(n_idx), V * B, 0, 0, 0)


@pytest.mark.parametrize("width", (64, 32))
def test_verdict_and_wrong_are_independent_buffers(engine, oracle, width):
    name, n_idx, V, B = "config", 19, 3, 65
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, secrets, D = _oracle_rows(name, V, B)
    idx = _indices(sch, n_idx, 77)
    canon = rows[0][:, idx, :] % p
    _plant(canon, p, kt_of(sch))
    shares = _represent_for(sch, n_idx, canon, p, width, np.random.default_rng(5))
    want, verdict, wrong, r, radius, bad, first, undecoded, blame = DM.reveal(oracle, sch, D, idx, shares)
    assert undecoded and bad > undecoded
    for with_v in (True, False):
        for with_w in (True, False):
            dev = DDev(shares, width, V, B, D, 8)
            got = _call(engine, sch, D, idx, V, dev, width, verdict=with_v, wrong=with_w)
            assert got == E.ShareDecode(r, radius, bad, first, undecoded, blame)
            assert np.array_equal(dev.out(), dev.expect_out(want))
            assert np.array_equal(dev.verdict(), dev.expect_verdict(verdict)) if with_v else (dev.verdict() == SENT).all()
            assert np.array_equal(dev.wrong(), dev.expect_wrong(wrong)) if with_w else (dev.wrong() == W_SENT).all()


def test_host_form_equals_the_device_form_and_keeps_the_checked_reveals_statuses(engine, oracle):
    for name, n_idx, B in (("config", 20, 257), ("b8", 8, 63), ("full_loop", 8, 63)):
        sch = SCHEMES[name]
        p = sch.prime_modulus
        rows, secrets, D = _oracle_rows(name, 1, B)
        idx = _indices(sch, n_idx, 11)
        canon = rows[0][:, idx, :] % p
        _plant(canon, p, kt_of(sch))
        shares = _represent_for(sch, n_idx, canon, p, 64, np.random.default_rng(2))
        want, verdict, wrong, r, radius, bad, first, undecoded, blame = DM.reveal(oracle, sch, D, idx, shares)
        dev = DDev(shares, 64, 1, B, D)
        got_dev = _call(engine, sch, D, idx, 1, dev, 64)
        rec = engine.packed_decode_last_launch()
        out, got, ver, wr = engine.secret_reconstruct_decoded(sch, D, list(zip(idx, shares[0])))
        assert got == got_dev == E.ShareDecode(r, radius, bad, first, undecoded, blame)
        assert np.array_equal(out, want[0]) and np.array_equal(ver, verdict[0]) and np.array_equal(wr, wrong[0])
        assert engine.packed_decode_last_launch() == rec
        out2, got2, ver2, wr2 = engine.secret_reconstruct_decoded(sch, D, list(zip(idx, shares[0])), want_verdict=False,
                                                                  want_wrong=False)
        assert np.array_equal(out2, out) and got2 == got and ver2 is None and wr2 is None
    # ragged rows, too few rows, repeated indices: sda_secret_reconstruct_checked's statuses
    sch, B = SCHEMES["config"], 257
    rows, secrets, D = _oracle_rows("config", 1, B)
    idx = list(range(18))
    full = list(zip(idx, rows[0][0, idx, :]))
    ragged = [(i, row if j != 2 else row[: B - 1]) for j, (i, row) in enumerate(full)]
    few = full[: kt_of(sch) - 1]
    few_ragged = [(i, row if j else row[:0]) for j, (i, row) in enumerate(few)]
    for rows_ in (ragged, few, few_ragged, [(idx[0], row) for _, row in full]):
        with pytest.raises(E.SdaError) as a:
            engine.secret_reconstruct_checked(sch, D, rows_)
        with pytest.raises(E.SdaError) as b:
            engine.secret_reconstruct_decoded(sch, D, rows_)
        assert a.value.status == b.value.status
    with pytest.raises(E.SdaError) as e:
        engine.secret_reconstruct_decoded(S.Additive(3, 433), 4, [(i, np.arange(4)) for i in range(3)])
    assert e.value.status == UNSUPPORTED
    n80 = SCHEMES["n80"]
    r80, _, D80 = _oracle_rows("n80", 1, 65)
    with pytest.raises(E.SdaError) as e:
        engine.secret_reconstruct_decoded(n80, D80, [(i, r80[0][0, i, :]) for i in range(40)])
    assert e.value.status == UNSUPPORTED and "32" in str(e.value)
    out, got, ver, wr = engine.secret_reconstruct_decoded(sch, 0, full)
    assert out.size == 0 and got == E.ShareDecode(3, 1, 0, E.CHECK_NO_BAD, 0, [0] * 18) and ver.size == wr.size == 0


def test_status_matrix_follows_the_checked_reveal_and_a_failing_call_writes_nothing(engine):
    name, V, B = "config", 2, 40
    sch = SCHEMES[name]
    rows, secrets, D = _oracle_rows(name, V, B)
    kt, n = kt_of(sch), sch.share_count
    good = list(range(18))
    dev = DDev(rows[0][:, :18, :], 64, V, B, D)
    first = _call(engine, sch, D, good, V, dev, 64)
    assert first == E.ShareDecode(3, 1, 0, E.CHECK_NO_BAD, 0, [0] * 18)
    assert np.array_equal(dev.out(), dev.expect_out(secrets[0]))
    assert np.array_equal(dev.wrong(), dev.expect_wrong(np.zeros(V * B, np.uint32)))
    clean = (dev.verdict().copy(), dev.out().copy(), dev.wrong().copy())
    rec = engine.packed_decode_last_launch()
    assert rec == E.DecodeLaunch(E.DECODE_PATH_FIRST_PASS, 32, 0, 0, 0, 0)

    def untouched():
        return (np.array_equal(dev.verdict(), clean[0]) and np.array_equal(dev.out(), clean[1])
                and np.array_equal(dev.wrong(), clean[2]) and engine.packed_decode_last_launch() == rec)

    bad_root = S.PackedShamir(sch.secret_count, n, sch.privacy_threshold(), sch.prime_modulus, sch.omega_secrets, 1)
    even_p = S.PackedShamir(sch.secret_count, n, sch.privacy_threshold(), sch.prime_modulus - 1, sch.omega_secrets,
                            sch.omega_shares)
    failing = [
        (sch, D, good[: kt - 1], V), (sch, D, list(range(1024)), V), (sch, D, good, 65536),
        (even_p, D, good, V), (bad_root, D, good, V), (even_p, D, good[: kt - 1], V),
        (sch, D, good[: kt - 1], 65536), (sch, D, list(range(1024)), 65536),
        (sch, D, [0] * 18, V), (sch, D, good[:16] + [3, 4], V),
    ]
    for s, d, idx, nv in failing:
        codes = []
        for call in (lambda: engine.packed_reveal_checked_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.out_ptr,
                                                              dev.verdict_ptr),
                     lambda: engine.packed_reveal_decoded_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.out_ptr,
                                                              dev.verdict_ptr, dev.wrong_ptr),
                     lambda: engine.packed_reveal_decoded32_dev(s, d, idx, nv, dev.shares.data_ptr(), dev.out_ptr,
                                                                dev.verdict_ptr, dev.wrong_ptr)):
            try:
                call()
                codes.append(0)
            except E.SdaError as e:
                codes.append(e.status)
        assert codes[0] != 0 and codes[0] == codes[1] == codes[2], (codes, d, len(idx), nv)
        assert untouched()
    # the three scopes outside the decoder
    n80 = SCHEMES["n80"]
    k9 = PM.scheme_for(9, 6, 26)
    for s, idx, word in ((n80, list(range(40)), "32"), (k9, list(range(20)), "8"), (S.Additive(18, 433), good, "Additive")):
        with pytest.raises(E.SdaError) as e:
            engine.packed_reveal_decoded_dev(s, D, idx, V, dev.shares.data_ptr(), dev.out_ptr, dev.verdict_ptr,
                                             dev.wrong_ptr)
        assert e.value.status == UNSUPPORTED and word in str(e.value), str(e.value)
        assert untouched()
    with pytest.raises(E.SdaError) as e:
        engine.packed_reveal_decoded_dev(sch, D, [0] * 18, V, dev.shares.data_ptr(), dev.out_ptr, dev.verdict_ptr,
                                         dev.wrong_ptr)
    assert e.value.status == UNSUPPORTED and "distinct" in str(e.value)
    # each NULL argument, through the C ABI; a failing call leaves the host outputs alone
    s = sch.c()
    idx = np.asarray(good, np.uint64)
    vals = [C.c_uint64(111 * (i + 1)) for i in range(5)]
    blame = np.full(18, 444, np.uint64)
    u64p = C.POINTER(C.c_uint64)

    def raw(h=engine.h, sp=C.byref(s), ip=idx.ctypes.data_as(u64p), sh=dev.shares.data_ptr(), out=dev.out_ptr,
            r=C.byref(vals[0]), rad=C.byref(vals[1]), b=C.byref(vals[2]), f=C.byref(vals[3]), u=C.byref(vals[4]),
            bl=blame.ctypes.data_as(u64p), n_idx=18, wrong=dev.wrong_ptr):
        return engine.lib.sda_packed_reveal_decoded_dev(h, sp, D, ip, n_idx, V, sh, out, dev.verdict_ptr, wrong, r, rad,
                                                        b, f, u, bl, None)
    for kw in ({"h": None}, {"sp": None}, {"ip": None}, {"sh": None}, {"out": None}, {"r": None}, {"rad": None},
               {"b": None}, {"f": None}, {"u": None}, {"bl": None}, {"wrong": dev.wrong_ptr + 2}):
        assert raw(**kw) == INVALID, kw
    assert raw(n_idx=kt - 1) == NOT_ENOUGH
    assert [v.value for v in vals] == [111, 222, 333, 444, 555] and (blame == 444).all()
    assert untouched()
    # SDA_OK with nothing launched: dimension == 0, no vectors
    dirty = DDev(rows[0][:, :18, :], 64, V, B, D)
    none = E.ShareDecode(3, 1, 0, E.CHECK_NO_BAD, 0, [0] * 18)
    assert _call(engine, sch, 0, good, V, dirty, 64) == none
    assert _call(engine, sch, 0, good[:3], V, dirty, 64).redundancy == 0
    assert _call(engine, sch, D, good, 0, dirty, 64) == none
    assert (dirty.verdict() == SENT).all() and (dirty.out() == OUT_SENT).all() and (dirty.wrong() == W_SENT).all()
    assert engine.packed_decode_last_launch() == rec


def test_record_is_all_zeros_before_the_first_decoded_reveal():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    e = E.Engine(0)
    try:
        assert e.packed_decode_last_launch() == E.DecodeLaunch(0, 0, 0, 0, 0, 0)
    finally:
        e.close()
