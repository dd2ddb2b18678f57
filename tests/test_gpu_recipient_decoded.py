"""GPU: the robust recipient job (sda_recipient_job_decoded, sda_recipient_job_decoded_dev,
sda_recipient_reveal_decoded_dev) against tests/recipient_decoded_model.py and against the composition of the calls a
recipient had to make before it existed: sda_varint_decode per blob, sda_secret_reconstruct_decoded,
sda_mask_combine, sda_secret_unmask, sda_recipient_positive.

Payloads are built as tests/recipient_job_cases.py builds them (each row encoded by the oracle, the device buffers
laid out by its layout()).  One scheme per register bucket, B at the edges of the 256-lane workgroup and its flush,
D = k B and the tail batch cut to one secret, `out` and the Full mask 16-byte aligned and 8 bytes off in all four
combinations, no masking / Full / ChaCha with 1 and 8 seed words.  Guarded out, verdict and wrong buffers are compared
whole; the record is asserted in every case.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import checked_reveal_model as R
from tests import packed_matrix_cases as PMC
from tests import pipeline_model as PM
from tests import recipient_decoded_model as RD
from tests import recipient_job_cases as RC
from tests.test_checked_reveal_model import SCHEMES, kt_of

pytestmark = pytest.mark.gpu

G = 4                                  # guard words on each side of every buffer
OUT_SENT, V_SENT, W_SENT = -0x0123456789ABCDEF, 0xA5C3, 0xFEEDBEEF
UNSUPPORTED, INVALID, NOT_ENOUGH, PRECONDITION = 66, 65, 6, 64
UND = 0xFFFF
I64_MIN, I64_MAX = -2**63, 2**63 - 1
BS = (1, 2, 255, 256, 257, 513)
KINDS = ("none", "full", "chacha1", "chacha8")
# one scheme per bucket; configs[2]'s scheme from 26 and from 17 results
BUCKETS = (("b8", 8), ("b16", 13), ("config", 26), ("config", 17))


@functools.lru_cache(maxsize=None)
def _sharing(name, B, tail):
    """([2 participants][n][B] exact signed shares, [2][D] canonical secrets, D) from the oracle."""
    from oracle import oracle as O
    sch = SCHEMES[name]
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    D = k * B - (k - 1 if tail else 0)
    rng = np.random.default_rng(9000 * B + tail)
    rows, secrets = [], []
    for _ in range(2):
        s = rng.integers(0, p, D)
        secrets.append(s)
        rows.append(O.packed_generate(R._params(O, sch), s, rng.integers(0, p - 1, B * t)))
    rows, secrets = np.stack(rows), np.stack(secrets)
    rows.setflags(write=False)
    return rows, secrets, D


def _masking(kind, p, D, rng):
    """(scheme, mask rows as the host form's blobs decode to them)"""
    if kind == "none":
        return S.NoMasking(), []
    if kind == "full":
        return S.FullMasking(p), [[int(v) for v in rng.integers(0, p, D)] for _ in range(3)]
    w = 1 if kind == "chacha1" else 8
    return S.ChaChaMasking(p, D, 32 * w), [[int(v) for v in rng.integers(0, 2**32, w)] for _ in range(3)]


def _enc(oracle, row):
    return oracle.varint_encode(np.asarray(row, np.int64)) if len(row) else b""


def _wrong_row(rows, clerk, p):
    wrong, right = rows[1][clerk].copy(), rows[0][clerk]
    same = (wrong - right) % p == 0
    wrong[same] += np.where(wrong[same] < p - 1, 1, -1)
    return wrong


class Guarded:
    """a device buffer of n elements between G guard words, its start moved by `off` elements"""

    def __init__(self, n, dtype, sent, off=0):
        import torch
        self.torch, self.n, self.off, self.sent, self.dtype = torch, n, off, sent, dtype
        host = np.full(G + off + n + G, sent, dtype)
        self.buf = torch.from_numpy(host.view({np.uint16: np.int16, np.uint32: np.int32}.get(dtype, dtype))).cuda()
        self.ptr = self.buf.data_ptr() + (G + off) * host.itemsize

    def host(self):
        self.torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(self.dtype)

    def expect(self, values):
        e = np.full(G + self.off + self.n + G, self.sent, self.dtype)
        e[G + self.off:G + self.off + self.n] = np.asarray(values, self.dtype)
        return e

    def untouched(self):
        return bool((self.host() == np.asarray(self.sent, self.dtype)).all())


class Bufs:
    def __init__(self, D, B, out_off=0):
        self.out = Guarded(D, np.int64, OUT_SENT, out_off)
        self.verdict = Guarded(B, np.uint16, V_SENT)
        self.wrong = Guarded(B, np.uint32, W_SENT)
        assert self.out.ptr % 16 == 8 * out_off

    def check(self, exp, what):
        assert np.array_equal(self.out.host(), self.out.expect(exp.out)), what
        assert np.array_equal(self.verdict.host(), self.verdict.expect(exp.verdict)), what
        assert np.array_equal(self.wrong.host(), self.wrong.expect(exp.wrong)), what

    def untouched(self):
        return self.out.untouched() and self.verdict.untouched() and self.wrong.untouched()


class DevBlobs:
    def __init__(self, blobs):
        import torch
        buf, off = RC.layout(list(blobs))
        self.off = off.astype(np.uint64)
        self.dev = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self):
        return self.dev.data_ptr()


def _dev_i64(values, off=0):
    """(tensor, pointer) of i64 values on the device, the pointer 8 * off bytes past a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.concatenate([np.zeros(2 + off, np.int64), np.asarray(values, np.int64).reshape(-1)])).cuda()
    ptr = t.data_ptr() + 8 * (2 + off)
    assert ptr % 16 == 8 * off
    return t, ptr


def _records(eng):
    return (eng.recipient_decoded_last_launch(), eng.packed_decode_last_launch(), tuple(eng.recipient_last_launch()),
            tuple(eng.recipient_job_last_launch()), eng.chacha_last_launch(), eng.codec_last_launch(),
            tuple(eng.combine_last_launch()))


def _decode_tuple(exp):
    return E.ShareDecode(exp.redundancy, exp.radius, exp.bad_batches, exp.first_bad, exp.undecoded, exp.blame)


def _composition(engine, sch, ms, mask_rows, D, idx, blobs):
    """today's robust sequence on the GPU: (out, ShareDecode, verdict, wrong)"""
    p = sch.prime_modulus
    rows = [engine.varint_decode(b) for b in blobs]
    secrets, dec, ver, wr = engine.secret_reconstruct_decoded(sch, D, list(zip(idx, rows)))
    if isinstance(ms, S.NoMasking):
        out = secrets
    else:
        mask = engine.mask_combine(ms, [np.asarray(r, np.int64) for r in mask_rows])
        out = engine.secret_unmask(ms, (mask, secrets))
    return engine.positive(p, out), dec, ver, wr


def _job_dev(engine, sch, ms, mask_rows, D, idx, clerk, bufs, mask_off=0, verdict=True, wrong=True, oracle=None):
    """sda_recipient_job_decoded_dev on guarded buffers: the Full mask folded by the model, ChaCha seeds as blobs"""
    kw = {}
    keep = None
    if isinstance(ms, S.FullMasking):
        keep, ptr = _dev_i64(PM.mask_combine(ms, mask_rows), mask_off)
        kw = dict(mask_ptr=ptr, mask_len=D)
    elif isinstance(ms, S.ChaChaMasking):
        keep = DevBlobs([_enc(oracle, r) for r in mask_rows])
        kw = dict(seed_ptr=keep.ptr(), seed_off=keep.off)
    n, dec = engine.recipient_job_decoded_dev(ms, sch, D, idx, clerk.ptr(), clerk.off, sch.prime_modulus, bufs.out.ptr,
                                              D, verdict_ptr=bufs.verdict.ptr if verdict else None,
                                              wrong_ptr=bufs.wrong.ptr if wrong else None, **kw)
    del keep
    return n, dec


def _reveal_dev(engine, sch, ms, mask_rows, D, idx, rows, bufs, verdict=True, wrong=True):
    """sda_recipient_reveal_decoded_dev: clerk rows [n_idx][len] and mask rows on the device"""
    import torch
    sh, sh_ptr = _dev_i64(rows)
    if isinstance(ms, S.FullMasking):
        m, m_ptr = _dev_i64(np.asarray(mask_rows, np.int64))
        nm, w = len(mask_rows), D
    elif isinstance(ms, S.ChaChaMasking):
        m = torch.from_numpy(np.asarray(mask_rows, np.uint32).view(np.int32)).cuda()
        m_ptr, nm, w = m.data_ptr(), len(mask_rows), len(mask_rows[0])
    else:
        m, m_ptr, nm, w = None, None, 0, 0
    return engine.recipient_reveal_decoded_dev(ms, m_ptr, nm, w, sch, D, idx, sh_ptr, rows.shape[1], sch.prime_modulus,
                                               bufs.out.ptr, D, verdict_ptr=bufs.verdict.ptr if verdict else None,
                                               wrong_ptr=bufs.wrong.ptr if wrong else None)


def _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, clerk_rows, out_off=0, mask_off=0, fused=True,
                    redo=False, clean=None):
    """One case through the model, the composition and the three entry points.  clerk_rows: the rows the clerk blobs
    encode (any lengths >= B).  clean: the expected output when the definitions promise it without the model."""
    B = (D + sch.secret_count - 1) // sch.secret_count
    blobs = [_enc(oracle, r) for r in clerk_rows]
    exp = RD.run(oracle, ms, mask_rows, sch, D, list(zip(idx, clerk_rows)))
    if clean is not None:
        assert np.array_equal(exp.out, clean)
    want = _decode_tuple(exp)
    stride = max(len(r) for r in clerk_rows)
    # the composition of today's calls
    c_out, c_dec, c_ver, c_wr = _composition(engine, sch, ms, mask_rows, D, idx, blobs)
    assert c_dec == want and np.array_equal(c_out, exp.out)
    assert np.array_equal(c_ver, exp.verdict) and np.array_equal(c_wr, exp.wrong)
    # host form
    out, dec, ver, wr = engine.recipient_job_decoded(ms, [_enc(oracle, r) for r in mask_rows], sch, D,
                                                     list(zip(idx, blobs)), sch.prime_modulus)
    assert dec == want
    assert np.array_equal(out, exp.out) and np.array_equal(ver, exp.verdict) and np.array_equal(wr, exp.wrong)
    assert tuple(engine.recipient_decoded_last_launch()) == RD.record(ms, stride, B, fused, redo)
    # device form
    bufs = Bufs(D, B, out_off)
    n, dec = _job_dev(engine, sch, ms, mask_rows, D, idx, DevBlobs(blobs), bufs, mask_off, oracle=oracle)
    assert (n, dec) == (D, want)
    bufs.check(exp, "job_dev")
    assert tuple(engine.recipient_decoded_last_launch()) == RD.record(ms, stride, B, fused, redo)
    return exp


MATRIX = [(name, n_idx, BS[(i + j) % len(BS)], (i + j) % 2, kind, (i + j) % 2, ((i + j) // 2) % 2)
          for i, (name, n_idx) in enumerate(BUCKETS) for j, kind in enumerate(KINDS)]
# every B and both tails at configs[2] from 26 under Full masking, all four alignment combinations among them
MATRIX += [("config", 26, B, t, "full", a % 2, (a // 2) % 2) for a, (B, t) in
           enumerate((B, t) for B in BS for t in (0, 1))]
MATRIX += [("b16", 13, 257, 1, "full", 1, 0), ("b16", 13, 257, 1, "full", 0, 1), ("b8", 8, 513, 0, "chacha8", 1, 0)]
MATRIX = sorted(set(MATRIX))


def test_the_matrix_reaches_every_shape():
    assert {c[2] for c in MATRIX} == set(BS) and {c[3] for c in MATRIX} == {0, 1}
    assert {c[4] for c in MATRIX} == set(KINDS) and {(c[0], c[1]) for c in MATRIX} == set(BUCKETS)
    assert {(c[5], c[6]) for c in MATRIX if c[4] == "full"} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def _scatter(sh, p, kt, B):
    """wrong cells in batch 0, the last batch and lanes 63 / 64 / 255 / 256: at a basis position, at a check position
    and, from a redundancy of 4 (two correctable errors), across both.  Of the matrix's schemes only configs[2]'s from
    17 results (r = 2) is below that and gets single cells at basis and check positions alone; b8 from 8 has r = 5, b16
    from 13 r = 6, configs[2]'s from 26 r = 11."""
    n_idx = sh.shape[0]
    r = n_idx - kt
    for i, b in enumerate(sorted({0, B - 1, 63, 64, 255, 256} & set(range(B)))):
        pos = ([0], [n_idx - 1], [kt - 1, kt])[i % 3] if r >= 4 else ([i % kt], [n_idx - 1])[i % 2]
        for j in pos:
            sh[j, b] = (sh[j, b] + 1 + i) % p


@pytest.mark.parametrize("name,n_idx,B,tail,kind,out_off,mask_off", MATRIX,
                         ids=[f"{a}-from{b}-B{c}-tail{d}-{e}-out{f}-mask{g}" for a, b, c, d, e, f, g in MATRIX])
def test_no_error_one_wrong_payload_and_scattered_cells(engine, oracle, name, n_idx, B, tail, kind, out_off, mask_off):
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    rows, secrets, D = _sharing(name, B, tail)
    rng = np.random.default_rng(n_idx * 1000 + B)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    ms, mask_rows = _masking(kind, p, D, rng)
    mask = PM.mask_combine(ms, mask_rows) or [0] * D
    clean = (secrets[0] - np.asarray(mask, np.int64)) % p
    sh = rows[0][idx].copy()
    # no error
    exp = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, list(sh), out_off, mask_off, clean=clean)
    assert exp.bad_batches == 0
    # one clerk's whole payload replaced (the model solves one linear system per bad batch: the widest B is left to
    # test_whole_wrong_payloads_at_and_past_the_radius, at a smaller scheme)
    if B <= 257:
        one = sh.copy()
        one[1] = _wrong_row(rows, idx[1], p)
        exp = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, list(one), out_off, mask_off, clean=clean)
        assert exp.bad_batches == B and exp.undecoded == 0
        assert exp.blame == [B if j == 1 else 0 for j in range(n_idx)]
    # scattered cells
    sc = sh.copy()
    _scatter(sc, p, kt, B)
    _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, list(sc), out_off, mask_off)


@pytest.mark.parametrize("kind", ("full", "chacha8", "none"))
@pytest.mark.parametrize("name,n_idx,B", (("config", 26, 257), ("config", 17, 256), ("b16", 13, 513), ("b8", 8, 255)))
def test_whole_wrong_payloads_at_and_past_the_radius(engine, oracle, name, n_idx, B, kind):
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    rows, secrets, D = _sharing(name, B, 1)
    rng = np.random.default_rng(n_idx + B)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    ms, mask_rows = _masking(kind, p, D, rng)
    e_max = (n_idx - kt) // 2
    pos = sorted({0, kt - 1, kt, n_idx - 1, 2, n_idx - 3, 4})
    sh = rows[0][idx].copy()
    for j in pos[:e_max]:
        sh[j] = _wrong_row(rows, idx[j], p)
    clean_blobs = [_enc(oracle, r) for r in rows[0][idx]]
    job = engine.recipient_job(ms, [_enc(oracle, r) for r in mask_rows], sch, D, list(zip(idx, clean_blobs)), p)
    exp = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, list(sh), clean=job)
    assert (exp.bad_batches, exp.undecoded) == (B, 0)
    # one more: every batch undecodable
    sh[pos[e_max]] = _wrong_row(rows, idx[pos[e_max]], p)
    exp = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, list(sh))
    assert (exp.bad_batches, exp.undecoded) == (B, B) and (exp.verdict == UND).all()


@pytest.mark.parametrize("kind", ("full", "chacha1"))
def test_a_long_wrong_payload_takes_the_compaction_route_and_i64_extremes_are_reduced_exactly(engine, oracle, kind):
    name, n_idx, B = "config", 19, 257
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, secrets, D = _sharing(name, B, 1)
    rng = np.random.default_rng(77)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    ms, mask_rows = _masking(kind, p, D, rng)
    mask = PM.mask_combine(ms, mask_rows)
    clean = (secrets[0] - np.asarray(mask, np.int64)) % p
    clerk_rows = [r for r in rows[0][idx]]
    clerk_rows[3] = np.concatenate([_wrong_row(rows, idx[3], p), np.arange(5, dtype=np.int64)])        # B + 5 values
    ext = np.asarray([I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, -p, p, 2**62, -2**62], np.int64)
    clerk_rows[7] = np.resize(ext, B)
    exp = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, clerk_rows, clean=clean)
    assert engine.recipient_decoded_last_launch().compact == 1 and exp.undecoded == 0
    assert exp.blame[3] == B and exp.blame[7] >= B - 2


def test_the_gap_the_plain_job_returns_ok_on_a_wrong_payload(engine, oracle):
    name, n_idx, B = "config", 26, 257
    sch = SCHEMES[name]
    p, k = sch.prime_modulus, sch.secret_count
    rows, secrets, D = _sharing(name, B, 0)
    rng = np.random.default_rng(3)
    idx = list(range(n_idx))
    ms, mask_rows = _masking("full", p, D, rng)
    mblobs = [_enc(oracle, r) for r in mask_rows]
    sh = rows[0][idx].copy()
    clean = engine.recipient_job(ms, mblobs, sch, D, [(i, _enc(oracle, r)) for i, r in zip(idx, sh)], p)
    planted = [0, 63, 256]
    sh[5, planted] = (sh[5, planted] + 1) % p
    bad = [(i, _enc(oracle, r)) for i, r in zip(idx, sh)]
    plain = engine.recipient_job(ms, mblobs, sch, D, bad, p)                 # SDA_OK, and wrong
    differs = {int(b) for b in np.flatnonzero(plain != clean) // k}
    assert differs == set(planted)
    out, dec, ver, wr = engine.recipient_job_decoded(ms, mblobs, sch, D, bad, p)
    assert np.array_equal(out, clean) and dec.blame == [3 if j == 5 else 0 for j in range(n_idx)]
    assert dec.bad_batches == 3 and dec.undecoded == 0 and set(np.flatnonzero(wr)) == set(planted)
    # a whole wrong payload: blamed in every batch
    sh[5] = _wrong_row(rows, idx[5], p)
    out, dec, ver, wr = engine.recipient_job_decoded(ms, mblobs, sch, D,
                                                     [(i, _enc(oracle, r)) for i, r in zip(idx, sh)], p)
    assert np.array_equal(out, clean) and dec.blame[5] == B and (wr == 1 << 5).all()


def _knob_case(oracle, kind):
    name, n_idx, B = "config", 19, 257
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, secrets, D = _sharing(name, B, 1)
    rng = np.random.default_rng(11)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    ms, mask_rows = _masking(kind, p, D, rng)
    sh = rows[0][idx].copy()
    sh[2] = _wrong_row(rows, idx[2], p)
    _scatter(sh, p, kt_of(sch), B)
    return sch, ms, mask_rows, D, idx, list(sh)


@pytest.mark.parametrize("kind", ("full", "chacha8"))
def test_knobs_give_identical_buffers_and_their_records(engine, oracle, monkeypatch, kind):
    sch, ms, mask_rows, D, idx, sh = _knob_case(oracle, kind)
    for var in ("SDA_RECIPIENT_REDO", "SDA_RECIPIENT_FUSE_UNMASK", "SDA_CHECK_LOG_CAP"):
        monkeypatch.delenv(var, raising=False)
    base = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, sh, out_off=1, mask_off=1)
    monkeypatch.setenv("SDA_RECIPIENT_REDO", "1")
    redo = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, sh, out_off=1, mask_off=1, redo=True)
    assert engine.recipient_decoded_last_launch().reveal_runs == (2 if kind == "chacha8" else 1)
    monkeypatch.delenv("SDA_RECIPIENT_REDO")
    monkeypatch.setenv("SDA_RECIPIENT_FUSE_UNMASK", "0")
    unfused = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, sh, out_off=1, mask_off=1, fused=False)
    assert engine.recipient_decoded_last_launch().unmask_route == 2
    monkeypatch.setenv("SDA_RECIPIENT_REDO", "1")
    _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, sh, fused=False, redo=True)
    monkeypatch.delenv("SDA_RECIPIENT_REDO")
    monkeypatch.delenv("SDA_RECIPIENT_FUSE_UNMASK")
    monkeypatch.setenv("SDA_CHECK_LOG_CAP", "1")
    over = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, sh, out_off=1, mask_off=1)
    assert engine.packed_decode_last_launch().overflowed == 1
    for other in (redo, unfused, over):
        assert np.array_equal(other.out, base.out) and _decode_tuple(other) == _decode_tuple(base)


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_entry_points_agree_with_verdict_and_wrong_given_or_not(engine, oracle, kind):
    sch, ms, mask_rows, D, idx, sh = _knob_case(oracle, kind)
    B = len(sh[0])
    exp = RD.run(oracle, ms, mask_rows, sch, D, list(zip(idx, sh)))
    want = _decode_tuple(exp)
    blobs = [_enc(oracle, r) for r in sh]
    mblobs = [_enc(oracle, r) for r in mask_rows]
    for with_v in (True, False):
        for with_w in (True, False):
            out, dec, ver, wr = engine.recipient_job_decoded(ms, mblobs, sch, D, list(zip(idx, blobs)),
                                                             sch.prime_modulus, want_verdict=with_v, want_wrong=with_w)
            assert dec == want and np.array_equal(out, exp.out)
            assert np.array_equal(ver, exp.verdict) if with_v else ver is None
            assert np.array_equal(wr, exp.wrong) if with_w else wr is None
            for form in ("job", "reveal"):
                bufs = Bufs(D, B, 1)
                if form == "job":
                    n, dec = _job_dev(engine, sch, ms, mask_rows, D, idx, DevBlobs(blobs), bufs, 1, with_v, with_w,
                                      oracle=oracle)
                else:
                    n, dec = _reveal_dev(engine, sch, ms, mask_rows, D, idx, np.stack(sh), bufs, with_v, with_w)
                assert (n, dec) == (D, want), form
                assert np.array_equal(bufs.out.host(), bufs.out.expect(exp.out)), form
                assert (np.array_equal(bufs.verdict.host(), bufs.verdict.expect(exp.verdict)) if with_v
                        else bufs.verdict.untouched()), form
                assert (np.array_equal(bufs.wrong.host(), bufs.wrong.expect(exp.wrong)) if with_w
                        else bufs.wrong.untouched()), form
                assert tuple(engine.recipient_decoded_last_launch()) == RD.record(ms, B, B)


def test_r0_r1_and_dimension_zero_behave_as_the_decoded_reveal(engine, oracle):
    name, B = "config", 65
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    rows, secrets, D = _sharing(name, B, 1)
    rng = np.random.default_rng(1)
    ms, mask_rows = _masking("full", p, D, rng)
    for n_idx in (kt, kt + 1):
        idx = rng.permutation(sch.share_count)[:n_idx].tolist()
        sh = rows[0][idx].copy()
        sh[0, 7] = (sh[0, 7] + 1) % p
        exp = _run_everything(engine, oracle, sch, ms, mask_rows, D, idx, list(sh))
        assert exp.radius == 0 and exp.undecoded == exp.bad_batches == (n_idx - kt)
    idx = list(range(18))
    before = _records(engine)
    out, dec, ver, wr = engine.recipient_job_decoded(S.FullMasking(p), [], sch, 0,
                                                     [(i, _enc(oracle, rows[0][i])) for i in idx], p)
    assert out.size == 0 and dec == E.ShareDecode(3, 1, 0, E.CHECK_NO_BAD, 0, [0] * 18)
    assert _records(engine) == before


# ---------------------------------------------------------------- statuses
def _raw_dev(eng, sch, ms, D, idx, clerk, bufs, seeds=None, mask=None, fault=None, m_out=None, counts=None,
             decoded=True, out_cap=None):
    """sda_recipient_job_decoded_dev (or, decoded=False, sda_recipient_job_dev) through ctypes -> status"""
    msc, ssc = ms.c(), sch.c()
    ia = np.asarray(list(idx) or [0], np.uint64)
    olen = C.c_uint64(77)
    soff = seeds.off.copy() if seeds is not None else np.zeros(1, np.uint64)
    coff = clerk.off.copy()
    a = {"ms": C.byref(msc), "ss": C.byref(ssc), "out_len": C.byref(olen), "indices": E._ptr(ia, E._u64p),
         "clerk_bytes": clerk.ptr(), "clerk_off": E._ptr(coff, E._u64p),
         "seed_bytes": seeds.ptr() if seeds is not None else None, "seed_off": E._ptr(soff, E._u64p),
         "mask": mask[1] if mask else None, "out": bufs.out.ptr, "wrong": bufs.wrong.ptr}
    cs = counts or ([C.c_uint64(111 * (i + 1)) for i in range(5)], np.full(max(len(idx), 1), 444, np.uint64))
    cp = {n: C.byref(c) for n, c in zip(("redundancy", "radius", "bad_batches", "first_bad", "undecoded"), cs[0])}
    cp["blame"] = E._ptr(cs[1], E._u64p)
    if fault in a:
        a[fault] = None
    if fault in cp:
        cp[fault] = None
    if fault in ("seed_bytes+8", "clerk_bytes+8"):
        a[fault[:-2]] += 8
    if fault == "wrong+2":
        a["wrong"] += 2
    if fault == "clerk_off-decreasing":
        coff[1], coff[2] = coff[2], coff[1]
    if fault == "seed_off-decreasing":
        soff[1], soff[2] = soff[2], soff[1]
    n_seeds = 0 if isinstance(ms, S.FullMasking) or seeds is None else soff.size - 1
    head = (eng.h, a["ms"], a["mask"], D if mask else 0, a["seed_bytes"], a["seed_off"], n_seeds, a["ss"], D,
            a["indices"], a["clerk_bytes"], a["clerk_off"], len(idx), sch.prime_modulus if m_out is None else m_out)
    cap = D if out_cap is None else out_cap
    if decoded:
        st = eng.lib.sda_recipient_job_decoded_dev(*head, a["out"], cap, a["out_len"], bufs.verdict.ptr, a["wrong"],
                                                   cp["redundancy"], cp["radius"], cp["bad_batches"], cp["first_bad"],
                                                   cp["undecoded"], cp["blame"], None)
    else:
        st = eng.lib.sda_recipient_job_dev(*head, E.REVEAL_CANONICAL, a["out"], cap, a["out_len"], None)
    bufs.out.torch.cuda.synchronize()
    return st


def test_status_matrix_and_a_failing_call_writes_nothing(engine, oracle):
    name, n_idx, B = "b8", 8, 9
    sch = SCHEMES[name]                                    # p = 433, the modulus of recipient_job_cases.fault_case
    p, kt = sch.prime_modulus, kt_of(sch)
    rows, secrets, D = _sharing(name, B, 0)
    idx = list(range(n_idx))
    blobs = [_enc(oracle, r) for r in rows[0][idx]]
    clerk = DevBlobs(blobs)
    rng = np.random.default_rng(2)
    chacha, seed_rows = _masking("chacha8", p, D, rng)
    full, mask_rows = _masking("full", p, D, rng)
    seeds = DevBlobs([_enc(oracle, r) for r in seed_rows])
    mask = _dev_i64(PM.mask_combine(full, mask_rows))
    # a first good call of each kind, so that every record is set
    bufs = Bufs(D, B)
    assert _raw_dev(engine, sch, chacha, D, idx, clerk, bufs, seeds=seeds) == 0
    bufs = Bufs(D, B)
    counts = ([C.c_uint64(111 * (i + 1)) for i in range(5)], np.full(n_idx, 444, np.uint64))
    rec = _records(engine)

    def untouched():
        return (bufs.untouched() and _records(engine) == rec and [c.value for c in counts[0]] == [111, 222, 333, 444, 555]
                and (counts[1] == 444).all())

    # every FAULTS row of the recipient job's device form on a PackedShamir scheme: sda_recipient_job_dev's status
    for fname, form, kind, arg, _ in RC.FAULTS:
        if form != "dev":
            continue
        ms = chacha if kind == "chacha" else full
        kw = dict(seeds=seeds) if kind == "chacha" else dict(mask=mask)
        a = _raw_dev(engine, sch, ms, D, idx, clerk, bufs, fault=arg, decoded=False, **kw)
        b = _raw_dev(engine, sch, ms, D, idx, clerk, bufs, fault=arg, counts=counts, **kw)
        assert a != 0 and a == b, (fname, a, b)
        assert untouched(), fname
    # the decoded outputs' own NULLs, a misaligned wrong, a short out
    for arg in ("redundancy", "radius", "bad_batches", "first_bad", "undecoded", "blame", "out", "wrong+2"):
        assert _raw_dev(engine, sch, chacha, D, idx, clerk, bufs, seeds=seeds, fault=arg, counts=counts) == INVALID, arg
        assert untouched(), arg
    assert _raw_dev(engine, sch, chacha, D, idx, clerk, bufs, seeds=seeds, counts=counts, out_cap=D - 1) == INVALID
    assert untouched()
    # the job's own data-dependent statuses: too few results, a result shorter than B, repeated indices
    assert _raw_dev(engine, sch, chacha, D, idx[:kt - 1], DevBlobs(blobs[:kt - 1]), bufs, seeds=seeds,
                    counts=counts) == NOT_ENOUGH
    short = DevBlobs(blobs[:-1] + [_enc(oracle, rows[0][idx[-1]][:B - 1])])
    assert _raw_dev(engine, sch, chacha, D, idx, short, bufs, seeds=seeds, counts=counts) == PRECONDITION
    assert untouched()
    with pytest.raises(E.SdaError) as e:
        engine.recipient_job_decoded_dev(chacha, sch, D, [0] * n_idx, clerk.ptr(), clerk.off, p, bufs.out.ptr, D,
                                         seed_ptr=seeds.ptr(), seed_off=seeds.off, verdict_ptr=bufs.verdict.ptr,
                                         wrong_ptr=bufs.wrong.ptr)
    assert e.value.status == UNSUPPORTED and "distinct" in str(e.value)
    assert untouched()
    # repeated indices come after the out_cap check
    assert _raw_dev(engine, sch, chacha, D, [0] * n_idx, clerk, bufs, seeds=seeds, counts=counts, out_cap=D - 1) == INVALID
    # the scope refusals, each with its word, on the schemes alone (the buffers are never looked at)
    k9 = PMC.scheme_for(9, 6, 26)
    n80 = SCHEMES["n80"]
    mblobs = [_enc(oracle, r) for r in mask_rows]
    cl = list(zip(idx, blobs))
    for ms_, ss_, m_out, word in ((full, S.Additive(8, p), p, "Additive"), (S.FullMasking(k9.prime_modulus), k9,
                                                                          k9.prime_modulus, "secrets per batch"),
                                  (full, sch, p + 2, "output_modulus"), (S.FullMasking(p + 2), sch, p, "masking modulus"),
                                  (S.ChaChaMasking(p + 2, D, 128), sch, p, "masking modulus")):
        with pytest.raises(E.SdaError) as e:
            engine.recipient_job_decoded(ms_, mblobs, ss_, D, cl, m_out)
        assert e.value.status == UNSUPPORTED and word in str(e.value), str(e.value)
        with pytest.raises(E.SdaError) as e:
            engine.recipient_job_decoded_dev(ms_, ss_, D, idx, clerk.ptr(), clerk.off, m_out, bufs.out.ptr, D,
                                             mask_ptr=mask[1], mask_len=D, seed_ptr=seeds.ptr(), seed_off=seeds.off,
                                             verdict_ptr=bufs.verdict.ptr, wrong_ptr=bufs.wrong.ptr)
        assert e.value.status == UNSUPPORTED and word in str(e.value), str(e.value)
        assert untouched(), word
    # more than 32 results: refused where the job refuses more than 1023
    B80 = 3
    r80 = oracle.packed_generate(R._params(oracle, n80), np.arange(n80.secret_count * B80) % n80.prime_modulus,
                                 np.arange(B80 * n80.privacy_threshold()) % 7)
    with pytest.raises(E.SdaError) as e:
        engine.recipient_job_decoded(S.NoMasking(), [], n80, n80.secret_count * B80,
                                     [(i, _enc(oracle, r80[i])) for i in range(40)], n80.prime_modulus)
    assert e.value.status == UNSUPPORTED and "32" in str(e.value)
    assert untouched()


# ---------------------------------------------------------------- host form and reveal form through the C ABI
class HostOut:
    """caller-owned host outputs of sda_recipient_job_decoded, filled with sentinels"""

    def __init__(self, D, B, n_idx):
        self.out = np.full(D + 2, OUT_SENT, np.int64)
        self.verdict = np.full(B + 2, V_SENT, np.uint16)
        self.wrong = np.full(B + 2, W_SENT, np.uint32)
        self.counts = [C.c_uint64(111 * (i + 1)) for i in range(5)]
        self.blame = np.full(max(n_idx, 1), 444, np.uint64)
        self.olen = C.c_uint64(77)

    def untouched(self):
        return ((self.out == OUT_SENT).all() and (self.verdict == V_SENT).all() and (self.wrong == W_SENT).all()
                and [c.value for c in self.counts] == [111, 222, 333, 444, 555] and (self.blame == 444).all())

    def count_ptrs(self, fault=None):
        names = ("redundancy", "radius", "bad_batches", "first_bad", "undecoded")
        ptrs = [None if fault == n else C.byref(c) for n, c in zip(names, self.counts)]
        return ptrs + [None if fault == "blame" else E._ptr(self.blame, E._u64p)]


def _raw_host(eng, sch, ms, D, idx, mask_blobs, clerk_blobs, ho, fault=None, decoded=True, m_out=None, out_cap=None):
    """sda_recipient_job_decoded (or, decoded=False, sda_recipient_job) through ctypes -> status"""
    msc, ssc = ms.c(), sch.c()
    mbufs, mptrs, mlens, nm = E.Engine._blobs(mask_blobs)
    sbufs, sptrs, slens, ns = E.Engine._blobs(clerk_blobs)
    ia = np.asarray(list(idx) or [0], np.uint64)
    if fault == "mask_blob_0":
        mptrs[0] = None
    if fault == "clerk_blob_1":
        sptrs[1] = None
    a = {"ms": C.byref(msc), "mask_blobs": mptrs, "mask_lens": mlens, "ss": C.byref(ssc), "indices": E._ptr(ia, E._u64p),
         "clerk_blobs": sptrs, "clerk_lens": slens, "out_len": C.byref(ho.olen), "out": E._ptr(ho.out[1:], E._i64p)}
    if fault in a:
        a[fault] = None
    head = (eng.h, a["ms"], a["mask_blobs"], a["mask_lens"], nm, a["ss"], D, a["indices"], a["clerk_blobs"],
            a["clerk_lens"], ns, sch.prime_modulus if m_out is None else m_out)
    cap = D if out_cap is None else out_cap
    if decoded:
        return eng.lib.sda_recipient_job_decoded(*head, a["out"], cap, a["out_len"], ho.verdict[1:].ctypes.data,
                                                 ho.wrong[1:].ctypes.data, *ho.count_ptrs(fault))
    return eng.lib.sda_recipient_job(*head, E.REVEAL_CANONICAL, a["out"], cap, a["out_len"])


def _raw_reveal(eng, sch, ms, D, idx, shares_ptr, share_len, bufs, counts, fault=None):
    """sda_recipient_reveal_decoded_dev with no masking through ctypes -> status"""
    msc, ssc = ms.c(), sch.c()
    ia = np.asarray(list(idx), np.uint64)
    olen = C.c_uint64(77)
    names = ("redundancy", "radius", "bad_batches", "first_bad", "undecoded")
    cp = [None if fault == n else C.byref(c) for n, c in zip(names, counts[0])]
    cp.append(None if fault == "blame" else E._ptr(counts[1], E._u64p))
    a = {"ms": C.byref(msc), "ss": C.byref(ssc), "indices": E._ptr(ia, E._u64p), "shares": shares_ptr,
         "out": bufs.out.ptr, "out_len": C.byref(olen), "wrong": bufs.wrong.ptr}
    if fault in a:
        a[fault] = None
    if fault == "wrong+2":
        a["wrong"] += 2
    st = eng.lib.sda_recipient_reveal_decoded_dev(eng.h, a["ms"], None, 0, 0, a["ss"], D, a["indices"], a["shares"],
                                                  len(idx), share_len, sch.prime_modulus, a["out"], D, a["out_len"],
                                                  bufs.verdict.ptr, a["wrong"], *cp, None)
    bufs.out.torch.cuda.synchronize()
    return st


def test_host_and_reveal_forms_null_ladders_and_failing_calls_write_nothing(engine, oracle):
    name, n_idx, B = "b8", 8, 9
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    rows, secrets, D = _sharing(name, B, 0)
    idx = list(range(n_idx))
    blobs = [_enc(oracle, r) for r in rows[0][idx]]
    rng = np.random.default_rng(4)
    chacha, seed_rows = _masking("chacha8", p, D, rng)
    seed_blobs = [_enc(oracle, r) for r in seed_rows]
    full, mask_rows = _masking("full", p, D, rng)
    mblobs = [_enc(oracle, r) for r in mask_rows]
    # a good call first: it writes exactly its outputs, and every record is set
    ho = HostOut(D, B, n_idx)
    assert _raw_host(engine, sch, chacha, D, idx, seed_blobs, blobs, ho) == 0
    exp = RD.run(oracle, chacha, seed_rows, sch, D, list(zip(idx, rows[0][idx])))
    assert np.array_equal(ho.out[1:-1], exp.out) and ho.out[0] == ho.out[-1] == OUT_SENT
    assert np.array_equal(ho.verdict[1:-1], exp.verdict) and ho.verdict[0] == ho.verdict[-1] == V_SENT
    assert np.array_equal(ho.wrong[1:-1], exp.wrong) and ho.wrong[0] == ho.wrong[-1] == W_SENT
    assert [c.value for c in ho.counts] == [exp.redundancy, exp.radius, 0, E.CHECK_NO_BAD, 0] and not ho.blame.any()
    assert ho.olen.value == D
    rec = _records(engine)
    ho = HostOut(D, B, n_idx)

    def untouched():
        return ho.untouched() and _records(engine) == rec

    # every host-form row of FAULTS on a PackedShamir scheme: sda_recipient_job's status
    host_rows = [f for f in RC.FAULTS if f[1] == "host"]
    assert len(host_rows) == 10
    for fname, _, kind, arg, _ in host_rows:
        assert kind == "chacha"
        plain = HostOut(D, B, n_idx)
        a = _raw_host(engine, sch, chacha, D, idx, seed_blobs, blobs, plain, fault=arg, decoded=False)
        b = _raw_host(engine, sch, chacha, D, idx, seed_blobs, blobs, ho, fault=arg)
        assert a != 0 and a == b, (fname, a, b)
        assert untouched(), fname
    # the decoded outputs' own NULLs
    for arg in ("redundancy", "radius", "bad_batches", "first_bad", "undecoded", "blame", "out"):
        assert _raw_host(engine, sch, chacha, D, idx, seed_blobs, blobs, ho, fault=arg) == INVALID, arg
        assert untouched(), arg
    # failing calls of every stage leave the caller's host memory and the records alone
    k9 = PMC.scheme_for(9, 6, 26)
    assert _raw_host(engine, sch, full, D, idx[:kt - 1], mblobs, blobs[:kt - 1], ho) == NOT_ENOUGH
    assert untouched()
    assert _raw_host(engine, sch, full, D, [0] * n_idx, mblobs, blobs, ho) == UNSUPPORTED           # repeated indices
    assert "distinct" in engine.lib.sda_last_error_message().decode() and untouched()
    assert _raw_host(engine, sch, full, D, idx, mblobs, blobs, ho, out_cap=D - 1) == INVALID
    assert "too small" in engine.lib.sda_last_error_message().decode() and untouched()
    assert _raw_host(engine, sch, full, D, [0] * n_idx, mblobs, blobs, ho, out_cap=D - 1) == INVALID   # cap comes first
    assert untouched()
    short = blobs[:-1] + [_enc(oracle, rows[0][idx[-1]][:B - 1])]
    assert _raw_host(engine, sch, full, D, idx, mblobs, short, ho) == PRECONDITION
    assert untouched()
    for ms_, ss_, m_out in ((full, S.Additive(8, p), p), (S.FullMasking(k9.prime_modulus), k9, k9.prime_modulus),
                            (full, sch, p + 2), (S.FullMasking(p + 2), sch, p), (S.ChaChaMasking(p + 2, D, 256), sch, p)):
        assert _raw_host(engine, ss_, ms_, D, idx, mblobs, blobs, ho, m_out=m_out) == UNSUPPORTED
        assert untouched()
    # the reveal form: its NULL ladder and a misaligned wrong
    sh, sh_ptr = _dev_i64(rows[0][idx])
    bufs = Bufs(D, B)
    counts = ([C.c_uint64(111 * (i + 1)) for i in range(5)], np.full(n_idx, 444, np.uint64))
    none = S.NoMasking()
    for arg in ("ms", "ss", "indices", "shares", "out", "out_len", "redundancy", "radius", "bad_batches", "first_bad",
                "undecoded", "blame", "wrong+2"):
        assert _raw_reveal(engine, sch, none, D, idx, sh_ptr, B, bufs, counts, fault=arg) == INVALID, arg
        assert bufs.untouched() and _records(engine) == rec, arg
        assert [c.value for c in counts[0]] == [111, 222, 333, 444, 555] and (counts[1] == 444).all(), arg
    assert _raw_reveal(engine, sch, none, D, idx, sh_ptr, B, bufs, counts) == 0
    assert np.array_equal(bufs.out.host(), bufs.out.expect(secrets[0] % p))


# ---------------------------------------------------------------- every i64 mask value is reduced exactly
@pytest.mark.parametrize("fuse", ("1", "0"))
@pytest.mark.parametrize("out_off,mask_off", ((0, 0), (0, 1), (1, 0), (1, 1)))
def test_edge_mask_values_are_reduced_exactly_on_the_device(engine, oracle, monkeypatch, out_off, mask_off, fuse):
    """A Full mask holding 0, +-1, +-(p - 1), +-p, the ends of i64 and other values far outside (-p, p), handed to the
    device form as its combined mask: compared with the big-integer model only (the composition of today's calls
    unmasks with a wrapping `-`, which leaves the residue class at these values).  Both alignments of the mask (one
    16-byte load a pair, or two 8-byte loads) and of `out`, both routes, with one whole wrong payload so that the
    decode pass corrects residues the mask has already been subtracted from."""
    name, n_idx, B = "config", 19, 257
    sch = SCHEMES[name]
    p = sch.prime_modulus
    rows, secrets, D = _sharing(name, B, 1)
    idx = np.random.default_rng(19).permutation(sch.share_count)[:n_idx].tolist()
    edge = [0, 1, -1, p - 1, -(p - 1), p, -p, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 2 * p, -2 * p, 2**32,
            -2**32, 2**32 - 1, 2**62 + 12345, -(2**62) - 12345, (p << 32) + 7, -(p << 32) - 7, 2**63 - p, p - 2**63, 5]
    mask = [edge[(3 * i + i // len(edge)) % len(edge)] for i in range(D)]
    assert set(mask) == set(edge)
    full = S.FullMasking(p)
    sh = rows[0][idx].copy()
    sh[4] = _wrong_row(rows, idx[4], p)
    exp = RD.run(oracle, full, None, sch, D, list(zip(idx, sh)), mask=mask)
    assert np.array_equal(exp.out, np.asarray([(int(s) - m) % p for s, m in zip(secrets[0], mask)], np.int64))
    assert exp.bad_batches == B and exp.undecoded == 0
    monkeypatch.setenv("SDA_RECIPIENT_FUSE_UNMASK", fuse)
    keep, mptr = _dev_i64(mask, mask_off)
    bufs = Bufs(D, B, out_off)
    clerk = DevBlobs([_enc(oracle, r) for r in sh])
    n, dec = engine.recipient_job_decoded_dev(full, sch, D, idx, clerk.ptr(), clerk.off, p, bufs.out.ptr, D,
                                              mask_ptr=mptr, mask_len=D, verdict_ptr=bufs.verdict.ptr,
                                              wrong_ptr=bufs.wrong.ptr)
    assert (n, dec) == (D, _decode_tuple(exp))
    bufs.check(exp, f"route {fuse}")
    assert tuple(engine.recipient_decoded_last_launch()) == (1 if fuse == "1" else 2, 1, 0)


def test_record_is_all_zeros_before_the_first_robust_call():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    e = E.Engine(0)
    try:
        assert tuple(e.recipient_decoded_last_launch()) == (0, 0, 0)
    finally:
        e.close()
