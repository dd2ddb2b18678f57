"""GPU: the argument checks of the `_dev` entry points that share one launch body (the four combines, the three
packed generates, the two packed reconstructs, the two encodes, the two participant calls): one failing call per
branch, with the status and the message (sda_last_error_message) it returns, in a table; and one passing call per
entry point at the smallest shape that launches, against the oracle.

The failing calls go to the library directly (ctypes), so that NULL handles, NULL schemes and NULL counters -- which
the Engine wrappers never pass -- are reachable.  All of them fail before a launch except the two "cap too small"
kinds, whose count pass runs over valid buffers and writes nothing."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from sda_amd import schemes as S
from sda_amd import engine as E
from tests.util import assert_same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = S.CONFIG_PACKED.prime_modulus
I64_MIN = -(1 << 63)
# k = 1, t = 0, n = 2 over p = 433: k + t + 1 = 2 and n + 1 = 3, with -1 of order 2 and 150^3 of order 3
# (150 is full_loop.rs' omega_shares, of order 9)
TINY = S.PackedShamir(1, 2, 0, 433, 432, pow(150, 3, 433))
NO_K = S.PackedShamir(0, 2, 0, 433, 432, pow(150, 3, 433))           # check_packed's first refusal
ADD = S.Additive(3, 433)
EXACT, CANON, BAD_MODE = E.REVEAL_EXACT, E.REVEAL_CANONICAL, 7

INVALID, PRECOND, UNSUPP = E.ERR_INVALID_ARGUMENT, E.ERR_PRECONDITION, E.ERR_UNSUPPORTED
NULL_ARG = "NULL argument"
NEED_PACKED = "need a PackedShamir scheme"
NO_K_MSG = "secret_count must be >= 1"
REM_ZERO = "attempt to calculate the remainder with a divisor of zero"
MIN_MOD = "modulus i64::MIN is outside the engine's domain"
GEN_RANGE = "Rng.gen_range called with low >= high"
VECTORS = "at most 65535 vectors per launch"
ADD32 = ("int32 shares need a PackedShamir scheme: an additive scheme's first n - 1 shares are the caller's draws, "
         "copied unchecked")


@pytest.fixture(scope="module")
def b(engine):
    """Handle, stream and a few small valid buffers; the schemes as C structs that outlive the calls."""
    ns = SimpleNamespace(h=engine.h, lib=engine.lib, stream=torch.cuda.current_stream().cuda_stream)
    ns.t64 = torch.arange(1, 17, dtype=torch.int64, device="cuda")
    ns.t32 = torch.arange(1, 17, dtype=torch.int32, device="cuda")
    ns.tout = torch.zeros(16, dtype=torch.int64, device="cuda")
    ns.tout32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    ns.tbytes = torch.zeros(256, dtype=torch.uint8, device="cuda")
    ns.x64, ns.x32, ns.out, ns.out32, ns.bytes = (t.data_ptr() for t in (ns.t64, ns.t32, ns.tout, ns.tout32, ns.tbytes))
    ns.rb_arr = np.zeros(4, np.uint64)
    ns.rb = ns.rb_arr.ctypes.data_as(C.POINTER(C.c_uint64))
    ns.idx_arr, ns.dup_arr = np.array([0, 1], np.uint64), np.array([0, 0], np.uint64)
    ns.idx = ns.idx_arr.ctypes.data_as(C.POINTER(C.c_uint64))
    ns.dup = ns.dup_arr.ctypes.data_as(C.POINTER(C.c_uint64))
    ns.seed_arr = np.arange(4, dtype=np.uint32)
    ns.seed = ns.seed_arr.ctypes.data_as(C.POINTER(C.c_uint32))
    ns.structs = {}
    yield ns
    torch.cuda.synchronize()


def _ref(b, scheme):
    """byref of the scheme's C struct, or NULL."""
    if scheme is None:
        return None
    if scheme not in b.structs:
        b.structs[scheme] = scheme.c()
    return C.byref(b.structs[scheme])


def _val(b, v):
    """A table value: the name of one of the fixture's buffers, or the value itself."""
    return getattr(b, v) if isinstance(v, str) else v


# ---- argument builders: the defaults make a valid call, a case overrides what its branch needs ----
def combine_args(b, **kw):
    d = dict(h=b.h, m=P, shares="x64", n=2, dim=5, stride=6, out="out")
    d.update(kw)
    return tuple(_val(b, d[k]) for k in ("h", "m", "shares", "n", "dim", "stride", "out")) + (b.stream,)


def generate_args(b, with_mode=True, **kw):
    d = dict(h=b.h, s=TINY, secrets="x64", dim=3, nvec=1, draws="x64", out="out", mode=EXACT)
    d.update(kw)
    head = (d["h"], _ref(b, d["s"]), _val(b, d["secrets"]), d["dim"], d["nvec"], _val(b, d["draws"]), _val(b, d["out"]))
    return head + ((d["mode"],) if with_mode else ()) + (b.stream,)


def reconstruct_args(b, **kw):
    d = dict(h=b.h, s=TINY, dim=3, idx="idx", n_idx=2, nvec=1, shares="x64", out="out", mode=EXACT)
    d.update(kw)
    return (d["h"], _ref(b, d["s"]), d["dim"], _val(b, d["idx"]), d["n_idx"], d["nvec"], _val(b, d["shares"]),
            _val(b, d["out"]), d["mode"], b.stream)


def encode_args(b, **kw):
    d = dict(h=b.h, vals="x64", rows=2, len=3, stride=3, dst="bytes", cap=256, rb="rb")
    d.update(kw)
    return tuple(_val(b, d[k]) for k in ("h", "vals", "rows", "len", "stride", "dst", "cap", "rb")) + (b.stream,)


def participant_args(b, **kw):
    d = dict(h=b.h, ms=S.NoMasking(), seed=None, seed_words=0, full=None, ss=TINY, secrets="x64", dim=3, draws="x64",
             mode=EXACT, out="out", payload=None, cap=0, rb="rb")
    d.update(kw)
    return (d["h"], _ref(b, d["ms"]), _val(b, d["seed"]), d["seed_words"], _val(b, d["full"]), _ref(b, d["ss"]),
            _val(b, d["secrets"]), d["dim"], _val(b, d["draws"]), d["mode"], _val(b, d["out"]), _val(b, d["payload"]),
            d["cap"], _val(b, d["rb"]), b.stream)


def _table():
    """(entry point, argument builder, the entry point's own defaults, the case's overrides, status, message)"""
    t = []

    def add(fn, build, fixed, what, status, msg, **kw):
        t.append(pytest.param(fn, build, fixed, kw, status, msg, id=f"{fn[4:]}-{what}"))

    for fn, sh in (("sda_combine_dev", "x64"), ("sda_combine_accumulate_dev", "x64"), ("sda_combine32_dev", "x32"),
                   ("sda_combine32_accumulate_dev", "x32")):
        c = (fn, combine_args, dict(shares=sh))
        add(*c, "null_handle", INVALID, NULL_ARG, h=None)
        add(*c, "null_out", INVALID, NULL_ARG, out=None)
        add(*c, "null_shares", INVALID, NULL_ARG, shares=None)
        add(*c, "stride", INVALID, "row_stride < dim", stride=4)
        add(*c, "stride_before_modulus", INVALID, "row_stride < dim", stride=4, m=0)
        add(*c, "modulus_zero", PRECOND, REM_ZERO, m=0)
        add(*c, "modulus_min", UNSUPP, MIN_MOD, m=I64_MIN)

    for fn, with_mode, out in (("sda_packed_generate_dev", False, "out"), ("sda_packed_generate_mode_dev", True, "out"),
                               ("sda_packed_generate32_dev", True, "out32")):
        c = (fn, generate_args, dict(with_mode=with_mode, out=out))
        add(*c, "null_handle", INVALID, NEED_PACKED, h=None)
        add(*c, "null_scheme", INVALID, NEED_PACKED, s=None)
        add(*c, "additive", INVALID, NEED_PACKED, s=ADD)
        add(*c, "check_packed", UNSUPP, NO_K_MSG, s=NO_K)
        add(*c, "vectors", UNSUPP, VECTORS, nvec=65536)
        if with_mode:
            add(*c, "bad_mode", INVALID, "bad mode", mode=BAD_MODE)
            add(*c, "bad_mode_before_check_packed", INVALID, "bad mode", mode=BAD_MODE, s=NO_K)
    c = ("sda_packed_generate32_dev", generate_args, dict(out="out32"))
    add(*c, "null_out", INVALID, NULL_ARG, out=None)
    add(*c, "null_secrets", INVALID, NULL_ARG, secrets=None)
    add(*c, "null_draws", INVALID, NULL_ARG, draws=None, s=S.FULL_LOOP_PACKED)
    add(*c, "vectors_before_null", UNSUPP, VECTORS, nvec=65536, out=None)

    for fn, sh in (("sda_packed_reconstruct_dev", "x64"), ("sda_packed_reconstruct32_dev", "x32")):
        c = (fn, reconstruct_args, dict(shares=sh))
        add(*c, "null_handle", INVALID, NEED_PACKED, h=None)
        add(*c, "null_scheme", INVALID, NEED_PACKED, s=None)
        add(*c, "additive", INVALID, NEED_PACKED, s=ADD)
        add(*c, "check_packed", UNSUPP, NO_K_MSG, s=NO_K)
        add(*c, "check_packed_before_bad_mode", UNSUPP, NO_K_MSG, s=NO_K, mode=BAD_MODE)
        add(*c, "bad_mode", INVALID, "bad mode", mode=BAD_MODE)
        add(*c, "bad_mode_at_dimension_0", INVALID, "bad mode", mode=BAD_MODE, dim=0)
        add(*c, "not_enough", E.ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct", n_idx=0)
        add(*c, "too_many", UNSUPP, "more than 1023 clerk shares per batch", n_idx=1024)
        add(*c, "vectors", UNSUPP, VECTORS, nvec=65536)
        add(*c, "duplicate_indices", UNSUPP, "canonical reveal needs distinct clerk indices", idx="dup", mode=CANON)
    c = ("sda_packed_reconstruct32_dev", reconstruct_args, dict(shares="x32"))
    add(*c, "null_out", INVALID, NULL_ARG, out=None)
    add(*c, "null_shares", INVALID, NULL_ARG, shares=None)
    add(*c, "null_indices", INVALID, NULL_ARG, idx=None)
    add(*c, "vectors_before_null", UNSUPP, VECTORS, nvec=65536, out=None)

    for fn, vals in (("sda_varint_encode_dev", "x64"), ("sda_varint_encode32_dev", "x32")):
        c = (fn, encode_args, dict(vals=vals))
        add(*c, "null_handle", INVALID, NULL_ARG, h=None)
        add(*c, "null_row_bytes", INVALID, NULL_ARG, rb=None)
        add(*c, "null_vals", INVALID, NULL_ARG, vals=None)
        add(*c, "null_dst", INVALID, NULL_ARG, dst=None)
        add(*c, "rows", UNSUPP, "at most 65535 rows per call", rows=65536)
        add(*c, "rows_before_stride", UNSUPP, "at most 65535 rows per call", rows=65536, stride=2)
        add(*c, "stride", INVALID, "stride < len", stride=2)
        add(*c, "dst_cap", INVALID, "dst_cap too small", cap=1)

    chacha = S.ChaChaMasking(433, 3, 128)
    for fn, out in (("sda_participant_share_dev", "out"), ("sda_participant_share32_dev", "out32")):
        c = (fn, participant_args, dict(out=out))
        add(*c, "null_handle", INVALID, NULL_ARG, h=None)
        add(*c, "null_masking", INVALID, NULL_ARG, ms=None)
        add(*c, "null_sharing", INVALID, NULL_ARG, ss=None)
        add(*c, "null_secrets", INVALID, NULL_ARG, secrets=None)
        add(*c, "null_shares", INVALID, NULL_ARG, out=None)
        add(*c, "null_row_bytes", INVALID, NULL_ARG, payload="bytes", cap=256, rb=None)
        add(*c, "sharing_kind", INVALID, "unknown sharing scheme kind", ss=_OtherKind(sharing=True))
        add(*c, "bad_mode", INVALID, "bad mode", mode=BAD_MODE)
        add(*c, "check_packed", UNSUPP, NO_K_MSG, ss=NO_K)
        add(*c, "mask_modulus", PRECOND, GEN_RANGE, ms=S.FullMasking(0), full="x64")
        add(*c, "full_without_masks", INVALID, "Full masking needs the drawn masks", ms=S.FullMasking(433))
        add(*c, "chacha_dimension", PRECOND, "assertion failed: dimension == secrets.len()",
            ms=S.ChaChaMasking(433, 4, 128), seed="seed", seed_words=4)
        add(*c, "chacha_seed_words", PRECOND, "expected 4 seed words", ms=chacha, seed="seed", seed_words=3)
        add(*c, "chacha_null_seed", PRECOND, "expected 4 seed words", ms=chacha, seed=None, seed_words=4)
        add(*c, "masking_kind", INVALID, "unknown masking scheme kind", ms=_OtherKind(sharing=False))
        add(*c, "null_draws", INVALID, "need the randomness draws", draws=None)
        add(*c, "payload_cap", INVALID, "payload_cap too small", payload="bytes", cap=1)
    c = ("sda_participant_share_dev", participant_args, dict(out="out"))
    add(*c, "additive_no_clerks", PRECOND, "share_count - 1 underflows (additive.rs:42)", ss=S.Additive(0, 433))
    add(*c, "additive_modulus", PRECOND, GEN_RANGE, ss=S.Additive(3, 0))
    add(*c, "clerks", UNSUPP, "at most 65535 clerks", ss=S.Additive(65536, 433), payload="bytes", cap=256)
    c = ("sda_participant_share32_dev", participant_args, dict(out="out32"))
    add(*c, "additive", UNSUPP, ADD32, ss=ADD)
    add(*c, "additive_before_bad_mode", UNSUPP, ADD32, ss=ADD, mode=BAD_MODE)
    return t


class _OtherKind:
    """A scheme struct of a kind the header does not define."""

    def __init__(self, sharing):
        self.sharing = sharing

    def __hash__(self):
        return hash(("other", self.sharing))

    def __eq__(self, o):
        return isinstance(o, _OtherKind) and o.sharing == self.sharing

    def c(self):
        return S.SharingSchemeC(9, 2, 433, 1, 0, 432, 198) if self.sharing else S.MaskingSchemeC(9, 433, 3, 128)


@pytest.mark.parametrize("fn,build,fixed,overrides,status,msg", _table())
def test_failing_call(b, fn, build, fixed, overrides, status, msg):
    st = getattr(b.lib, fn)(*build(b, **{**fixed, **overrides}))
    got = b.lib.sda_last_error_message().decode()
    assert (st, got) == (status, msg)


def test_reconstruct_of_dimension_0_checks_nothing_more(b):
    """batched.rs:77-81: no batch, no check -- too few indices, too many vectors and NULL buffers pass."""
    for fn, sh in (("sda_packed_reconstruct_dev", "x64"), ("sda_packed_reconstruct32_dev", "x32")):
        st = getattr(b.lib, fn)(*reconstruct_args(b, dim=0, n_idx=0, nvec=65536, out=None, shares=None, idx=None))
        assert (st, b.lib.sda_last_error_message().decode()) == (E.OK, "")


# ---------------- passing calls, smallest shapes that launch ----------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


ROWS = np.array([[5, -7, 432, 1000, -1, 77], [-433, 9, 1, -1000, 433, 88]], np.int64)   # [2][dim 5 + 1 of padding]


@pytest.mark.parametrize("wide", [True, False], ids=["i64", "i32"])
def test_combine_passes(engine, oracle, wide):
    m, dim, stride = 433, 5, 6
    x = torch.from_numpy(ROWS if wide else ROWS.astype(np.int32)).cuda()
    plain = engine.combine_dev if wide else engine.combine32_dev
    accumulate = engine.combine_accumulate_dev if wide else engine.combine32_accumulate_dev
    exp = oracle.combine(m, ROWS[:, :dim])
    out = torch.full((dim + 1,), -12345, dtype=torch.int64, device="cuda")
    plain(m, x.data_ptr(), 2, dim, stride, out.data_ptr(), _stream())              # n > 1: the row stride counts
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), list(exp) + [-12345], "n = 2, dim = 5, row_stride = 6")
    # n = 1: the stride is not read, so one below dim passes; then row 1 continues the recurrence
    out.fill_(-12345)
    plain(m, x.data_ptr(), 1, dim, dim - 1, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), list(oracle.combine(m, ROWS[:1, :dim])) + [-12345], "n = 1, row_stride < dim")
    accumulate(m, x[1].data_ptr(), 1, dim, dim - 1, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), list(exp) + [-12345], "accumulate, n = 1, row_stride < dim")
    out.fill_(-12345)
    accumulate(m, x.data_ptr(), 0, dim, stride, out.data_ptr(), _stream())        # n == 0: inout untouched
    accumulate(m, None, 0, dim, 0, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), [-12345] * (dim + 1), "accumulate, n = 0")
    plain(m, x.data_ptr(), 0, dim, stride, out.data_ptr(), _stream())             # the plain form launches: zeros
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), [0] * dim + [-12345], "n = 0")
    out.fill_(7)
    accumulate(m, x.data_ptr(), 2, dim, stride, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    seven = np.full((1, dim), 7, np.int64)
    assert_same(out.cpu().numpy(), list(oracle.combine(m, np.concatenate([seven, ROWS[:, :dim]]))) + [7],
                "accumulate, n = 2, dim = 5, row_stride = 6")


SECRETS = np.array([5, -7, 432], np.int64)                             # D = 3: three batches of k = 1


@pytest.fixture(scope="module")
def tiny_shares(oracle):
    """[n = 2][B = 3] shares of SECRETS under TINY (t = 0: no draws), computed once."""
    pp = oracle.packed_params(1, 2, 0, 433, 432, pow(150, 3, 433))
    return pp, oracle.packed_generate(pp, SECRETS, np.zeros(0, np.int64))


def test_packed_generate_passes(engine, tiny_shares):
    exp = tiny_shares[1]
    sec = torch.from_numpy(SECRETS).cuda()
    draws = torch.zeros(1, dtype=torch.int64, device="cuda")            # t = 0: never read
    out = torch.full((2, 3), -1, dtype=torch.int64, device="cuda")
    engine.packed_generate_dev(TINY, sec.data_ptr(), 3, 1, draws.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), exp, "sda_packed_generate_dev")
    # the canonical forms give each share's residue in [0, p)
    for mode, want in ((EXACT, exp), (CANON, np.mod(exp, 433))):
        out.fill_(-1)
        engine.packed_generate_mode_dev(TINY, sec.data_ptr(), 3, 1, draws.data_ptr(), out.data_ptr(), mode, _stream())
        out32 = torch.full((2, 3), -1, dtype=torch.int32, device="cuda")
        engine.packed_generate32_dev(TINY, sec.data_ptr(), 3, 1, draws.data_ptr(), out32.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy(), want, f"sda_packed_generate_mode_dev, mode {mode}")
        assert_same(out32.cpu().numpy(), want, f"sda_packed_generate32_dev, mode {mode}")


def test_packed_reconstruct_passes(engine, oracle, tiny_shares):
    pp, shares = tiny_shares
    rc, exp = oracle.packed_reconstruct(pp, 3, [0, 1], shares)
    assert rc == 0
    sh = torch.from_numpy(shares).cuda()
    sh32 = torch.from_numpy(shares.astype(np.int32)).cuda()
    for mode, want in ((EXACT, exp), (CANON, np.mod(exp, 433))):
        out = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        out32 = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        engine.packed_reconstruct_dev(TINY, 3, [0, 1], 1, sh.data_ptr(), out.data_ptr(), mode, _stream())
        engine.packed_reconstruct32_dev(TINY, 3, [0, 1], 1, sh32.data_ptr(), out32.data_ptr(), mode, _stream())
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy(), want, f"sda_packed_reconstruct_dev, mode {mode}")
        assert_same(out32.cpu().numpy(), want, f"sda_packed_reconstruct32_dev, mode {mode}")
    assert_same(np.mod(exp, 433), np.mod(SECRETS, 433), "the reconstruction is the secrets")


def _blobs(buf, row_bytes):
    host = buf.cpu().numpy().tobytes()
    off = np.concatenate([[0], np.cumsum(row_bytes)]).astype(np.int64)
    return [host[off[r]:off[r + 1]] for r in range(len(row_bytes))]


def test_encode_passes(engine, oracle):
    vals = np.array([[0, -1, 300, 99], [1 << 30, -(1 << 31), 63, 99]], np.int64)   # 2 rows x 3 values, stride 4
    exp = [oracle.varint_encode(vals[r, :3]) for r in range(2)]
    for fn, x in ((engine.varint_encode_dev, torch.from_numpy(vals).cuda()),
                  (engine.varint_encode32_dev, torch.from_numpy(vals.astype(np.int32)).cuda())):
        dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
        rb = fn(x.data_ptr(), 2, 3, 4, dst.data_ptr(), 64, _stream())
        torch.cuda.synchronize()
        assert _blobs(dst, rb) == exp


def test_participant_passes(engine, oracle, tiny_shares):
    exp = tiny_shares[1]
    sec = torch.from_numpy(SECRETS).cuda()
    draws = torch.zeros(1, dtype=torch.int64, device="cuda")            # t = 0: never read
    want = [oracle.varint_encode(exp[c]) for c in range(2)]
    for fn, dtype in ((engine.participant_share_dev, torch.int64), (engine.participant_share32_dev, torch.int32)):
        out = torch.full((2, 3), -1, dtype=dtype, device="cuda")
        pay = torch.zeros(96, dtype=torch.uint8, device="cuda")
        rb = fn(S.NoMasking(), TINY, sec.data_ptr(), 3, draws.data_ptr(), out.data_ptr(), payload_ptr=pay.data_ptr(),
                payload_cap=96, stream=_stream())
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy(), exp, fn.__name__)
        assert _blobs(pay, rb) == want
