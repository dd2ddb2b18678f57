"""GPU: packed-Shamir share generation with in-kernel draws (sda_packed_generate_keyed_dev and its int32 form), the
record of where the draws were made (sda_packed_keyed_last_launch), and the callers that go through the keyed launch.

The contract under test: the keyed call is bit-identical to sda_draws_dev(key, stream_id, first_batch t,
n_vectors B t, p - 1) fed to the unkeyed entry point, in both modes and widths, with the same fix-up count.  So most
tests compare whole output buffers of the two calls; tests/test_gpu_draws.py holds sda_draws_dev to the CPU model and
tests/test_gpu_packed_matrix.py the unkeyed kernels to the oracle, and test_cpu_anchor closes the loop directly.
The plan's claims (slice residues, planted tiles) are checked on the CPU in tests/test_packed_keyed_model.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from sda_amd import Engine, SdaError, schemes as S
from sda_amd import engine as E
from tests import draws_model as DM
from tests import packed_dispatch as PD
from tests import packed_matrix_cases as PM
from tests import test_packed_keyed_model as KM
from tests.test_gpu_packed_matrix import gen_inputs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEY, STREAM, V = KM.KEY, KM.STREAM, PM.V
SENT64, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
GUARD = 16                                  # guard bytes before and after the output
WIDTHS = [False, True]
MODES = (PD.EXACT, PD.CANONICAL)


def _dev(a):
    """a on the device (int64), 16-byte aligned, never empty"""
    flat = np.concatenate([np.ascontiguousarray(a, dtype=np.int64).reshape(-1), np.zeros(2, np.int64)])
    d = torch.as_tensor(flat).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def _out(words, narrow, offset=0):
    """(buffer, output pointer): `words` shares behind GUARD + offset bytes of sentinel, GUARD bytes after"""
    size = 8 if not narrow else 4
    pad = (GUARD + offset) // size
    buf = torch.full((pad + words + GUARD // size + 2,), SENT32 if narrow else SENT64,
                     dtype=torch.int32 if narrow else torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + GUARD + offset


def _generate(engine, sch, secrets, D, nvec, mode, narrow, first=0, keyed=True, offset=0, stream_id=STREAM,
              key=KEY):
    """(whole buffer incl. guards, fix-up count) of one call; keyed=False feeds sda_draws_dev's draws."""
    k, t, n = sch.secret_count, sch.privacy_threshold(), sch.share_count
    B = (D + k - 1) // k
    buf, ptr = _out(nvec * n * B, narrow, offset)
    if keyed:
        call = engine.packed_generate_keyed32_dev if narrow else engine.packed_generate_keyed_dev
        call(sch, secrets.data_ptr(), D, nvec, key, stream_id, ptr, mode, first_batch=first)
    else:
        count = nvec * B * t
        draws = torch.zeros(count + 2, dtype=torch.int64, device="cuda")
        engine.draws_dev(key, stream_id, first * t, count, sch.prime_modulus - 1, draws.data_ptr())
        call = engine.packed_generate32_dev if narrow else engine.packed_generate_mode_dev
        call(sch, secrets.data_ptr(), D, nvec, draws.data_ptr(), ptr, mode)
    count = engine.packed_fixup_count()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), count


def _shares(host, sch, B, nvec, narrow, offset=0):
    """the [nvec][n][B] shares of a _generate buffer; asserts the guards"""
    size = 4 if narrow else 8
    pad, words = (GUARD + offset) // size, nvec * sch.share_count * B
    sent = SENT32 if narrow else SENT64
    assert (host[:pad] == sent).all() and (host[pad + words:] == sent).all(), "wrote outside the output"
    return host[pad:pad + words].reshape(nvec, sch.share_count, B)


# ---------------------------------------------------------------------------------------------------------------
# 1. kernel matrix
# ---------------------------------------------------------------------------------------------------------------
MATRIX = [c for c in PM.GEN_CASES if c.sch.share_count + 1 <= 27]


@pytest.mark.parametrize("case", MATRIX, ids=lambda c: c.id)
def test_kernel_matrix(engine, case):
    """Every register-path share-gen case up to n + 1 = 27 (two full tiles and a ragged one, an unaligned vector, PAD
    and unpadded layouts, t = 0), i64 and int32, at first_batch 0 and at an odd one."""
    sch = case.sch
    assert case.kernel != "wide"
    secrets = gen_inputs(sch, case.B)[0]
    D = secrets.shape[1]
    ds = _dev(secrets)
    old = os.environ.pop("SDA_GEN_SIGNBIT", None)
    try:
        if case.signbit_env is not None:
            os.environ["SDA_GEN_SIGNBIT"] = case.signbit_env
        for narrow in WIDTHS:
            for first in (0, KM.ODD_FIRST):
                want, wc = _generate(engine, sch, ds, D, V, case.mode, narrow, first, keyed=False,
                                     offset=case.out_offset)
                got, gc = _generate(engine, sch, ds, D, V, case.mode, narrow, first, offset=case.out_offset)
                assert engine.packed_keyed_last_launch() == (1, 0), case.id
                _shares(want, sch, case.B, V, narrow, case.out_offset)
                assert np.array_equal(got, want), (case.id, narrow, first)
                assert gc == wc and gc >= 2, (case.id, narrow, first, gc, wc)      # gen_inputs plants raw secrets
    finally:
        os.environ.pop("SDA_GEN_SIGNBIT", None)
        if old is not None:
            os.environ["SDA_GEN_SIGNBIT"] = old


# ---------------------------------------------------------------------------------------------------------------
# 2. fix-up: the keyed fix-up kernel makes a logged batch's draws itself
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", WIDTHS, ids=["i64", "int32"])
@pytest.mark.parametrize("mode", MODES, ids=["exact", "canon"])
def test_fixup_draws(engine, mode, narrow):
    sch = S.CONFIG_PACKED
    p, k = sch.prime_modulus, sch.secret_count
    B = KM.FIX_B
    D = B * k
    rng = np.random.default_rng(11)
    secrets = rng.integers(0, p, size=(V, D), dtype=np.int64)
    for v, b in KM.FIX_PLANTS:
        secrets[v, b * k + (v + b) % k] = (1 << 40) + 12345 * (v + 1)
    ds = _dev(secrets)
    for first in (0, KM.ODD_FIRST):
        want, wc = _generate(engine, sch, ds, D, V, mode, narrow, first, keyed=False)
        got, gc = _generate(engine, sch, ds, D, V, mode, narrow, first)
        assert gc == wc and gc >= 2 * len(KM.FIX_PLANTS), (gc, wc)
        assert np.array_equal(got, want)
        sh = _shares(got, sch, B, V, narrow)
        if mode == PD.CANONICAL:
            assert 0 <= sh.min() and sh.max() < p


# ---------------------------------------------------------------------------------------------------------------
# 3. first_batch is a batch slice
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", WIDTHS, ids=["i64", "int32"])
@pytest.mark.parametrize("sch", KM.SLICE_SCHEMES, ids=PM.sid)
def test_first_batch_is_a_batch_slice(engine, sch, narrow):
    p, k = sch.prime_modulus, sch.secret_count
    B = KM.SLICE_B
    D = PM.dimension(B, k)
    secrets = np.random.default_rng(B + k).integers(0, p, size=D, dtype=np.int64)
    for mode in MODES:
        whole = _shares(_generate(engine, sch, _dev(secrets), D, 1, mode, narrow)[0], sch, B, 1, narrow)[0]
        for f, w in KM.SLICES:
            part = secrets[f * k:min(D, (f + w) * k)]
            got = _shares(_generate(engine, sch, _dev(part), part.size, 1, mode, narrow, first=f)[0], sch, w, 1, narrow)
            assert np.array_equal(got[0], whole[:, f:f + w]), (f, w, mode)
    # n_vectors = 3: vector v is the one-vector call at first_batch = v B
    Bv = 300
    Dv = PM.dimension(Bv, k)
    sec3 = np.random.default_rng(Bv).integers(0, p, size=(V, Dv), dtype=np.int64)
    three = _shares(_generate(engine, sch, _dev(sec3), Dv, V, PD.EXACT, narrow, first=7)[0], sch, Bv, V, narrow)
    for v in range(V):
        one = _shares(_generate(engine, sch, _dev(sec3[v]), Dv, 1, PD.EXACT, narrow, first=7 + v * Bv)[0], sch, Bv, 1,
                      narrow)
        assert np.array_equal(one[0], three[v]), v


# ---------------------------------------------------------------------------------------------------------------
# 4. CPU anchor
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sch,B", [("config", S.CONFIG_PACKED, 300), ("full_loop", S.FULL_LOOP_PACKED, 41)])
def test_cpu_anchor(engine, oracle, name, sch, B):
    """The shares from the CPU alone: the oracle's packed_generate over the draws model."""
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    D = B * k
    secrets = np.random.default_rng(B).integers(0, p, size=D, dtype=np.int64)
    pp = oracle.packed_params(k, n, t, p, sch.omega_secrets, sch.omega_shares)
    first = 5
    draws = DM.draws(KEY, STREAM, first * t, B * t, p - 1)
    exp = oracle.packed_generate(pp, secrets, draws)
    ds = _dev(secrets)
    for mode in MODES:
        want = exp if mode == PD.EXACT else np.mod(exp, p)
        for narrow in WIDTHS:
            got = _shares(_generate(engine, sch, ds, D, 1, mode, narrow, first=first)[0], sch, B, 1, narrow)[0]
            assert np.array_equal(got, want.astype(got.dtype)), (name, mode, narrow)
    other = _shares(_generate(engine, sch, ds, D, 1, PD.EXACT, False, first=first, stream_id=STREAM + 1)[0], sch, B, 1,
                    False)[0]
    assert not np.array_equal(other, exp)


# ---------------------------------------------------------------------------------------------------------------
# 5. staged path
# ---------------------------------------------------------------------------------------------------------------
STAGED = [  # (id, scheme, B, mode)
    ("n81-L8-exact", PM.scheme_for(3, 4, 80), 38, PD.EXACT),
    ("n81-L8-canon", PM.scheme_for(3, 4, 80), 38, PD.CANONICAL),
    ("n81-L16-exact-oddB-workspace", PM.scheme_for(8, 7, 80), 37, PD.EXACT),
    ("n81-L32-exact", PM.scheme_for(17, 14, 80), 38, PD.EXACT),
    ("L128-n243-workspace", PM.scheme_for(64, 63, 242), 37, PD.EXACT),
]


@pytest.mark.parametrize("name,sch,B,mode", STAGED, ids=[s[0] for s in STAGED])
def test_staged_path(engine, name, sch, B, mode):
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    assert ("workspace" in name) == (PD.gen_kernel(sch, B, 0, mode) == "wide")
    D = PM.dimension(B, k)
    secrets = np.random.default_rng(B + t).integers(-(p - 1), p, size=(V, D), dtype=np.int64)
    ds = _dev(secrets)
    for narrow in WIDTHS:
        for first in (0, KM.ODD_FIRST):
            want, wc = _generate(engine, sch, ds, D, V, mode, narrow, first, keyed=False)
            got, gc = _generate(engine, sch, ds, D, V, mode, narrow, first)
            assert engine.packed_keyed_last_launch() == (2, V * B * t * 8)
            _shares(want, sch, B, V, narrow)
            assert np.array_equal(got, want) and gc == wc, (name, narrow, first)


# ---------------------------------------------------------------------------------------------------------------
# 6. the status matrix of the header, in its order; a refused call leaves out and the record untouched
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", WIDTHS, ids=["i64", "int32"])
def test_status_matrix(engine, narrow):
    INV, PRE, UNS = E.ERR_INVALID_ARGUMENT, E.ERR_PRECONDITION, E.ERR_UNSUPPORTED
    sch = S.CONFIG_PACKED
    k, t, n = sch.secret_count, sch.privacy_threshold(), sch.share_count
    B = 6
    D = B * k
    ds = _dev(np.arange(D, dtype=np.int64))
    _generate(engine, sch, ds, D, 1, PD.EXACT, narrow)
    record = engine.packed_keyed_last_launch()
    assert record == (1, 0)
    call = engine.packed_generate_keyed32_dev if narrow else engine.packed_generate_keyed_dev
    even_p = S.PackedShamir(k, n, t, sch.prime_modulus + 1, sch.omega_secrets, sch.omega_shares)
    short = S.PackedShamir(k, 8, t, sch.prime_modulus, sch.omega_secrets, sch.omega_shares)   # n < k + t

    def refused(status, text, scheme=sch, nvec=1, mode=PD.EXACT, key=KEY, first=0, no_secrets=False, no_out=False,
                dim=D):
        buf, ptr = _out(n * B, narrow)
        with pytest.raises(SdaError) as ei:
            call(scheme, None if no_secrets else ds.data_ptr(), dim, nvec, key, STREAM, None if no_out else ptr, mode,
                 first_batch=first)
        torch.cuda.synchronize()
        assert ei.value.status == status and text in str(ei.value), str(ei.value)
        assert (buf == (SENT32 if narrow else SENT64)).all()
        assert engine.packed_keyed_last_launch() == record

    # 1. the scheme kind, ahead of the mode
    refused(INV, "PackedShamir", scheme=S.Additive(3, 433), mode=7)
    # 2. the mode, ahead of the scheme's domain
    refused(INV, "bad mode", scheme=even_p, mode=7)
    # 3. the scheme's domain, ahead of the vector limit
    refused(UNS, "prime_modulus", scheme=even_p, nvec=70000)
    refused(PRE, "share_count", scheme=short, nvec=70000)
    # 4. the vector limit, ahead of the buffers
    refused(UNS, "65535", nvec=70000, no_out=True)
    # 5. a NULL needed buffer, ahead of the key
    refused(INV, "NULL argument", no_out=True, key=None)
    refused(INV, "NULL argument", no_secrets=True, key=None)
    # 6. a NULL key, ahead of the wrap
    refused(INV, "NULL key", key=None, first=(1 << 64) - 1)
    # 7. (first_batch + n_vectors B) t wraps
    refused(INV, "wraps", first=(1 << 64) - B)
    refused(INV, "wraps", first=(1 << 64) // t)
    refused(INV, "wraps", first=1 << 63, nvec=3)
    # nothing to launch: OK without buffers, the record stays; t = 0 never wraps
    call(sch, None, 0, 1, KEY, STREAM, None, PD.EXACT)
    call(sch, None, D, 0, KEY, STREAM, None, PD.EXACT)
    assert engine.packed_keyed_last_launch() == record
    t0 = PM.scheme_for(7, 0, 8)
    buf, ptr = _out(8 * B, narrow)
    d0 = _dev(np.arange(7 * B))
    call(t0, d0.data_ptr(), 7 * B, 1, KEY, STREAM, ptr, PD.EXACT, first_batch=(1 << 64) - 1)
    torch.cuda.synchronize()
    assert engine.packed_keyed_last_launch() == (1, 0)
    # a NULL handle, and the record's own checks
    kk = (C.c_uint32 * 8)(*KEY)
    sc = sch.c()
    fn = engine.lib.sda_packed_generate_keyed32_dev if narrow else engine.lib.sda_packed_generate_keyed_dev
    assert fn(None, C.byref(sc), None, 0, 0, kk, 0, 0, None, 0, None) == INV
    assert engine.lib.sda_packed_keyed_last_launch(engine.h, None, None) == INV


def test_record_of_a_fresh_handle():
    e = Engine(0)
    try:
        assert e.packed_keyed_last_launch() == (0, 0)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. callers
# ---------------------------------------------------------------------------------------------------------------
D_PIPE = 4099
SEED = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]


def _participant(engine, ms, ss, secrets, full, keyed, narrow):
    d = secrets.numel()
    n, k, t = ss.share_count, ss.secret_count, ss.privacy_threshold()
    B = (d + k - 1) // k
    sh = torch.full((n, B), SENT32 if narrow else SENT64, dtype=torch.int32 if narrow else torch.int64, device="cuda")
    cap = n * B * 10 + 32
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    kw = dict(seed=SEED if isinstance(ms, S.ChaChaMasking) else None,
              full_masks_ptr=full.data_ptr() if full is not None else None, payload_ptr=pay.data_ptr(), payload_cap=cap)
    if keyed:
        call = engine.participant_share32_keyed_dev if narrow else engine.participant_share_keyed_dev
        rb = call(ms, ss, secrets.data_ptr(), d, KEY, STREAM, sh.data_ptr(), **kw)
    else:
        draws = torch.zeros(B * t + 2, dtype=torch.int64, device="cuda")
        engine.draws_dev(KEY, STREAM, 0, B * t, ss.prime_modulus - 1, draws.data_ptr())
        call = engine.participant_share32_dev if narrow else engine.participant_share_dev
        rb = call(ms, ss, secrets.data_ptr(), d, draws.data_ptr(), sh.data_ptr(), **kw)
    torch.cuda.synchronize()
    return sh.cpu().numpy(), rb.tolist(), pay.cpu().numpy()[:int(rb.sum())].tobytes()


@pytest.mark.parametrize("mask", ["none", "full", "chacha"])
def test_participant_pipelines_make_their_draws_in_the_share_kernel(engine, mask):
    ss = S.CONFIG_PACKED
    m = ss.prime_modulus
    ms = {"none": S.NoMasking(), "full": S.FullMasking(m), "chacha": S.ChaChaMasking(m, D_PIPE, 128)}[mask]
    secrets = _dev(np.random.default_rng(7).integers(0, m, size=D_PIPE, dtype=np.int64))[:D_PIPE]
    full = None
    if mask == "full":
        full = torch.zeros(D_PIPE, dtype=torch.int64, device="cuda")
        engine.draws_dev(KEY, STREAM + 1, 0, D_PIPE, m, full.data_ptr())
    # a staged launch first, so that the record below is the pipeline's own
    st_sch = PM.scheme_for(3, 4, 80)
    _generate(engine, st_sch, _dev(np.arange(12)), 12, 1, PD.EXACT, False)
    assert engine.packed_keyed_last_launch()[0] == 2
    for narrow in WIDTHS:
        want = _participant(engine, ms, ss, secrets, full, keyed=False, narrow=narrow)
        assert engine.packed_keyed_last_launch()[0] == 2          # the unkeyed pipeline leaves the record
        got = _participant(engine, ms, ss, secrets, full, keyed=True, narrow=narrow)
        assert engine.packed_keyed_last_launch() == (1, 0)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
        assert (want[0] != (SENT32 if narrow else SENT64)).all() and len(want[2]) > want[0].size
        _generate(engine, st_sch, _dev(np.arange(12)), 12, 1, PD.EXACT, False)


def test_share_generate_keyed_host_call(engine):
    sch = S.CONFIG_PACKED
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    D = 8 * 777 - 3
    B = (D + k - 1) // k
    secrets = np.random.default_rng(3).integers(0, p, size=D, dtype=np.int64)
    want = engine.share_generate(sch, secrets, engine.draws(KEY, STREAM, 0, B * t, p - 1))
    assert np.array_equal(engine.share_generate_keyed(sch, secrets, KEY, STREAM), want)
    assert engine.packed_keyed_last_launch() == (1, 0)
    multi = Engine(devices=[0, 0, 0])
    try:
        assert np.array_equal(multi.share_generate_keyed(sch, secrets, KEY, STREAM), want)
    finally:
        multi.close()
