"""GPU: int32 share rows through packed-Shamir share generation and reveal (sda_packed_generate32_dev,
sda_packed_reconstruct32_dev), bit for bit against the oracle and against the i64 entry points.

The cases are those of tests/test_gpu_packed_matrix.py (plan: tests/packed_matrix_cases.py, dispatch:
tests/packed_dispatch.py, input builders: that module's gen_inputs): ONE launch of V = 3 vectors of B = 550 / 549
batches with an odd dimension, raw i64 secrets planted in a few batches.  Added here: outputs 4 and 12 bytes off
a 16-byte boundary (int32 rows need only 4-byte alignment), and B = 548 -- the matrix's even B is no multiple of
4, so its int32 rows alternate between 16- and 8-byte alignment; at B = 548 every row is 16-byte aligned.

Every share is a `% p` result with p < 2^31, so narrowing the oracle's i64 shares is lossless; each test asserts
that on the oracle's array before it compares.  The fix-up counts are held between the number of planted batches
(the fast path really logs them) and 2 * planted + 16 (each planted batch takes its store-pair partner along;
16 is the lazily truncating kernels' trap allowance of the i64 matrix): a fast path that is bypassed in favour of
the fix-up fails although its output is right.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import packed_dispatch as PD
from tests import packed_matrix_cases as PM
from tests.test_gpu_packed_matrix import _O, _dev, _pp, _raw, _seed, gen_inputs, planted_reveal_batches
from tests.util import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = PM.V
SENT32 = 0x5A5A5A5A
SENT64 = 0x5A5A5A5A5A5A5A5A
GUARD = 4                                  # int32 words before the first 16-byte boundary of the output
B_QUAD = 548                               # B % 4 == 0, two full tiles and a ragged one at every workgroup size
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _gen_cases():
    """The matrix's rows, then per scheme: exact 4 bytes off, canonical 12 bytes off, and B = 548 in both modes
    (with SDA_GEN_SIGNBIT=0 too where the prime reaches the lazy kernels)."""
    cases = list(PM.GEN_CASES)
    seen = []
    for c in PM.GEN_CASES:
        if c.sch in seen:
            continue
        seen.append(c.sch)
        extra = [("exact-off4", PM.B_EVEN, 4, PD.EXACT, None), ("canon-off12", PM.B_EVEN, 12, PD.CANONICAL, None),
                 ("exact-B548", B_QUAD, 0, PD.EXACT, None), ("canon-B548", B_QUAD, 0, PD.CANONICAL, None)]
        if c.sch.prime_modulus >= PD.LAZY_TRUNC_MIN_P:
            extra.append(("exact-B548-signbit0", B_QUAD, 0, PD.EXACT, "0"))
        cases += [PM.GenCase(name, c.sch, B, off, mode, env, PD.gen_kernel(c.sch, B, off, mode, env))
                  for name, B, off, mode, env in extra]
    return cases


GEN32_CASES = _gen_cases()


def _narrow(exp, p):
    """The oracle's shares as int32, after checking that nothing is lost."""
    assert (np.abs(exp) < p).all() and p < (1 << 31)
    return exp.astype(np.int32)


def _out32(torch, words, offset):
    """(buffer, pointer, first word): int32 sentinel words, `offset` bytes past a 16-byte boundary, at least two
    guard words on each side."""
    buf = torch.full((GUARD + words + 8,), SENT32, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0 and offset % 4 == 0
    return buf, buf.data_ptr() + 4 * GUARD + offset, GUARD + offset // 4


def run_gen32_case(engine, case):
    import torch
    sch = case.sch
    p, n = sch.prime_modulus, sch.share_count
    secrets, draws, planted, exp = gen_inputs(sch, case.B)
    D = secrets.shape[1]
    ds, dd = _dev(torch, secrets), _dev(torch, draws)
    words = V * n * case.B
    buf, ptr, first = _out32(torch, words, case.out_offset)
    old = os.environ.pop("SDA_GEN_SIGNBIT", None)
    try:
        if case.signbit_env is not None:
            os.environ["SDA_GEN_SIGNBIT"] = case.signbit_env
        twin = PD.gen_kernel(sch, case.B, ptr % 16, case.mode, os.environ.get("SDA_GEN_SIGNBIT"))
        assert twin == case.kernel
        engine.packed_generate32_dev(sch, ds.data_ptr(), D, V, dd.data_ptr(), ptr, case.mode)
    finally:
        os.environ.pop("SDA_GEN_SIGNBIT", None)
        if old is not None:
            os.environ["SDA_GEN_SIGNBIT"] = old
    count = engine.packed_fixup_count()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    want = _narrow(exp if case.mode == PD.EXACT else np.mod(exp, p), p)
    assert_same(host[first:first + words].reshape(V, n, case.B), want, case.id)
    assert (host[:first] == SENT32).all() and (host[first + words:] == SENT32).all(), "wrote outside the output"
    print(f"MATRIX32 {case.id} twin {twin} fixups {count} planted {len(planted)}")
    assert count <= 2 * len(planted) + 16, (case.id, count)
    if twin != "wide":
        assert count >= len(planted), (case.id, count)
    return count


@pytest.mark.parametrize("case", GEN32_CASES, ids=lambda c: c.id)
def test_share_gen32_case(engine, case):
    run_gen32_case(engine, case)


# ---------------------------------------------------------------------------------------------- reveal
@functools.lru_cache(maxsize=None)
def reveal32_inputs(case):
    """(indices, shares int32 [V][n_idx][B], D, planted, oracle secrets [V][D]) -- tests/test_gpu_packed_matrix's
    reveal_inputs with plants that fit int32, at the same (vec, b) positions: INT32_MIN / INT32_MAX for
    p > 2^30 (both lie outside (-p, p) for every p < 2^31), share +- c p with 1 <= c <= 64 for p < 2^24."""
    O = _O()
    sch, B = case.sch, case.B
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    assert p > (1 << 30) or p < (1 << 24)
    rng = np.random.default_rng(_seed(sch, B, case.n_idx, case.mode, 32))
    D = PM.dimension(B, k)
    pp = _pp(O, sch)
    idx = rng.permutation(n)[:case.n_idx]
    planted = planted_reveal_batches(B)
    shares, exp = [], []
    for v in range(V):
        secrets = rng.integers(0, p, size=D, dtype=np.int64)
        draws = rng.integers(0, p - 1, size=B * t, dtype=np.int64)
        sh = np.ascontiguousarray(O.packed_generate(pp, secrets, draws)[idx])
        assert (np.abs(sh) < p).all()
        for pv, b in sorted(planted):
            if pv == v:
                row = int(rng.integers(0, case.n_idx))
                if p > (1 << 30):
                    sh[row, b] = I32_MAX if b % 2 else I32_MIN
                else:
                    sh[row, b] += int(rng.integers(1, 65)) * p * (1 if b % 2 else -1)
                assert not -p < sh[row, b] < p and I32_MIN <= sh[row, b] <= I32_MAX
        rc, e = O.packed_reconstruct(pp, D, idx, sh)              # over the widened shares
        assert rc == 0
        shares.append(sh.astype(np.int32))
        exp.append(e)
    shares, exp = np.stack(shares), np.stack(exp)
    shares.setflags(write=False)
    exp.setflags(write=False)
    return idx, shares, D, planted, exp


def run_reveal32_case(engine, case):
    import torch
    sch = case.sch
    p, k = sch.prime_modulus, sch.secret_count
    idx, shares, D, planted, exp = reveal32_inputs(case)
    assert PD.reveal_kernel(sch, case.n_idx, k, case.mode) == case.kernel
    dsh = _dev(torch, shares, pad=4)
    buf = torch.full((V * D + 2,), SENT64, dtype=torch.int64, device="cuda")
    engine.packed_reconstruct32_dev(sch, D, idx.tolist(), V, dsh.data_ptr(), buf.data_ptr(), mode=case.mode)
    count = engine.packed_fixup_count()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert_same(host[:V * D].reshape(V, D), exp if case.mode == PD.EXACT else np.mod(exp, p), case.id)
    assert (host[V * D:] == SENT64).all(), "wrote outside the output"
    print(f"MATRIX32 {case.id} kernel {case.kernel} fixups {count} planted {len(planted)}")
    if case.mode == PD.EXACT and case.kernel != "wide":
        assert len(planted) <= count <= len(planted) + 16, (case.id, count)
    return count


@pytest.mark.parametrize("case", PM.REVEAL_CASES, ids=lambda c: c.id)
def test_reveal32_case(engine, case):
    run_reveal32_case(engine, case)


# ---------------------------------------------------------------------------------------------- twin equality
TWIN_SCHEMES = {
    "configs2": S.CONFIG_PACKED,                          # k = 8, t = 7, n = 26: the benchmarked scheme
    "n81": PM.scheme_for(8, 7, 80),                       # the i64 register kernels + the narrowing pass
    "workspace": PM.scheme_for(64, 63, 242),              # L = 128 > 64: packed_wide.hip
}


@pytest.mark.parametrize("mode", [PD.EXACT, PD.CANONICAL], ids=["exact", "canon"])
@pytest.mark.parametrize("family", list(TWIN_SCHEMES))
def test_twin_equality(engine, family, mode):
    """generate32 == (int32) of the i64 entry point's output; reconstruct32 == the i64 reveal of the widened
    shares -- at B = 1, 2, 3 and around one tile."""
    import torch
    sch = TWIN_SCHEMES[family]
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    want = {"configs2": "packed_gen_kernel<16, 27,", "n81": "packed_gen_kernel<16, 81,", "workspace": "wide"}[family]
    assert PD.gen_kernel(sch, 256, 0, mode).startswith(want)
    idx = list(range(n - (k + t), n))                     # the last t + k clerks
    for B in (1, 2, 3, 255, 256, 257):
        rng = np.random.default_rng(_seed(sch, B, mode, 99))
        D = PM.dimension(B, k)
        secrets = rng.integers(-(p - 1), p, size=(V, D), dtype=np.int64)
        secrets[1, 0] = _raw(rng, 1)[0]
        draws = rng.integers(0, p - 1, size=(V, B, t), dtype=np.int64)
        ds, dd = _dev(torch, secrets), _dev(torch, draws)
        words = V * n * B
        o64 = torch.full((words + 2,), SENT64, dtype=torch.int64, device="cuda")
        engine.packed_generate_mode_dev(sch, ds.data_ptr(), D, V, dd.data_ptr(), o64.data_ptr(), mode)
        o32, ptr, first = _out32(torch, words, 0)
        engine.packed_generate32_dev(sch, ds.data_ptr(), D, V, dd.data_ptr(), ptr, mode)
        torch.cuda.synchronize()
        h64, h32 = o64.cpu().numpy(), o32.cpu().numpy()
        assert (np.abs(h64[:words]) < p).all()
        assert_same(h32[first:first + words], h64[:words].astype(np.int32), f"{family} gen B={B}")
        assert (h32[:first] == SENT32).all() and (h32[first + words:] == SENT32).all()
        # reveal from t + k clerks: rows idx of every vector, dense
        sh32 = np.ascontiguousarray(h32[first:first + words].reshape(V, n, B)[:, idx, :])
        r64 = torch.full((V * D + 2,), SENT64, dtype=torch.int64, device="cuda")
        r32 = torch.full((V * D + 2,), SENT64, dtype=torch.int64, device="cuda")
        d64, d32 = _dev(torch, sh32.astype(np.int64)), _dev(torch, sh32, pad=4)
        engine.packed_reconstruct_dev(sch, D, idx, V, d64.data_ptr(), r64.data_ptr(), mode=mode)
        engine.packed_reconstruct32_dev(sch, D, idx, V, d32.data_ptr(), r32.data_ptr(), mode=mode)
        torch.cuda.synchronize()
        assert_same(r32.cpu().numpy(), r64.cpu().numpy(), f"{family} reveal B={B}")
        if mode == PD.CANONICAL:                          # and the round trip: canonical secrets back
            got = r32.cpu().numpy()[:V * D].reshape(V, D)
            ok = np.ones((V, D), bool)
            ok[1, :k] = False                             # the batch of the raw secret
            assert_same(got[ok], np.mod(secrets, p)[ok], f"{family} round trip B={B}")


# ---------------------------------------------------------------------------------------------- the int32 chain
def test_int32_chain_generate_combine_reveal(engine):
    """P = 5 participants' shares in one generate32 launch, each clerk's combine32 over the strided view of that
    buffer, the n clerk results narrowed, reveal32 from t + k = 15 clerks and from all 26: equal to the oracle's
    generate -> combine -> reconstruct and to the all-i64 device chain."""
    import torch
    O = _O()
    sch = S.CONFIG_PACKED
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    P, B = 5, PM.B_ODD
    D = PM.dimension(B, k)
    rng = np.random.default_rng(_seed(sch, B, P))
    secrets = rng.integers(0, p, size=(P, D), dtype=np.int64)
    draws = rng.integers(0, p - 1, size=(P, B, t), dtype=np.int64)
    pp = _pp(O, sch)
    oshares = np.stack([O.packed_generate(pp, secrets[i], draws[i].reshape(-1)) for i in range(P)])   # [P][n][B]
    oclerk = np.stack([O.combine(p, np.ascontiguousarray(oshares[:, c, :])) for c in range(n)])       # [n][B]
    ds, dd = _dev(torch, secrets), _dev(torch, draws)
    sh32 = torch.full((P * n * B + 4,), SENT32, dtype=torch.int32, device="cuda")
    sh64 = torch.full((P * n * B + 2,), SENT64, dtype=torch.int64, device="cuda")
    engine.packed_generate32_dev(sch, ds.data_ptr(), D, P, dd.data_ptr(), sh32.data_ptr(), PD.EXACT)
    engine.packed_generate_mode_dev(sch, ds.data_ptr(), D, P, dd.data_ptr(), sh64.data_ptr(), PD.EXACT)
    ck32 = torch.zeros((n * B,), dtype=torch.int64, device="cuda")      # clerk results of the int32 chain (i64)
    ck64 = torch.zeros((n * B,), dtype=torch.int64, device="cuda")
    for c in range(n):
        engine.combine32_dev(p, sh32.data_ptr() + 4 * c * B, P, B, n * B, ck32.data_ptr() + 8 * c * B)
        engine.combine_dev(p, sh64.data_ptr() + 8 * c * B, P, B, n * B, ck64.data_ptr() + 8 * c * B)
    nar = torch.full((n * B + 4,), SENT32, dtype=torch.int32, device="cuda")
    flag = torch.zeros((1,), dtype=torch.int64, device="cuda")
    engine.narrow32_dev(ck32.data_ptr(), n, B, B, nar.data_ptr(), B, flag.data_ptr())
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert_same(sh32.cpu().numpy()[:P * n * B].reshape(P, n, B), _narrow(oshares, p), "generate32")
    assert_same(ck32.cpu().numpy().reshape(n, B), oclerk, "combine32")
    assert_same(ck64.cpu().numpy().reshape(n, B), oclerk, "combine i64")
    for n_idx in (k + t, n):
        idx = list(range(n_idx))
        rc, exp = O.packed_reconstruct(pp, D, idx, np.ascontiguousarray(oclerk[:n_idx]))
        assert rc == 0
        o32 = torch.full((D + 2,), SENT64, dtype=torch.int64, device="cuda")
        o64 = torch.full((D + 2,), SENT64, dtype=torch.int64, device="cuda")
        engine.packed_reconstruct32_dev(sch, D, idx, 1, nar.data_ptr(), o32.data_ptr())
        engine.packed_reconstruct_dev(sch, D, idx, 1, ck64.data_ptr(), o64.data_ptr())
        torch.cuda.synchronize()
        assert_same(o32.cpu().numpy()[:D], exp, f"chain from {n_idx}")
        assert_same(o32.cpu().numpy(), o64.cpu().numpy(), f"chain vs i64 from {n_idx}")
        assert_same(np.mod(exp, p), np.mod(secrets.sum(axis=0), p), f"the sum of the secrets from {n_idx}")


# ---------------------------------------------------------------------------------------------- contract
def _small(torch, sch, B, seed):
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    rng = np.random.default_rng(seed)
    D = B * k
    secrets = rng.integers(0, p, size=(1, D), dtype=np.int64)
    draws = rng.integers(0, p - 1, size=(1, B, t), dtype=np.int64)
    return D, secrets, draws, _dev(torch, secrets), _dev(torch, draws)


def test_contract_empty_and_errors(engine):
    import torch
    sch = S.CONFIG_PACKED
    k, t, n = sch.secret_count, sch.privacy_threshold(), sch.share_count
    B = 8
    D, _, _, ds, dd = _small(torch, sch, B, 5)
    out = torch.full((n * B + 4,), SENT32, dtype=torch.int32, device="cuda")
    o64 = torch.full((n * B + 4,), SENT64, dtype=torch.int64, device="cuda")
    # nothing to do: as the twins, no error and nothing written
    for dim, nv in ((D, 0), (0, 1), (0, 0)):
        engine.packed_generate_mode_dev(sch, ds.data_ptr(), dim, nv, dd.data_ptr(), o64.data_ptr(), PD.EXACT)
        engine.packed_generate32_dev(sch, ds.data_ptr(), dim, nv, dd.data_ptr(), out.data_ptr(), PD.EXACT)
        engine.packed_reconstruct_dev(sch, dim, list(range(k + t)), nv, o64.data_ptr(), o64.data_ptr())
        engine.packed_reconstruct32_dev(sch, dim, list(range(k + t)), nv, out.data_ptr(), o64.data_ptr())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT32).all() and (o64.cpu().numpy() == SENT64).all()
    with pytest.raises(E.SdaError) as ei:
        engine.packed_generate32_dev(sch, ds.data_ptr(), D, 1, dd.data_ptr(), None, PD.EXACT)
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    with pytest.raises(E.SdaError) as ei:
        engine.packed_reconstruct32_dev(sch, D, list(range(k + t)), 1, out.data_ptr(), None)
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    with pytest.raises(E.SdaError) as ei:
        engine.packed_generate32_dev(sch, ds.data_ptr(), D, 1, dd.data_ptr(), out.data_ptr(), 7)
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    with pytest.raises(E.SdaError) as ei:
        engine.packed_generate32_dev(sch, ds.data_ptr(), D, 65536, dd.data_ptr(), out.data_ptr(), PD.EXACT)
    assert ei.value.status == E.ERR_UNSUPPORTED
    with pytest.raises(E.SdaError) as ei:
        engine.packed_reconstruct32_dev(sch, D, list(range(k + t)), 65536, out.data_ptr(), o64.data_ptr())
    assert ei.value.status == E.ERR_UNSUPPORTED
    with pytest.raises(E.SdaError) as ei:
        engine.packed_reconstruct32_dev(sch, D, list(range(k + t - 1)), 1, out.data_ptr(), o64.data_ptr())
    assert ei.value.status == E.ERR_NOT_ENOUGH_SHARES
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT32).all() and (o64.cpu().numpy() == SENT64).all()


def test_contract_second_stream_follows_the_first(engine):
    """generate32 on one stream, reveal32 of its output on another, no host wait in between: the handle orders
    the second call after the first."""
    import torch
    sch = S.CONFIG_PACKED
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    B = 4096
    D, secrets, _, ds, dd = _small(torch, sch, B, 6)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    sh = torch.full((n * B + 4,), SENT32, dtype=torch.int32, device="cuda")
    out = torch.full((D + 2,), SENT64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    engine.packed_generate32_dev(sch, ds.data_ptr(), D, 1, dd.data_ptr(), sh.data_ptr(), PD.CANONICAL,
                                 stream=s1.cuda_stream)
    engine.packed_reconstruct32_dev(sch, D, list(range(k + t)), 1, sh.data_ptr(), out.data_ptr(),
                                    mode=PD.CANONICAL, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert_same(host[:D], secrets[0])
    assert (host[D:] == SENT64).all()


def run_xcd_rows32():
    """One share-gen and one reveal row whose kernels read SDA_XCD_ORDER, in a fresh process with the knob at 0."""
    import torch
    from sda_amd import Engine
    assert os.environ.get("SDA_XCD_ORDER") == "0"
    torch.cuda.init()
    engine = Engine(0)
    try:
        run_gen32_case(engine, _xcd_gen_case())
        run_reveal32_case(engine, _xcd_reveal_case())
        print("XCD_ROWS32_OK")
    finally:
        engine.close()


def _xcd_gen_case():
    return next(c for c in PM.xcd_gen_cases() if c.kernel.startswith("packed_gen_kernel<16, 27, true, false, true, true"))


def _xcd_reveal_case():
    return next(c for c in PM.xcd_reveal_cases() if c.kernel.startswith("packed_reveal_exact_kernel<16, true, 8, true, true"))


def test_contract_xcd_order_off(engine):
    """SDA_XCD_ORDER=0 (natural workgroup order): the same output for one share-gen and one reveal case."""
    run_gen32_case(engine, _xcd_gen_case())
    run_reveal32_case(engine, _xcd_reveal_case())
    env = dict(os.environ, SDA_XCD_ORDER="0")
    env.pop("SDA_GEN_SIGNBIT", None)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_packed32 import run_xcd_rows32; run_xcd_rows32()"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "XCD_ROWS32_OK" in r.stdout
