"""GPU: every shipped packed-Shamir kernel variant at multi-tile, multi-vector shapes, bit for bit against
the oracle, with the number of batches each launch handed to its fix-up kernel (sda_packed_fixup_count).

The plan is tests/packed_matrix_cases.py (built on the CPU; tests/test_packed_matrix_plan.py holds it against
the instantiations in the library).  Each share-gen / reveal case is ONE launch of V = 3 vectors of B = 550 or
549 batches with an odd dimension D = B k - r:
  * two or more full tiles and a ragged last one at every workgroup size, blockIdx.y > 0, a grid whose size is
    no multiple of 8 (xcd_block_xy's remainder path);
  * vectors 0 and 2 start 16-byte aligned, vector 1 8 bytes off: share-gen's full tiles take the LDS-DMA
    stage in vectors 0 and 2 (L <= 16, n + 1 < 81 or 5 waves) and the register full-tile stage in vector 1, the
    last tile the bounds-checked stage with a zero-padded tail batch; the reveal's flush takes its 16-byte
    stores and its 8-byte stores, and odd store counts;
  * a few batches per vector carry raw i64 inputs outside (-p, p), placed at the first batch of a full tile, at
    batch B - 1 (not in every vector: the fix-up rewrites what it recomputes, which would hide the fast path's
    tail), in a batch whose store-pair partner stays in range, and in both batches of a pair.
Every output word is compared (a sentinel is written first), then the fix-up count: equal to the count
tests/packed_dispatch.py predicts from the planted batches, plus at most LAZY_ALLOWANCE for the lazily
truncating kernels (a trap rate of about 2 big / p per multiplied operand, big <= 4096,
p ~ 2^31, <= 250 operands per batch: ~1e-3 per batch, ~2 over the 1,650 batches; 16 is 1 % of the launch).  So
a fast path that is bypassed (everything recomputed by the fix-up) fails even though its output is right.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import packed_dispatch as PD
from tests import packed_matrix_cases as PM
from tests.util import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = PM.V
SENTINEL = 0x5A5A5A5A5A5A5A5A          # no share or secret of a prime below 2^31 looks like this
LAZY_ALLOWANCE = 16


def _O():
    from oracle import oracle as O
    O.lib()
    return O


def _pp(O, sch):
    return O.packed_params(sch.secret_count, sch.share_count, sch.privacy_threshold(), sch.prime_modulus,
                           sch.omega_secrets, sch.omega_shares)


def _seed(sch, *more):
    return [sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count, *more]


def _raw(rng, size):
    """raw i64 values far outside any field: 2^33 <= |v| < 2^40"""
    return rng.integers(1 << 33, 1 << 40, size=size, dtype=np.int64) * rng.choice(np.array([-1, 1]), size=size)


def planted_gen_batches(B):
    """{(vec, b)}: the first batch of a full tile (256 starts one at every workgroup size), batch B - 1, one
    batch whose pair partner stays in range, and one whole pair -- shifted per vector.  Vector 2 keeps its
    batch B - 1 in range: the fix-up kernel rewrites whatever it recomputes, so a plant there in every vector
    would hide the fast path's zero-padded tail batch."""
    out = set()
    for v in range(V):
        out |= {(v, 256), (v, 10 + 2 * v), (v, 300 + 2 * v), (v, 301 + 2 * v)}
        if v < 2:
            out.add((v, B - 1))
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def gen_inputs(sch, B):
    """(secrets [V][D], draws [V][B][t], planted, oracle shares [V][n][B]) -- computed once per (scheme, B) and
    shared by the variants; never modified."""
    O = _O()
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    rng = np.random.default_rng(_seed(sch, B))
    D = PM.dimension(B, k)
    secrets = rng.integers(-(p - 1), p, size=(V, D), dtype=np.int64)
    draws = rng.integers(0, p - 1, size=(V, B, t), dtype=np.int64)
    planted = planted_gen_batches(B)
    for v, b in sorted(planted):
        secrets[v, b * k] = _raw(rng, 1)[0]
    exp = np.stack([O.packed_generate(_pp(O, sch), secrets[v], draws[v].reshape(-1)) for v in range(V)])
    for a in (secrets, draws, exp):
        a.setflags(write=False)
    return secrets, draws, planted, exp


def _dev(torch, a, pad=2):
    """a on the device, 16-byte aligned, never empty"""
    flat = np.concatenate([np.ascontiguousarray(a).reshape(-1), np.zeros(pad, a.dtype)])
    d = torch.as_tensor(flat).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def _check_count(kernel, lazy, count, want):
    print(f"MATRIX {kernel} fixups {count} planted {want}")
    if lazy:
        assert want <= count <= want + LAZY_ALLOWANCE, (kernel, count, want)
    else:
        assert count == want, (kernel, count, want)


def run_gen_case(engine, case):
    import torch
    sch = case.sch
    p, k, n = sch.prime_modulus, sch.secret_count, sch.share_count
    secrets, draws, planted, exp = gen_inputs(sch, case.B)
    D = secrets.shape[1]
    ds, dd = _dev(torch, secrets), _dev(torch, draws)
    words, off = V * n * case.B, case.out_offset // 8
    buf = torch.full((words + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    ptr = buf.data_ptr() + case.out_offset
    assert buf.data_ptr() % 16 == 0
    old = os.environ.pop("SDA_GEN_SIGNBIT", None)
    try:
        if case.signbit_env is not None:
            os.environ["SDA_GEN_SIGNBIT"] = case.signbit_env
        assert PD.gen_kernel(sch, case.B, ptr % 16, case.mode, os.environ.get("SDA_GEN_SIGNBIT")) == case.kernel
        engine.packed_generate_mode_dev(sch, ds.data_ptr(), D, V, dd.data_ptr(), ptr, case.mode)
    finally:
        os.environ.pop("SDA_GEN_SIGNBIT", None)
        if old is not None:
            os.environ["SDA_GEN_SIGNBIT"] = old
    count = engine.packed_fixup_count()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    want = exp if case.mode == PD.EXACT else np.mod(exp, p)
    assert_same(host[off:off + words].reshape(V, n, case.B), want, case.id)
    assert (host[:off] == SENTINEL).all() and (host[off + words:] == SENTINEL).all(), "wrote outside the output"
    _check_count(case.kernel, PD.gen_kernel_is_lazy(case.kernel), count,
                 PD.gen_fixup_count(case.kernel, planted, case.B))
    return count


@pytest.mark.parametrize("case", PM.GEN_CASES, ids=lambda c: c.id)
def test_share_gen_case(engine, case):
    run_gen_case(engine, case)


def planted_reveal_batches(B):
    """{(vec, b)} with raw shares: batch B - 1 only in vector 1 (the 8-byte flush); vectors 0 and 2 leave their
    tail -- the 16-byte flush's odd last word -- to the fast path (the fix-up rewrites what it recomputes)."""
    out = {(1, B - 1)}
    for v in range(V):
        out |= {(v, v), (v, 255), (v, 256 + 3 * v)}
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def reveal_inputs(case):
    """(indices, shares [V][n_idx][B], D, planted, oracle secrets [V][D]) of one reveal case."""
    O = _O()
    sch, B = case.sch, case.B
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    rng = np.random.default_rng(_seed(sch, B, case.n_idx, case.mode))
    D = PM.dimension(B, k)
    pp = _pp(O, sch)
    idx = rng.permutation(n)[:case.n_idx]                 # random order
    planted = planted_reveal_batches(B)
    shares, exp = [], []
    for v in range(V):
        secrets = rng.integers(0, p, size=D, dtype=np.int64)
        draws = rng.integers(0, p - 1, size=B * t, dtype=np.int64)
        sh = np.ascontiguousarray(O.packed_generate(pp, secrets, draws)[idx])
        for pv, b in sorted(planted):
            if pv == v:
                sh[int(rng.integers(0, case.n_idx)), b] += int(rng.integers(2, 1 << 20)) * p * (1 if b % 2 else -1)
        rc, e = O.packed_reconstruct(pp, D, idx, sh)
        assert rc == 0
        shares.append(sh)
        exp.append(e)
    shares, exp = np.stack(shares), np.stack(exp)
    shares.setflags(write=False)
    exp.setflags(write=False)
    return idx, shares, D, planted, exp


def run_reveal_case(engine, case):
    import torch
    sch = case.sch
    p, k = sch.prime_modulus, sch.secret_count
    idx, shares, D, planted, exp = reveal_inputs(case)
    assert D % 2 == 1 and (k == 1 or D % k)
    assert PD.reveal_kernel(sch, case.n_idx, k, case.mode) == case.kernel
    dsh = _dev(torch, shares)
    buf = torch.full((V * D + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    engine.packed_reconstruct_dev(sch, D, idx.tolist(), V, dsh.data_ptr(), buf.data_ptr(), mode=case.mode)
    count = engine.packed_fixup_count()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert_same(host[:V * D].reshape(V, D), exp if case.mode == PD.EXACT else np.mod(exp, p), case.id)
    assert (host[V * D:] == SENTINEL).all(), "wrote outside the output"
    _check_count(case.kernel, PD.reveal_kernel_is_lazy(case.kernel), count,
                 PD.reveal_fixup_count(case.kernel, planted))
    return count


@pytest.mark.parametrize("case", PM.REVEAL_CASES, ids=lambda c: c.id)
def test_reveal_case(engine, case):
    run_reveal_case(engine, case)


# ---------------------------------------------------------------------------------------------- workspace kernels
# packed_wide.hip walks the batches with a fixed grid of lanes, `for (gb = gid; gb < total; gb += lanes)`, each lane
# reusing its workspace columns: these cases make total > wide_lanes(total, words), so some lanes take a second batch.
def _tiled(unique, B, shift):
    """[V][B] indices into `unique` distinct batches: vector v holds batch (b + v shift) % unique at b.  The
    period is prime, so a lane's second batch differs from its first whatever the lane count."""
    return (np.arange(B)[None, :] + shift * np.arange(V)[:, None]) % unique


def test_workspace_gen_register_exclusion_second_pass(engine):
    """L = 64 over 81 points with p < 2^24, exact: the register kernels' exclusion (gen_register_path), V B just
    past the 65,536-lane cap, odd B, ragged D, all batches distinct."""
    import torch
    O = _O()
    sch = PM.scheme_for(33, 30, 80, 1 << 24)
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    B = 21847
    lanes = PD.wide_lanes(V * B, k + t + 1 + n + 1)
    assert B % 2 == 1 and V * B > 65536 == lanes and PD.gen_kernel(sch, B, 0, PD.EXACT) == "wide"
    rng = np.random.default_rng(_seed(sch, B))
    D = PM.dimension(B, k)
    secrets = rng.integers(-(p - 1), p, size=(V, D), dtype=np.int64)
    secrets[:, ::997] = _raw(rng, secrets[:, ::997].shape)
    draws = rng.integers(0, p - 1, size=(V, B, t), dtype=np.int64)
    exp = np.stack([O.packed_generate(_pp(O, sch), secrets[v], draws[v].reshape(-1)) for v in range(V)])
    ds, dd = _dev(torch, secrets), _dev(torch, draws)
    buf = torch.full((V * n * B + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    engine.packed_generate_mode_dev(sch, ds.data_ptr(), D, V, dd.data_ptr(), buf.data_ptr(), PD.EXACT)
    assert engine.packed_fixup_count() == 0
    host = buf.cpu().numpy()
    assert_same(host[:-2].reshape(V, n, B), exp)
    assert (host[-2:] == SENTINEL).all()


def test_workspace_gen_243_points_second_pass(engine):
    """L = 128 over 243 points (the widest transform below 243 points), V B just past its lane cap, exact and
    canonical.  4,999 distinct batches tiled over the launch keep the oracle's side short."""
    import torch
    O = _O()
    sch = PM.scheme_for(64, 63, 242)
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    cap = PD.wide_lanes(1 << 40, k + t + 1 + n + 1)
    B = cap // V + 1
    assert V * B > cap == PD.wide_lanes(V * B, k + t + 1 + n + 1) and V * B - cap < V
    U = 4999
    rng = np.random.default_rng(_seed(sch, B))
    us = rng.integers(-(p - 1), p, size=(U, k), dtype=np.int64)
    us[::7, 3] = _raw(rng, us[::7, 3].shape)
    ud = rng.integers(0, p - 1, size=(U, t), dtype=np.int64)
    uexp = O.packed_generate(_pp(O, sch), us.reshape(-1), ud.reshape(-1))          # [n][U]
    sel = _tiled(U, B, 1667)
    ds, dd = _dev(torch, us[sel]), _dev(torch, ud[sel])
    exp = np.stack([uexp[:, sel[v]] for v in range(V)])
    for mode in (PD.EXACT, PD.CANONICAL):
        buf = torch.full((V * n * B + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        engine.packed_generate_mode_dev(sch, ds.data_ptr(), B * k, V, dd.data_ptr(), buf.data_ptr(), mode)
        assert engine.packed_fixup_count() == 0
        host = buf.cpu().numpy()
        assert_same(host[:-2].reshape(V, n, B), exp if mode == PD.EXACT else np.mod(exp, p))
        assert (host[-2:] == SENTINEL).all()
        del buf


def test_workspace_reveal_second_pass(engine):
    """The wide reveal (96 shares: one past the register kernels) with V B just past its lane cap.  1,999
    distinct batches (the oracle inverts per Newton step: ~1 ms a batch), tiled with a prime period."""
    import torch
    O = _O()
    sch = PM.scheme_for(5, 2, 242)
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    n_idx = 96
    cap = PD.wide_lanes(1 << 40, n_idx + 1)
    B = cap // V + 1
    assert V * B > cap == PD.wide_lanes(V * B, n_idx + 1) and PD.reveal_kernel(sch, n_idx, k, PD.EXACT) == "wide"
    U = 1999
    rng = np.random.default_rng(_seed(sch, B, n_idx))
    pp = _pp(O, sch)
    idx = rng.permutation(n)[:n_idx]
    ush = np.ascontiguousarray(O.packed_generate(pp, rng.integers(0, p, size=U * k, dtype=np.int64),
                                                 rng.integers(0, p - 1, size=U * t, dtype=np.int64))[idx])
    ush[5, ::11] += 3 * p                                   # raw shares: any i64 goes
    rc, uexp = O.packed_reconstruct(pp, U * k, idx, ush)
    assert rc == 0
    sel = _tiled(U, B, 667)
    dsh = _dev(torch, np.stack([ush[:, sel[v]] for v in range(V)]))
    exp = np.stack([uexp.reshape(U, k)[sel[v]].reshape(-1) for v in range(V)])
    for mode in (PD.EXACT, PD.CANONICAL):
        buf = torch.full((V * B * k + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        engine.packed_reconstruct_dev(sch, B * k, idx.tolist(), V, dsh.data_ptr(), buf.data_ptr(), mode=mode)
        assert engine.packed_fixup_count() == 0
        host = buf.cpu().numpy()
        assert_same(host[:-2].reshape(V, B * k), exp if mode == PD.EXACT else np.mod(exp, p))
        assert (host[-2:] == SENTINEL).all()


@pytest.mark.parametrize("width", [64, 32], ids=["i64", "int32"])
def test_cached_table_keeps_the_duplicate_refusal(engine, width):
    """A CANONICAL reveal of repeated clerk indices is refused even when an EXACT reveal of the same indices has
    just built and cached the table it would use -- from 40 shares (the detour shares the EXACT call's table, and
    takes the verdict kept with it) and from 7 (the Lagrange kernels' own table).  The refused call launches
    nothing, and the CANONICAL reveal of distinct indices that follows is the oracle's."""
    import torch
    from sda_amd import engine as E
    O = _O()
    sch = PM.scheme_for(3, 4, 80)                           # n + 1 = 81, k + t + 1 = 8
    p, k, n = sch.prime_modulus, sch.secret_count, sch.share_count
    D, nv = 8, 2                                            # B = 3 with a padded tail batch
    B = (D + k - 1) // k
    assert B == 3 and D % k
    rng = np.random.default_rng(_seed(sch, D, width))
    reveal = engine.packed_reconstruct_dev if width == 64 else engine.packed_reconstruct32_dev
    for n_idx in (40, 7):
        assert PD.reveal_takes_detour(n_idx, k, PD.CANONICAL) == (n_idx == 40)
        idx = rng.permutation(n)[:n_idx]
        dup = idx.copy()
        dup[n_idx - 2] = dup[1]
        shares = rng.integers(-(p - 1), p, size=(nv, n_idx, B), dtype=np.int64)
        dsh = _dev(torch, shares if width == 64 else shares.astype(np.int32))
        buf = torch.full((nv * D + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        reveal(sch, D, dup.tolist(), nv, dsh.data_ptr(), buf.data_ptr(), mode=PD.EXACT)        # SDA_OK
        buf.fill_(SENTINEL)
        with pytest.raises(E.SdaError) as err:
            reveal(sch, D, dup.tolist(), nv, dsh.data_ptr(), buf.data_ptr(), mode=PD.CANONICAL)
        assert err.value.status == E.ERR_UNSUPPORTED
        assert "canonical reveal needs distinct clerk indices" in str(err.value)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all(), "the refused call wrote"
        reveal(sch, D, idx.tolist(), nv, dsh.data_ptr(), buf.data_ptr(), mode=PD.CANONICAL)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        for v in range(nv):
            rc, exp = O.packed_reconstruct(_pp(O, sch), D, idx, shares[v])
            assert rc == 0
            assert_same(host[v * D:(v + 1) * D], np.mod(exp, p), f"from {n_idx}, vector {v}")
        assert (host[nv * D:] == SENTINEL).all(), "wrote outside the output"


def test_fixup_count_before_any_packed_launch():
    """A fresh handle reports 0."""
    from sda_amd import Engine
    e = Engine(0)
    try:
        assert e.packed_fixup_count() == 0
    finally:
        e.close()


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi1"])
def test_fixup_count_follows_the_host_entry_points(multi):
    """The host entry points launch on the handle's own stream (a multi-device handle: on each device's
    sub-handle, whose counts are summed): one raw secret logs its batch and the pair partner; the reveal at
    the threshold that follows logs nothing."""
    from sda_amd import Engine, schemes as S
    O = _O()
    sch = S.CONFIG_PACKED
    p, k, t = sch.prime_modulus, sch.secret_count, sch.privacy_threshold()
    rng = np.random.default_rng(77)
    B = 40
    secrets = rng.integers(-(p - 1), p, size=B * k, dtype=np.int64)
    secrets[5 * k + 2] = 1 << 45
    draws = rng.integers(0, p - 1, size=B * t, dtype=np.int64)
    e = Engine(0, devices=[0]) if multi else Engine(0)
    try:
        shares = e.share_generate(sch, secrets, draws)
        assert_same(shares, O.packed_generate(_pp(O, sch), secrets, draws))
        assert e.packed_fixup_count() == 2
        idx = list(range(3, 3 + k + t))
        got = e.secret_reconstruct(sch, B * k, [(i, shares[i]) for i in idx])
        rc, exp = O.packed_reconstruct(_pp(O, sch), B * k, idx, shares[idx])
        assert rc == 0
        assert_same(got, exp)
        assert e.packed_fixup_count() == 0
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- SDA_XCD_ORDER=0
def run_xcd_rows():
    """The rows whose kernels take the XCD-chunked tile order (share-gen L <= 16, reveals of up to 16 points).
    Run by test_xcd_order_off in a fresh process with SDA_XCD_ORDER=0 (the knob is read once per process)."""
    import torch
    from sda_amd import Engine
    assert os.environ.get("SDA_XCD_ORDER") == "0"
    torch.cuda.init()
    engine = Engine(0)
    try:
        gen, rev = PM.xcd_gen_cases(), PM.xcd_reveal_cases()
        for case in gen:
            run_gen_case(engine, case)
        for case in rev:
            run_reveal_case(engine, case)
        print(f"XCD_ROWS_OK {len(gen)} {len(rev)}")
    finally:
        engine.close()


def test_xcd_order_off(engine):
    """SDA_XCD_ORDER=0 (natural workgroup order, the documented A/B knob): the same rows, same checks."""
    gen, rev = PM.xcd_gen_cases(), PM.xcd_reveal_cases()
    assert len(gen) >= 90 and len(rev) >= 10
    run_gen_case(engine, gen[0])                          # this process (default order) first
    env = dict(os.environ, SDA_XCD_ORDER="0")
    env.pop("SDA_GEN_SIGNBIT", None)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_packed_matrix import run_xcd_rows; run_xcd_rows()"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"XCD_ROWS_OK {len(gen)} {len(rev)}" in r.stdout
