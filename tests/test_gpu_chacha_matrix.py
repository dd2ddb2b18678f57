"""GPU: every dispatch of the ChaCha mask expansion (sda_amd/csrc/chacha.hip) against the oracle, with the
kernel that ran asserted through sda_chacha_last_launch -- a case that reaches another kernel than the one it
names fails even when the numbers are right.

The oracle (oracle.chacha_mask_combine / oracle.chacha_mask) walks each stream sequentially with gen_range's
rejection loop; every comparison is bit-exact.  Seeds come from np.random.default_rng with fixed seeds, four
words each.  The moduli are classified by the dispatcher's own rules, UINT64_MAX % m + 1 <= 2^36 (fast path)
and max_c = UINT64_MAX // (m - 1) (the u64 accumulator's headroom: one canonical partial < m per chunk):
  lazy 96-bit sums (m <= 2^32)   1, 2, 433, 2147482801, 4294901761, 2^32 (the last lazy modulus: 2^64 mod m = 0)
  64-bit Barrett                 2^32 + 1 (one rejected value), 68719676673, 2^40 - 87, 2^48 - 59,
                                 2^61 - 1 (max_c 8), 2^62 - 57 and 2^62 - 1 (max_c 4)
"""
import json
import os

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests.util import assert_same

gpu = pytest.mark.gpu          # per test: the two checks of the cases themselves need no device
torch = pytest.importorskip("torch")

U64_MAX = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LAZY = [1, 2, 433, 2147482801, 4294901761, 1 << 32]
BARRETT = [(1 << 32) + 1, 68719676673, (1 << 40) - 87, (1 << 48) - 59, (1 << 61) - 1, (1 << 62) - 57, (1 << 62) - 1]
FAST = LAZY + BARRETT

_G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "chacha_rejects.json")))
REJECTS = {int(m): [tuple(h) for h in hits] for m, hits in _G["moduli"].items()}


def max_c(m, n_seeds):
    """chacha_fast_enqueue's cap on the chunks: at most one per seed, 65535, and the accumulator's headroom."""
    c = min(n_seeds, 65535)
    return min(c, U64_MAX // (m - 1)) if m > 1 else c


def test_moduli_are_classified_as_documented():
    for m in FAST:
        assert U64_MAX % m + 1 <= 1 << 36 and m <= 1 << 62, m          # chacha_needs_stream_path is false
    assert all(m <= 1 << 32 for m in LAZY) and all(m > 1 << 32 for m in BARRETT)
    assert U64_MAX % ((1 << 32) + 1) + 1 == 1                            # exactly one rejected value
    assert (U64_MAX % (1 << 32) + 1) % (1 << 32) == 0                    # r64 = 0
    assert [max_c(m, 1 << 20) for m in BARRETT[-3:]] == [8, 4, 4]


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("SDA_CHACHA_CHUNKS", "SDA_CHACHA_SK", "SDA_CHACHA_PATH"):
        monkeypatch.delenv(k, raising=False)


def _random_seeds(rng_seed, n):
    return np.random.default_rng(rng_seed).integers(0, 2**32, size=(n, 4), dtype=np.uint64).astype(np.int64)


_EXPECTED = {}


def _expected(oracle, m, D, key, rows):
    """oracle.chacha_mask_combine, computed once per (modulus, dimension, seed set) and shared, read-only."""
    k = (m, D, key)
    if k not in _EXPECTED:
        exp = oracle.chacha_mask_combine(m, D, rows)
        exp.setflags(write=False)
        _EXPECTED[k] = exp
    return _EXPECTED[k]


def _combine(engine, m, D, rows):
    """sda_chacha_mask_combine_dev into a poisoned buffer -> (result, (path, grid_y, fixups))."""
    seeds = torch.as_tensor(np.ascontiguousarray(rows).astype(np.uint32).view(np.int32)).cuda()
    out = torch.full((D,), -7, dtype=torch.int64, device="cuda")
    engine.chacha_mask_combine_dev(m, D, seeds.data_ptr(), rows.shape[1], rows.shape[0], out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), engine.chacha_last_launch()


# ------------------------------------------------------------------ a. forced grids
N_FORCED = 37


def _forced_chunks(m):
    cap = max_c(m, N_FORCED)
    cs = [c for c in (1, 3, 12, 37) if c <= cap]
    return cs + ([cap] if cap not in cs else [])        # the cap itself: 4 (2^62 - 57, 2^62 - 1), 8 (2^61 - 1)


@gpu
@pytest.mark.parametrize("D", [9, 2049, 10_235])
@pytest.mark.parametrize("m,chunks", [(m, c) for m in FAST for c in _forced_chunks(m)])
def test_forced_grid(engine, oracle, monkeypatch, m, chunks, D):
    """SDA_CHACHA_CHUNKS (which also disables stream-K) over 37 seeds: 1 = the multi-seed DIRECT kernel, 3 =
    13 + 13 + 11 seeds per workgroup, 12 = 4 per chunk with the last two chunks empty, 37 = one seed each, and
    the headroom cap itself where it is below 37.  D = 9: a short last block; 2049: one element in the second
    tile; 10 235: five tiles, the last one ragged."""
    rows = _random_seeds(1000 + D, N_FORCED)
    exp = _expected(oracle, m, D, "forced", rows)
    monkeypatch.setenv("SDA_CHACHA_CHUNKS", str(chunks))
    got, (path, grid_y, fixups) = _combine(engine, m, D, rows)
    assert (path, grid_y) == (E.CHACHA_DIRECT if chunks == 1 else E.CHACHA_CHUNKED, chunks)
    assert_same(got, exp)
    assert fixups == 0


# ------------------------------------------------------------------ b. headroom at the cap
@gpu
@pytest.mark.parametrize("m,cap", [((1 << 62) - 57, 4), ((1 << 61) - 1, 8)])
def test_headroom_at_the_cap(engine, oracle, monkeypatch, m, cap):
    """2000 seeds in max_c chunks: every u64 accumulator receives max_c canonical partials just below m, i.e.
    up to 2^64 - 232 (m = 2^62 - 57) or 2^64 - 16 (m = 2^61 - 1).  The chunked kernel's own partials (seeds
    [c per, (c + 1) per)) are recomputed with the oracle: their exact sum gives the expected vector again and
    passes 2^63 in many elements, so neither a signed nor a wrapped accumulator can pass.  Also without the
    knob: the dispatcher itself must stop at max_c chunks (its grid would hold 359) and refuse stream-K (401
    runs per tile), and it must ignore a knob value above the cap."""
    N, D = 2000, 10_235
    assert max_c(m, N) == cap
    rows = _random_seeds(m % 1013, N)
    exp = _expected(oracle, m, D, "headroom", rows)
    per = (N + cap - 1) // cap
    partial = [oracle.chacha_mask_combine(m, D, rows[c * per:(c + 1) * per]).astype(object) for c in range(cap)]
    acc = sum(partial)
    assert ((acc % m) == exp.astype(object)).all()
    assert int(acc.max()) <= U64_MAX
    over = int((acc >= (1 << 63)).sum())
    print(f"m={m}: {over} of {D} accumulators pass 2^63, max {int(acc.max()):#x}")
    assert over > D // 10
    for knob in (str(cap), None, str(cap + 1)):
        if knob is None:
            monkeypatch.delenv("SDA_CHACHA_CHUNKS")
        else:
            monkeypatch.setenv("SDA_CHACHA_CHUNKS", knob)
        got, (path, grid_y, fixups) = _combine(engine, m, D, rows)
        assert (path, grid_y, fixups) == (E.CHACHA_CHUNKED, cap, 0), knob
        assert_same(got, exp)


# ------------------------------------------------------------------ c. stream-K, chosen by the dispatcher
STREAM_K_SHAPES = [((1 << 61) - 1, 1_228_795, 16), ((1 << 62) - 57, 2_457_595, 8),
                   ((1 << 40) - 87, 67_001, 256), (2147482801, 67_001, 256)]


def test_stream_k_shapes_satisfy_the_dispatch_rule():
    """chacha_fast_enqueue's rule, restated: stream-K when the chunked grid fills less than 95 % of its rounds
    of cap_wgs resident workgroups and ceil(n / (units / G)) + 1 runs per tile fit max_c.  Both occupancy
    figures are workgroups per CU times the MI355X's 256 CUs and nobody pins the per-CU counts, so the shapes
    hold for 4 .. 9 workgroups per CU (1024 .. 2304 resident), and the second condition for every cap_sk there."""
    for m, D, n in STREAM_K_SHAPES:
        gx = ((D + 7) // 8 + 255) // 256
        cap = max_c(m, n)
        for cap_wgs in range(1024, 2305, 256):
            chunks = min((cap_wgs + gx - 1) // gx, cap)
            wgs = gx * chunks
            rounds = (wgs + cap_wgs - 1) // cap_wgs
            assert wgs < 0.95 * rounds * cap_wgs, (m, cap_wgs)
        for cap_sk in range(1024, 2305):
            units = gx * n
            G = min(units, cap_sk)
            assert (n + units // G - 1) // (units // G) + 1 <= cap, (m, cap_sk)


@gpu
@pytest.mark.parametrize("m,D,n", STREAM_K_SHAPES)
def test_stream_k_without_knobs(engine, oracle, monkeypatch, m, D, n):
    """No knobs: the dispatcher picks chacha_combine_sk_kernel (both LAZY instantiations; runs that start
    mid-tile, at most max_c = 8 / 4 of them per tile for the two big moduli).  SDA_CHACHA_SK=0 then takes the
    chunked grid for the same job; both equal the oracle."""
    rows = _random_seeds(m % 1019 + n, n)
    exp = _expected(oracle, m, D, "sk", rows)
    got, (path, grid_y, fixups) = _combine(engine, m, D, rows)
    print(f"stream-K m={m} D={D} n={n}: path {path}, grid {grid_y}")
    assert path == E.CHACHA_STREAM_K and 1 <= grid_y <= ((D + 7) // 8 + 255) // 256 * n
    assert_same(got, exp)
    assert fixups == 0
    monkeypatch.setenv("SDA_CHACHA_SK", "0")
    got, (path, grid_y, fixups) = _combine(engine, m, D, rows)
    print(f"chunked  m={m} D={D} n={n}: path {path}, grid {grid_y}")
    assert path == E.CHACHA_CHUNKED and 2 <= grid_y <= max_c(m, n)
    assert_same(got, exp)
    assert fixups == 0


# ------------------------------------------------------------------ d. rejections in multi-seed workgroups
def _reject_rows(m, n, rng_seed):
    rows = [np.array([s, 0x5DA, 7, 11], np.int64) for s, _ in REJECTS[m]]
    return np.concatenate([np.stack(rows), _random_seeds(rng_seed, n - len(rows))])


def _rejecting_streams(oracle, m, D, rows):
    """Streams with a rejected draw among their first D pairs: the fix-up launches the engine owes."""
    hits = [s for s in range(rows.shape[0]) if oracle.chacha_first_reject(m, rows[s].astype(np.uint32), D) < D]
    # a random seed rejects with probability < 2^-28 per draw: only the golden seeds may (else: another rng seed)
    assert hits == list(range(len(REJECTS[m]))), hits
    return len(hits)


@gpu
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("m", sorted(REJECTS))
def test_rejections_in_multi_seed_lanes(engine, oracle, monkeypatch, m, chunks):
    """The (seed, pair) event written from inside a lane's seed loop (32 or 16 seeds per workgroup; the golden
    seeds come first, so all of them share chunk 0), and one fix-up launch per rejecting stream."""
    D, n = 65_536, 32
    rows = _reject_rows(m, n, 77)
    want = _rejecting_streams(oracle, m, D, rows)
    exp = _expected(oracle, m, D, "rej32", rows)
    monkeypatch.setenv("SDA_CHACHA_CHUNKS", str(chunks))
    got, (path, grid_y, fixups) = _combine(engine, m, D, rows)
    assert (path, grid_y) == (E.CHACHA_DIRECT if chunks == 1 else E.CHACHA_CHUNKED, chunks)
    assert_same(got, exp)
    assert fixups == want


@gpu
@pytest.mark.parametrize("m", sorted(REJECTS))
def test_rejections_in_stream_k_runs(engine, oracle, m):
    """The same events logged from stream-K runs (33 tiles x 256 seeds: workgroups start mid-tile), no knobs."""
    D, n = 67_001, 256
    rows = _reject_rows(m, n, 78)
    want = _rejecting_streams(oracle, m, D, rows)
    exp = _expected(oracle, m, D, "rej256", rows)
    got, (path, grid_y, fixups) = _combine(engine, m, D, rows)
    print(f"stream-K rejects m={m}: path {path}, grid {grid_y}, fixups {fixups}")
    assert path == E.CHACHA_STREAM_K
    assert_same(got, exp)
    assert fixups == want


# ------------------------------------------------------------------ e. one stream: the participant's mask
def _secret_variants(m, D, rng):
    """Secrets over the whole i64 range, with the extremes and the edges of add_trem's fast branch planted at
    the first and last positions and on both sides of the 2048-element tile boundary; a dimension too short to
    hold them gets one variant per planted value."""
    special = [I64_MIN, I64_MAX, -m, m, -(m - 1), m - 1, 0]
    base = rng.integers(I64_MIN, I64_MAX, size=D, dtype=np.int64, endpoint=True)
    if D < 2 * len(special):
        out = []
        for v in special:
            s = base.copy()
            s[0] = s[-1] = v
            out.append(s)
        return out
    s = base.copy()
    k = len(special)
    s[:k] = special
    s[D - k:] = special
    if D > 2048:
        lo = min(k, D - 2048)
        s[2048 - k:2048] = special
        s[2048:2048 + lo] = special[::-1][:lo]
    return [s]


@gpu
@pytest.mark.parametrize("D", [1, 2047, 2049, 10_235])
@pytest.mark.parametrize("m", FAST)
def test_single_stream_mask(engine, oracle, m, D):
    """masked = (secret + draw) % m over one stream, secrets anywhere in i64: sda_secret_mask (the one-seed
    DIRECT combine, then the elementwise add) and sda_participant_share_dev (chacha_mask_add_kernel: add_trem's
    compare/adjust branch for secrets in (-m, m), its Barrett branch and the wrapping add outside).  The oracle
    adds with or_wadd, a wrapping u64 add, as Rust release arithmetic does, so the whole range is defined.
    Additive(2, m) with zero draws hands the masked secrets out as share row 1."""
    rng = np.random.default_rng(m % 1021 + D)
    seed = rng.integers(0, 2**32, size=4, dtype=np.uint64).astype(np.uint32)
    ms, ss = S.ChaChaMasking(m, D, 128), S.Additive(2, m)
    draws = torch.zeros(D, dtype=torch.int64, device="cuda")
    for secrets in _secret_variants(m, D, rng):
        exp = oracle.chacha_mask(m, seed, secrets)
        mask, masked = engine.secret_mask(ms, secrets, seed=seed)
        assert engine.chacha_last_launch() == (E.CHACHA_DIRECT, 1, 0)
        assert_same(mask, seed.astype(np.int64))
        assert_same(masked, exp)
        d_sec = torch.as_tensor(secrets).cuda()
        shares = torch.full((2, D), -7, dtype=torch.int64, device="cuda")
        engine.participant_share_dev(ms, ss, d_sec.data_ptr(), D, draws.data_ptr(), shares.data_ptr(), seed=seed)
        torch.cuda.synchronize()
        assert engine.chacha_last_launch() == (E.CHACHA_MASK_ADD, 1, 0)
        got = shares.cpu().numpy()
        assert_same(got[1], exp)
        assert not got[0].any()


# ------------------------------------------------------------------ f. the diagnostic itself
@gpu
def test_last_launch_record(oracle, monkeypatch):
    """A fresh handle reports no launch; a call of dimension 0 leaves the record; the stream path is reported
    for a modulus that needs it and for SDA_CHACHA_PATH=stream; NULL is an invalid argument."""
    import ctypes as C

    from sda_amd import Engine, SdaError
    eng = Engine(0)
    try:
        assert eng.chacha_last_launch() == (E.CHACHA_NONE, 0, 0)
        rows = _random_seeds(5, 3)
        for m in ((1 << 40) + 7, (1 << 62) + 1):                          # 2^40 rejected values; m > 2^62
            got, rec = _combine(eng, m, 777, rows)
            assert rec == (E.CHACHA_STREAM, 0, 0)
            assert_same(got, oracle.chacha_mask_combine(m, 777, rows))
        got, rec = _combine(eng, 433, 777, rows)
        assert rec[0] in (E.CHACHA_DIRECT, E.CHACHA_CHUNKED, E.CHACHA_STREAM_K) and rec[1] >= 1
        seeds = torch.zeros((3, 4), dtype=torch.int32, device="cuda")
        eng.chacha_mask_combine_dev(1 << 62, 0, seeds.data_ptr(), 4, 3, seeds.data_ptr())      # D = 0: nothing
        assert eng.chacha_last_launch() == rec
        monkeypatch.setenv("SDA_CHACHA_PATH", "stream")
        got, rec = _combine(eng, 433, 777, rows)
        assert rec == (E.CHACHA_STREAM, 0, 0)
        assert_same(got, oracle.chacha_mask_combine(433, 777, rows))
        v = C.c_uint64()
        with pytest.raises(SdaError) as ei:
            E._check(eng.lib.sda_chacha_last_launch(eng.h, None, C.byref(v), C.byref(v)))
        assert ei.value.status == E.ERR_INVALID_ARGUMENT
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("m", sorted(REJECTS))
def test_pipelines_record_their_late_resolve(engine, oracle, m):
    """The recipient pipeline resolves its mask's rejections after the reveal was queued, the participant redoes
    a rejecting mask exactly: both leave the fix-up count in the record (and the results equal the oracle's)."""
    D = 65_536
    ms, ss = S.ChaChaMasking(m, D, 128), S.Additive(2, m)
    rows = _reject_rows(m, 12, 79)
    want = _rejecting_streams(oracle, m, D, rows)
    rng = np.random.default_rng(m % 89)
    clerks = np.stack([rng.integers(-(m - 1), m, size=D, dtype=np.int64) for _ in range(2)])
    mask = _expected(oracle, m, D, "rej12", rows)
    exp = oracle.positive(m, oracle.unmask(m, mask, oracle.combine(m, clerks)))
    seeds = torch.as_tensor(rows.astype(np.uint32).view(np.int32)).cuda()
    sh = torch.as_tensor(clerks).cuda()
    out = torch.full((D,), -7, dtype=torch.int64, device="cuda")
    n = engine.recipient_reveal_dev(ms, seeds.data_ptr(), rows.shape[0], 4, ss, D, [0, 1], sh.data_ptr(), D, m,
                                    out.data_ptr(), D)
    torch.cuda.synchronize()
    path, grid_y, fixups = engine.chacha_last_launch()
    assert n == D and path in (E.CHACHA_DIRECT, E.CHACHA_CHUNKED, E.CHACHA_STREAM_K) and fixups == want
    assert_same(out.cpu().numpy(), exp)
    # participant: the first golden seed's own stream
    secrets = rng.integers(-(m - 1), m, size=D, dtype=np.int64)
    seed = rows[0].astype(np.uint32)
    d_sec = torch.as_tensor(secrets).cuda()
    draws = torch.zeros(D, dtype=torch.int64, device="cuda")
    shares = torch.full((2, D), -7, dtype=torch.int64, device="cuda")
    engine.participant_share_dev(ms, ss, d_sec.data_ptr(), D, draws.data_ptr(), shares.data_ptr(), seed=seed)
    torch.cuda.synchronize()
    assert engine.chacha_last_launch() == (E.CHACHA_MASK_ADD, 1, 1)
    assert_same(shares.cpu().numpy()[1], oracle.chacha_mask(m, seed, secrets))
