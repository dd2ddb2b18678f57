"""GPU: sda_participant_share32_dev (mask -> int32 share generation -> int32 payload encoder) against the oracle's
step-wise flow, as tests/test_gpu_pipelines.py::test_participant_share_dev holds the i64 pipeline: D = 4099 (odd: a
ragged last batch), inputs and expected shares from OracleBackend.

Schemes (tests/encode32_cases.py: participant_schemes): S.CONFIG_PACKED (the direct int32 share-gen kernels), one
n + 1 = 81 scheme with k + t + 1 = 8 (the register kernels in EXACT and CANONICAL mode at any B: i64 shares into
scratch, then the narrowing pass) and one workspace-kernel scheme (n + 1 = 243), both from
tests/packed_matrix_cases.py.  tests/test_encode32_plan.py asserts each scheme's route on the CPU.
shares_out and the payload sit between guard words.
"""
import json
import os

import numpy as np
import pytest

from sda_amd import SdaError, schemes as S
from sda_amd import engine as E
from tests import encode32_cases as EC
from tests.oracle_backend import OracleBackend
from tests.pipeline import Draws, sharing_draws

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

P = S.CONFIG_PACKED.prime_modulus
D = EC.PARTICIPANT_D
GUARD32 = 0x5A5A5A5A
GUARD8 = 0xA5

SCHEMES = EC.participant_schemes()      # each scheme's share-gen route, in both modes: tests/test_encode32_plan.py
MASKINGS = {"none": S.NoMasking(), "full": S.FullMasking(P), "chacha": S.ChaChaMasking(P, D, 128)}


def _device(a, dtype=torch.int64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _inputs(ms, ss, d=D, secrets=None, seed=None):
    """(secrets, full masks, seed, draws, the oracle's shares [n][B])"""
    rng = Draws(0xABC)
    if secrets is None:
        secrets = np.random.default_rng(5).integers(-(P - 1), P, size=d, dtype=np.int64)
    be = OracleBackend()
    full = None
    if isinstance(ms, S.FullMasking):
        full = rng.below(ms.modulus, d)
        _, masked = be.secret_mask(ms, secrets, full_masks=full)
    elif isinstance(ms, S.ChaChaMasking):
        if seed is None:
            seed = rng.u32(ms.seed_words())
        _, masked = be.secret_mask(ms, secrets, seed=seed)
    else:
        masked = secrets
    draws = sharing_draws(ss, d, rng)
    return secrets, full, seed, draws, be.share_generate(ss, masked, draws)


def _expected(ss, exp, mode):
    """the oracle's shares as the mode states them, narrowed (every share is a `% p` result: |share| < p < 2^31)"""
    p = ss.prime_modulus
    assert (np.abs(exp) < p).all()
    if mode == E.REVEAL_CANONICAL:
        exp = np.mod(exp, p)
    return exp.astype(np.int32)


class _Run:
    """One call of sda_participant_share32_dev into guarded buffers."""

    def __init__(self, engine, ms, ss, inputs, mode, off=0, payload=True, cap=None, d=D):
        secrets, full, seed, draws, exp = inputs
        self.n, self.B = exp.shape
        n, B = self.n, self.B
        self.keep = (_device(secrets), _device(draws), _device(full) if full is not None else None)
        self.sh = torch.full((8 + off + n * B + 8,), GUARD32, dtype=torch.int32, device="cuda")
        self.lo = 8 + off
        ptr = self.sh.data_ptr() + 4 * self.lo
        assert ptr % 16 == 4 * off
        self.cap = n * B * 5 if cap is None else cap
        self.pay = torch.full((16 + n * B * 5 + 64,), GUARD8, dtype=torch.uint8, device="cuda") if payload else None
        self.rb = engine.participant_share32_dev(
            ms, ss, self.keep[0].data_ptr(), d, self.keep[1].data_ptr(), ptr, seed=seed,
            full_masks_ptr=self.keep[2].data_ptr() if full is not None else None,
            payload_ptr=self.pay.data_ptr() + 16 if payload else None, payload_cap=self.cap if payload else 0,
            mode=mode)
        torch.cuda.synchronize()

    def shares(self):
        host = self.sh.cpu().numpy()
        hi = self.lo + self.n * self.B
        assert (host[:self.lo] == GUARD32).all() and (host[hi:] == GUARD32).all(), "wrote around shares_out"
        return host[self.lo:hi].reshape(self.n, self.B)

    def payload(self):
        host = self.pay.cpu().numpy()
        total = int(self.rb.sum())
        assert (host[:16] == GUARD8).all() and (host[16 + total:] == GUARD8).all(), "wrote around the payload"
        return host[16:16 + total].tobytes()


def _check(oracle, run, want):
    assert np.array_equal(run.shares(), want)
    host = run.payload()
    off = np.concatenate([[0], np.cumsum(run.rb)]).astype(np.int64)
    for c in range(run.n):
        assert host[off[c]:off[c + 1]] == oracle.varint_encode(want[c].astype(np.int64)), f"clerk {c}"


@pytest.mark.parametrize("mode", [E.REVEAL_EXACT, E.REVEAL_CANONICAL], ids=["exact", "canonical"])
@pytest.mark.parametrize("ms", list(MASKINGS), ids=list(MASKINGS))
@pytest.mark.parametrize("ss", list(SCHEMES), ids=list(SCHEMES))
def test_participant_share32_dev(engine, oracle, ss, ms, mode):
    ms, ss = MASKINGS[ms], SCHEMES[ss]
    inputs = _inputs(ms, ss)
    off = 1 if isinstance(ms, S.ChaChaMasking) else 0        # shares_out 4 bytes off a 16-byte boundary
    run = _Run(engine, ms, ss, inputs, mode, off=off)
    _check(oracle, run, _expected(ss, inputs[4], mode))


def test_twin_i64_pipeline_gives_the_same_outputs(engine):
    ms, ss = MASKINGS["chacha"], S.CONFIG_PACKED
    inputs = _inputs(ms, ss)
    secrets, _, seed, draws, exp = inputs
    run = _Run(engine, ms, ss, inputs, E.REVEAL_EXACT)
    record32 = engine.chacha_last_launch()
    n, B = exp.shape
    d_sec, d_dr = _device(secrets), _device(draws)
    out = torch.empty((n, B), dtype=torch.int64, device="cuda")
    cap = n * B * 10 + 32
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    rb = engine.participant_share_dev(ms, ss, d_sec.data_ptr(), D, d_dr.data_ptr(), out.data_ptr(), seed=seed,
                                      payload_ptr=pay.data_ptr(), payload_cap=cap)
    torch.cuda.synchronize()
    assert engine.chacha_last_launch() == record32
    assert rb.tolist() == run.rb.tolist()
    assert pay.cpu().numpy()[:int(rb.sum())].tobytes() == run.payload()
    wide = out.cpu().numpy()
    assert np.array_equal(wide.astype(np.int32), run.shares()) and np.array_equal(wide.astype(np.int32), wide)


def test_chacha_redo_after_a_late_rejection(engine, oracle):
    """A mask stream that really rejects a draw (tests/golden/chacha_rejects.json, as tests/test_gpu_chacha_rejects.py
    uses them for the i64 pipeline): the rejection count is read at the end of the call, the mask is redone
    exactly, and share generation and the encode run again."""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "chacha_rejects.json")))
    m = min(int(k) for k in g["moduli"])
    s = g["moduli"][str(m)][0][0]
    d = 65536
    ms, ss = S.ChaChaMasking(m, d, 128), S.CONFIG_PACKED
    secrets = np.random.default_rng(9).integers(-(m - 1), m, size=d, dtype=np.int64)
    inputs = _inputs(ms, ss, d=d, secrets=secrets, seed=np.array([s, 0x5DA, 7, 11], np.uint32))
    run = _Run(engine, ms, ss, inputs, E.REVEAL_EXACT, d=d)
    path, _, fixups = engine.chacha_last_launch()
    _check(oracle, run, _expected(ss, inputs[4], E.REVEAL_EXACT))
    assert path == 4 and fixups >= 1


def test_payload_none_generates_shares_only(engine):
    ms, ss = MASKINGS["full"], S.CONFIG_PACKED
    inputs = _inputs(ms, ss)
    run = _Run(engine, ms, ss, inputs, E.REVEAL_EXACT, payload=False)
    assert np.array_equal(run.shares(), _expected(ss, inputs[4], E.REVEAL_EXACT))
    assert run.rb.tolist() == [0] * run.n


def test_errors(engine):
    ms, ss = MASKINGS["none"], S.CONFIG_PACKED
    inputs = _inputs(ms, ss)
    with pytest.raises(SdaError) as ei:
        add = S.Additive(4, P)
        _Run(engine, ms, add, _inputs(ms, add), E.REVEAL_EXACT)
    assert ei.value.status == E.ERR_UNSUPPORTED and "draws" in str(ei.value)
    with pytest.raises(SdaError) as ei:
        _Run(engine, ms, ss, inputs, 7)
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    total = int(_Run(engine, ms, ss, inputs, E.REVEAL_EXACT).rb.sum())
    with pytest.raises(SdaError) as ei:
        _Run(engine, ms, ss, inputs, E.REVEAL_EXACT, cap=total - 1)
    assert ei.value.status == E.ERR_INVALID_ARGUMENT
    _Run(engine, ms, ss, inputs, E.REVEAL_EXACT, cap=total)
