"""GPU: the keyed host entry points (sda_share_generate_keyed, sda_secret_mask_keyed) and the device chain
sda_draws_dev -> sda_participant_share32_dev.

share_generate_keyed must equal share_generate fed with sda_draws of the same key, stream and bound (the draws
themselves are held to the CPU model here and in tests/test_gpu_draws.py), on one device and on a three-slice
handle whose slices start their draws at b0 * t (packed) or d0 * (n - 1) (Additive).  Dimensions: none, one, and
both sides of one batch, plus 2049 batches and a ragged one -- more draws than one workgroup makes, and slices of
a three-way split that start inside a ChaCha block.
"""
import numpy as np
import pytest

from sda_amd import Engine, SdaError, schemes as S
from sda_amd import engine as E
from tests import draws_model as DM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEY, STREAM = DM.TEST_KEY, DM.TEST_STREAM
SCHEMES = {"additive": S.Additive(3, 433), "full_loop": S.FULL_LOOP_PACKED, "config": S.CONFIG_PACKED}


def _plan(sch, d):
    """(modulus, number of draws, their bound) of a generate call"""
    if isinstance(sch, S.Additive):
        return sch.modulus, d * (sch.share_count - 1), sch.modulus
    k, t = sch.secret_count, sch.privacy_threshold()
    return sch.prime_modulus, ((d + k - 1) // k) * t, sch.prime_modulus - 1


def _dims(sch):
    k = sch.input_size()
    return sorted({0, 1, k - 1, k, k + 1, 2049 * k + 3})


@pytest.fixture(scope="module")
def multi3():
    e = Engine(devices=[0, 0, 0])
    yield e
    e.close()


@pytest.mark.parametrize("name", list(SCHEMES))
def test_share_generate_keyed(engine, multi3, name):
    sch = SCHEMES[name]
    for d in _dims(sch):
        m, n_draws, bound = _plan(sch, d)
        secrets = np.random.default_rng(d + 1).integers(0, m, size=d, dtype=np.int64)
        draws = engine.draws(KEY, STREAM, 0, n_draws, bound)
        assert np.array_equal(draws, DM.draws(KEY, STREAM, 0, n_draws, bound)), d
        want = engine.share_generate(sch, secrets, draws)
        got = engine.share_generate_keyed(sch, secrets, KEY, STREAM)
        assert got.shape == want.shape and np.array_equal(got, want), (name, d)
        rec = engine.secret_reconstruct(sch, d, [(i, got[i]) for i in range(sch.output_size())])
        assert np.array_equal(np.mod(rec, m), secrets), (name, d)
        split = multi3.share_generate_keyed(sch, secrets, KEY, STREAM)
        assert np.array_equal(split, want), (name, d, "three slices")
        if d:
            other = engine.share_generate_keyed(sch, secrets, KEY, STREAM + 1)
            assert not np.array_equal(other, want), (name, d)


def test_share_generate_keyed_keeps_the_scheme_checks(engine):
    secrets = np.arange(8, dtype=np.int64)
    for sch, status in ((S.Additive(0, 433), E.ERR_PRECONDITION), (S.Additive(3, 0), E.ERR_PRECONDITION),
                        (S.Additive(3, -7), E.ERR_PRECONDITION),
                        (S.PackedShamir(8, 26, 7, 2147482800, 2, 3), E.ERR_UNSUPPORTED)):
        with pytest.raises(SdaError) as plain:
            engine.share_generate(sch, secrets, np.zeros(16 if sch.output_size() else 0, np.int64))
        with pytest.raises(SdaError) as keyed:
            engine.share_generate_keyed(sch, secrets, KEY, STREAM)
        assert keyed.value.status == plain.value.status == status, sch


def test_secret_mask_keyed(engine, oracle):
    m = S.CONFIG_PACKED.prime_modulus
    for d in (0, 1, 2 * E.DRAWS_TILE + 5):
        secrets = np.random.default_rng(d).integers(-(m - 1), m, size=d, dtype=np.int64)
        mask, masked = engine.secret_mask_keyed(S.FullMasking(m), secrets, KEY, STREAM)
        want = DM.draws(KEY, STREAM, 0, d, m)
        assert np.array_equal(mask, want), d
        assert np.array_equal(masked, oracle.full_mask(m, want, secrets)), d
        plain_mask, plain_masked = engine.secret_mask(S.FullMasking(m), secrets, full_masks=want)
        assert np.array_equal(plain_mask, mask) and np.array_equal(plain_masked, masked), d
    for ms in (S.NoMasking(), S.ChaChaMasking(m, 8, 128)):
        with pytest.raises(SdaError) as ei:
            engine.secret_mask_keyed(ms, np.arange(8, dtype=np.int64), KEY, STREAM)
        assert ei.value.status == E.ERR_INVALID_ARGUMENT and "sda_secret_mask" in str(ei.value)
    for bad in (0, -433):
        with pytest.raises(SdaError) as ei:
            engine.secret_mask_keyed(S.FullMasking(bad), np.arange(8, dtype=np.int64), KEY, STREAM)
        assert ei.value.status == E.ERR_PRECONDITION


def test_draws_dev_feeds_participant_share32_dev(engine):
    """The device chain of INTEGRATION.md: the draws never exist on the host."""
    ss, ms = S.CONFIG_PACKED, S.NoMasking()
    p, k, t, n = ss.prime_modulus, ss.secret_count, ss.privacy_threshold(), ss.share_count
    d = 4099
    B = (d + k - 1) // k
    secrets = torch.as_tensor(np.random.default_rng(4).integers(0, p, size=d, dtype=np.int64)).cuda()
    cap = n * B * 5 + 32

    def run(draws_ptr):
        sh = torch.zeros((n, B), dtype=torch.int32, device="cuda")
        pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        rb = engine.participant_share32_dev(ms, ss, secrets.data_ptr(), d, draws_ptr, sh.data_ptr(),
                                            payload_ptr=pay.data_ptr(), payload_cap=cap)
        torch.cuda.synchronize()
        return sh.cpu().numpy(), rb, pay.cpu().numpy()[:int(rb.sum())].tobytes()

    on_dev = torch.zeros(B * t, dtype=torch.int64, device="cuda")
    engine.draws_dev(KEY, STREAM, 0, B * t, p - 1, on_dev.data_ptr())
    uploaded = torch.as_tensor(DM.draws(KEY, STREAM, 0, B * t, p - 1)).cuda()
    got, want = run(on_dev.data_ptr()), run(uploaded.data_ptr())
    assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist() and got[2] == want[2]
    assert np.abs(got[0]).max() > 0
