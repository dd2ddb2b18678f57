"""GPU: sda_draws_dev / sda_draws against the CPU model of the draw rule (tests/draws_model.py).

T = E.DRAWS_TILE is the number of elements one workgroup produces; the counts and offsets below sit on both sides of
its multiples, of the 8-draw ChaCha block and of the 2^32 block counter.  tests/test_draws_model.py checks on the CPU
that the two large bounds make at least a fifth of the elements retry (some of them four rounds deep), so those
cases cannot pass without the retry path.  Every output buffer sits between guard words.
"""
import numpy as np
import pytest

from sda_amd import SdaError
from sda_amd import engine as E
from tests import draws_model as DM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = E.DRAWS_TILE
KEY, STREAM = DM.TEST_KEY, DM.TEST_STREAM
P1 = 2147482800                 # configs[2]'s prime - 1: the packed-Shamir bound
GUARD = 0x5A5A5A5A5A5A5A5A
PAD = 16


def _dev(engine, key, stream_id, first, count, bound, into=None, at=0):
    """sda_draws_dev into a guarded buffer (or into `into` at element `at`); returns the buffer."""
    buf = into if into is not None else torch.full((PAD + count + PAD,), GUARD, dtype=torch.int64, device="cuda")
    engine.draws_dev(key, stream_id, first, count, bound, buf.data_ptr() + 8 * (PAD + at))
    torch.cuda.synchronize()
    return buf


def _body(buf, count):
    host = buf.cpu().numpy()
    assert (host[:PAD] == GUARD).all() and (host[PAD + count:] == GUARD).all(), "wrote around the output"
    return host[PAD:PAD + count]


def test_rfc7539_coordinates_on_the_device(engine):
    coords = DM.rfc_coordinates()
    assert any(first >> 35 for _, _, _, first, _ in coords)         # a non-zero high counter word
    for name, key, stream_id, first, want in coords:
        got = _body(_dev(engine, key, stream_id, first, 8, 1 << 32), 8)
        assert got.tolist() == want, name


@pytest.mark.parametrize("count", [0, 1, 7, 8, 9, T - 1, T, T + 1, 3 * T + 5])
def test_counts(engine, count):
    got = _body(_dev(engine, KEY, STREAM, 0, count, P1), count)
    assert np.array_equal(got, DM.draws(KEY, STREAM, 0, count, P1))


@pytest.mark.parametrize("first", [3, 2045, (1 << 35) - 5])
def test_ragged_ends(engine, first):
    count = T + 11
    got = _body(_dev(engine, KEY, STREAM, first, count, P1), count)
    assert np.array_equal(got, DM.draws(KEY, STREAM, first, count, P1))


@pytest.mark.parametrize("bound", [1, 2, 433, 2147482800, 2147482801, 1 << 31, 1 << 32, (1 << 32) + 1,
                                   DM.BOUND_QUARTER, DM.BOUND_THIRD, (1 << 63) - 1])
def test_bounds(engine, bound):
    count = 4096
    got = _body(_dev(engine, KEY, STREAM, 0, count, bound), count)
    assert (got >= 0).all() and (got.astype(np.uint64) < np.uint64(bound)).all()
    assert np.array_equal(got, DM.draws(KEY, STREAM, 0, count, bound))


def test_composition_and_host_form(engine):
    a, b, n = 1001, 2 * T + 3, 3 * T + 5
    whole = _body(_dev(engine, KEY, STREAM, 0, n, DM.BOUND_THIRD), n)
    parts = torch.full((PAD + n + PAD,), GUARD, dtype=torch.int64, device="cuda")
    for lo, hi in ((0, a), (a, b), (b, n)):
        _dev(engine, KEY, STREAM, lo, hi - lo, DM.BOUND_THIRD, into=parts, at=lo)
    assert np.array_equal(_body(parts, n), whole)
    assert np.array_equal(engine.draws(KEY, STREAM, 0, n, DM.BOUND_THIRD), whole)
    assert np.array_equal(engine.draws(KEY, STREAM, a, b - a, DM.BOUND_THIRD), whole[a:b])
    assert np.array_equal(whole, DM.draws(KEY, STREAM, 0, n, DM.BOUND_THIRD))


def test_stream_id_and_every_key_word_change_every_block(engine):
    n = 2 * T
    base = _body(_dev(engine, KEY, STREAM, 0, n, 1 << 62), n).reshape(-1, 8)
    others = [(KEY, STREAM + 1)] + [(KEY[:w] + (KEY[w] ^ 1,) + KEY[w + 1:], STREAM) for w in range(8)]
    for key, stream_id in others:
        got = _body(_dev(engine, key, stream_id, 0, n, 1 << 62), n).reshape(-1, 8)
        assert (got != base).any(axis=1).all(), (key, stream_id)
        assert np.array_equal(got.reshape(-1)[:64], DM.draws(key, stream_id, 0, 64, 1 << 62))


def test_statuses(engine):
    buf = torch.full((PAD + 8 + PAD,), GUARD, dtype=torch.int64, device="cuda")
    for bound in (0, -5):
        with pytest.raises(SdaError) as ei:
            engine.draws_dev(KEY, STREAM, 0, 8, bound, buf.data_ptr() + 8 * PAD)
        assert ei.value.status == E.ERR_PRECONDITION and "gen_range" in str(ei.value)
        with pytest.raises(SdaError) as ei:
            engine.draws(KEY, STREAM, 0, 8, bound)
        assert ei.value.status == E.ERR_PRECONDITION
    for call in (lambda: engine.draws_dev(KEY, STREAM, (1 << 64) - 4, 8, 433, buf.data_ptr() + 8 * PAD),
                 lambda: engine.draws(KEY, STREAM, (1 << 64) - 4, 8, 433),
                 lambda: engine.draws_dev(KEY, STREAM, 0, 8, 433, None)):
        with pytest.raises(SdaError) as ei:
            call()
        assert ei.value.status == E.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()
    # the last elements of the index space are a valid range
    top = _body(_dev(engine, KEY, STREAM, (1 << 64) - 8, 8, 433), 8)
    assert np.array_equal(top, DM.draws(KEY, STREAM, (1 << 64) - 8, 8, 433))
