"""CPU: the expected values of keyed Additive share generation (sda_additive_generate_keyed_dev), and checks that the
inputs tests/test_gpu_additive_keyed.py feeds the kernel really reach what they are there for -- retried draws, a
retried draw in a ChaCha block shared by several columns, a fold whose order shows, slices that start or end inside
a block -- so that the GPU test cannot pass vacuously.

Expected values come from the CPU alone: oracle.additive_generate over tests/draws_model.py's draws.  Column d of a
call is absolute column c = first_column + d and owns draws c (n - 1) + j, j < n - 1.
"""
import numpy as np

from oracle import oracle as O
from sda_amd import engine as E
from tests import draws_model as DM

KEY, STREAM = DM.TEST_KEY, DM.TEST_STREAM
T = E.ADDITIVE_KEYED_TILE
M_SMALL, M_PRIME = 433, 2147482801
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)

# (modulus, share_count) at bounds whose reject rate is about 1/4 and 1/3, and the column count of those cases
RETRY_CASES = [(DM.BOUND_QUARTER, 2), (DM.BOUND_QUARTER, 4), (DM.BOUND_THIRD, 2), (DM.BOUND_THIRD, 4)]
RETRY_COLUMNS = 600


def _first_widths(n, first):
    """Two slice widths for a slice starting at column `first`: one whose end falls inside a ChaCha block, one whose
    end is a block boundary."""
    n1 = n - 1
    ragged = T + 2
    while (first + ragged) * n1 % 8 == 0:
        ragged += 1
    aligned = 40
    while (first + aligned) * n1 % 8:
        aligned += 1
    return ragged, aligned


# (share_count, first_column, width) of the first_column cases; the full job they are slices of has FIRST_TOTAL columns
FIRST_CASES = [(n, f, w) for n in (3, 4, 10) for f in (1, 5, T + 3) for w in _first_widths(n, f)]
FIRST_TOTAL = 2 * T + 8


def expected(m, n, secrets, first_column=0, key=KEY, stream_id=STREAM):
    """out[n][len(secrets)] of sda_additive_generate_keyed_dev, from the CPU oracle and the CPU draws model."""
    secrets = np.asarray(secrets, dtype=np.int64)
    draws = DM.draws(key, stream_id, first_column * (n - 1), secrets.size * (n - 1), m)
    return O.additive_generate(m, n, secrets, draws)


def matrix_secrets(m, d, seed):
    """Uniform on (-m, m), with raw values the fold has to reduce itself at a few positions."""
    s = np.random.default_rng(seed).integers(-(m - 1), m, size=d, dtype=np.int64)
    raw = [5 * m + 3, -(5 * m + 3), I64_MAX, I64_MIN + 1]
    for i, v in enumerate(raw):
        if 3 * i + 1 < d:
            s[3 * i + 1] = v
    if d:
        s[d - 1] = raw[d % 4]
    return s


def _trem(v, m):
    """Rust's truncated `%` on Python integers."""
    return -((-v) % m) if v < 0 else v % m


def test_retry_cases_contain_retried_draws_in_blocks_that_straddle_columns():
    for m, n in RETRY_CASES:
        n1 = n - 1
        _, rounds = DM.draws_with_rounds(KEY, STREAM, 0, RETRY_COLUMNS * n1, m)
        retried = np.nonzero(rounds)[0]
        assert retried.size > RETRY_COLUMNS * n1 // 8, (m, n)          # about a quarter / a third of them
        assert rounds.max() >= 2, (m, n)                                # and not only the first retry round
        straddling = [e for e in retried if (8 * (e >> 3)) // n1 != (8 * (e >> 3) + 7) // n1]
        assert straddling, (m, n)


def test_fold_order_shows_on_a_raw_secret():
    """Secret 5m + 3 with n = 3: the sequential fold of additive.rs:47 first reduces to [0, m) and may then go
    negative; a one-shot (s - x0 - x1) % m of the positive difference never does."""
    m, n, cols = M_SMALL, 3, 64
    secrets = np.full(cols, 5 * m + 3, dtype=np.int64)
    want = expected(m, n, secrets)
    one_shot = np.array([_trem(int(secrets[d]) - int(want[0, d]) - int(want[1, d]), m) for d in range(cols)])
    assert (one_shot >= 0).all()
    assert ((want[2] - one_shot) % m == 0).all()
    differs = np.nonzero(np.sign(want[2]) != np.sign(one_shot))[0]
    assert differs.size, "no column of the case tells the fold order"
    assert (want[2][differs] < 0).all()


def test_expected_is_the_draws_then_the_fold():
    m, n, d = M_PRIME, 4, 37
    secrets = matrix_secrets(m, d, 1)
    want = expected(m, n, secrets, first_column=5)
    draws = DM.draws(KEY, STREAM, 5 * 3, d * 3, m).reshape(d, 3)
    assert np.array_equal(want[:3], draws.T)
    for col in (0, 1, 4, d - 1):                                        # raw secrets sit at 1, 4, d - 1
        last = int(secrets[col])
        for x in draws[col]:
            v = (last - int(x) + (1 << 63)) % (1 << 64) - (1 << 63)     # wrapping i64 subtraction
            last = _trem(v, m)
        assert last == want[3, col], col


def test_first_column_cases_cover_partial_blocks_at_both_ends():
    kinds = set()
    for n, f, w in FIRST_CASES:
        assert f + w <= FIRST_TOTAL
        lead, tail = f * (n - 1) % 8, (f + w) * (n - 1) % 8
        assert lead, (n, f)                                             # every slice starts inside a block
        kinds.add("both" if tail else "first only")
    assert kinds == {"both", "first only"}
    # the last block alone is partial wherever first_column = 0 and dimension * (n - 1) is no multiple of 8:
    # the kernel matrix's dimensions 1, T - 1, T + 1 and 2T + 5 at most share counts
    assert (T + 1) * 2 % 8 and (2 * T + 5) * 3 % 8
