"""CPU model of the engine's device-side draws (include/sda_engine.h, sda_draws_dev), in Python integers over
oracle.chacha20_core -- the function tests/test_oracle_golden.py pins to RFC 7539.

Element i (an absolute 64-bit index), retry round r = 0, 1, ...:
    state = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, key[0..7],
             (i >> 3) & 0xFFFFFFFF, (i >> 3) >> 32, stream_id, r]
    o = chacha20_core(state);  j = i & 7;  v = (o[2j] << 32) | o[2j + 1]      (high word first)
    zone = (2^64 - 1) - ((2^64 - 1) mod bound)
    v < zone: the draw is v mod bound; otherwise round r + 1, same block counter and position;
    at r = 63 the draw is v mod bound unconditionally.
"""
import functools
import json
import os

import numpy as np

from oracle import oracle as O

# Shared by the draws tests: a fixed key, and the two bounds whose reject rates (about 1/3 and 1/4) make the retry
# path unavoidable -- tests/test_draws_model.py checks that condition on (TEST_KEY, TEST_STREAM, these bounds).
TEST_KEY = (0x03020100, 0x07060504, 0x0B0A0908, 0x0F0E0D0C, 0x13121110, 0x17161514, 0x1B1A1918, 0x1F1E1D1C)
TEST_STREAM = 0x5DA
BOUND_THIRD = 6148914691236517206          # floor(2^64 / 3) + 1: zone = 2 * bound
BOUND_QUARTER = (1 << 62) + 1

CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
LAST_ROUND = 63
U64_MAX = (1 << 64) - 1


@functools.lru_cache(maxsize=1 << 16)
def _block(key, stream_id, counter, r):
    state = list(CONSTANTS) + list(key) + [counter & 0xFFFFFFFF, counter >> 32, stream_id, r]
    return tuple(int(w) for w in O.chacha20_core(np.array(state, dtype=np.uint32)))


def draw(key, stream_id, i, bound):
    """(value, round it was taken at) of element i."""
    key = tuple(int(w) for w in key)
    zone = U64_MAX - U64_MAX % bound
    j = i & 7
    for r in range(LAST_ROUND + 1):
        o = _block(key, stream_id, i >> 3, r)
        v = (o[2 * j] << 32) | o[2 * j + 1]
        if v < zone or r == LAST_ROUND:
            return v % bound, r
    raise AssertionError("unreachable")


def draws_with_rounds(key, stream_id, first, count, bound):
    pairs = [draw(key, stream_id, first + p, bound) for p in range(count)]
    vals = np.array([v for v, _ in pairs], dtype=np.int64).reshape(count)      # bound <= 2^63 - 1: every value fits
    return vals, np.array([r for _, r in pairs], dtype=np.int64).reshape(count)


def draws(key, stream_id, first, count, bound):
    """out[p] = draw(first + p), p < count, as int64."""
    return draws_with_rounds(key, stream_id, first, count, bound)[0]


def rfc_coordinates():
    """(name, key, stream_id, first, the eight expected draws at bound 2^32) of both RFC 7539 blocks."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chacha_rfc7539.json")
    g = json.load(open(golden))["rfc7539"]
    out = []
    for name in sorted(g):
        state, o = g[name]["state"], g[name]["out"]
        assert state[15] == 0                                   # the rule's round word at r = 0
        assert all(o[2 * j] != 0xFFFFFFFF for j in range(8))    # nothing is rejected at bound 2^32
        out.append((name, tuple(state[4:12]), state[14], 8 * (state[12] | state[13] << 32),
                    [o[2 * j + 1] for j in range(8)]))
    return out
