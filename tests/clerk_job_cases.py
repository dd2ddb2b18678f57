"""The plan of tests/test_gpu_clerk_job.py as data, and a Python-integer model of the tiled clerk job
(sda_clerk_job_dev: fold tile after tile from the carried state, then zigzag-LEB128 the result).  No GPU, no
product import; tests/test_clerk_job_plan.py holds the tables and the model against the oracle on the CPU.

A case is (modulus, participations, dimension).  Its rows come from rows(): field moduli get shares in
(-m, m) -- they fit int32, so the slot path serves them and the payload takes the device-length encode -- and the
moduli past 2^31 get shares over all of (-m, m), which leave int32: the slot attempt is abandoned and the payload is
encoded with the host's length.  The first STEER columns are steered (steer()): their running state at every blob
boundary that a split can cut at walks through the edges of add_trem.  The columns behind them are witnesses
(witness()): one per boundary, on which a split that restarted from 0 or carried a canonicalised state ends
somewhere else.
"""
import functools

import numpy as np

I64_MAX = 2**63 - 1
M31 = 2147482801
FIELD_MODULI = (433, M31)
WIDE_MODULI = (2**62, 2**62 + 1, I64_MAX)          # both sides of SMALL_M (m <= 2^62), and the largest
MODULI = FIELD_MODULI + WIDE_MODULI
BLOBS = (1, 7, 8, 9, 17)                           # around the combine's unroll of 8

SLOT_TILE = 1024                                   # slot_combine_kernel at 4 columns per lane: 4 x 256
ENC_CHUNK = 2048                                   # codec_encode.hip: kEncChunk
REGION = 16384                                     # codec_decode.hip: kRegionBytes
# dim: (slot tiles it spans, encode chunks, whether a blob of 5-byte values crosses a region)
DIMS = {
    1:    (1, 1, False),     # one element
    1023: (1, 1, False),     # one short of a slot tile
    1024: (1, 1, False),     # a slot tile exactly
    1025: (2, 1, False),     # one into the second slot tile
    2047: (2, 1, False),     # one short of an encode chunk
    2048: (2, 1, False),     # an encode chunk (and two slot tiles) exactly
    2049: (3, 2, False),     # one into the second encode chunk
    3276: (4, 2, False),     # 16,380 bytes of 5-byte values: the last that stay inside one region
    3278: (4, 2, True),      # 16,390 bytes: past the region
    4097: (5, 3, True),      # one into the third encode chunk and the fifth slot tile
}
REGION_CROSS_FROM = 3277                           # 5 * 3277 = 16,385 > 16,384

STEER = 8                                          # steered columns per case (dim 1: the one column)


def splits(n):
    """The splits of n blobs into calls: one call, 1 | rest, rest | 1, and three tiles with a boundary inside a
    group of 8 (n >= 7).  Tiles are blob counts; a split of one blob is the one call."""
    out = [(n,)]
    if n >= 2:
        out += [(1, n - 1), (n - 1, 1)]
    three = {7: (3, 2, 2), 8: (3, 3, 2), 9: (3, 3, 3), 17: (5, 6, 6)}      # 17: a boundary at 11, inside 8..15
    if n in three:
        out.append(three[n])
    return out


def boundaries(n):
    """every blob index some split of n cuts at"""
    return sorted({sum(s[:i]) for s in splits(n) for i in range(1, len(s))})


def cases():
    """(m, n, dim): every dimension with every modulus, the participations rotating so that every count meets every
    modulus and every dimension."""
    out = []
    for di, dim in enumerate(DIMS):
        for mi, m in enumerate(MODULI):
            out.append((m, BLOBS[(di + mi) % len(BLOBS)], dim))
    return out


def case_id(c):
    m, n, dim = c
    name = {433: "m433", M31: "m31", 2**62: "m2p62", 2**62 + 1: "m2p62+1", I64_MAX: "mmax"}[m]
    return f"{name}-n{n}-d{dim}"


# ---------------------------------------------------------------- the model (Python integers)
def wrap(a):
    """i64 wrapping"""
    return (a + 2**63) % 2**64 - 2**63


def trem(a, m):
    """Rust's / C's `%`: the remainder takes the dividend's sign"""
    return a % m if a >= 0 else -((-a) % m)


def fold(state, rows, m):
    """combiner.rs:22-25 continued from `state` (a list of Python ints) over rows, in order"""
    for r in rows:
        state = [trem(wrap(s + int(v)), m) for s, v in zip(state, r)]
    return state


def zigzag_leb128(vals):
    out = bytearray()
    for v in vals:
        z = ((v << 1) ^ (v >> 63)) & (2**64 - 1)
        while z >= 0x80:
            out.append(0x80 | (z & 0x7F))
            z >>= 7
        out.append(z)
    return bytes(out)


def tiled_job(rows, split, m, carry=lambda s: s):
    """(state, payload) of the job over `rows` cut into the calls of `split`; carry() is applied to the state
    between calls (identity: the engine's contract)."""
    dim = len(rows[0]) if len(rows) else 0
    state, b = [0] * dim, 0
    for i, k in enumerate(split):
        if i:
            state = carry(state)
        state = fold(state, rows[b:b + k], m)
        b += k
    return state, zigzag_leb128(state)


def restart(_state):
    return [0] * len(_state)


def canonical(m):
    return lambda state: [s + m if s < 0 else s for s in state]


# ---------------------------------------------------------------- inputs
# The states a steered column is driven to, one per blob, as a cycle: the largest magnitude of either sign, 0 reached
# from a sum of exactly +m and of exactly -m (add_trem's equality edges), and the smallest magnitudes.  Column c
# starts the cycle at phase c, so from STEER >= 6 columns every state of the cycle is carried across every blob
# boundary, and the blob behind a boundary meets the +-m sums.  Every step keeps the share inside [-(m - 1), m - 1].
def targets(m):
    return [m - 1, 0, -(m - 1), 0, -1, 1]


def steer(x, m):
    """Rewrite the first STEER columns of x so that column c's state after blob b is targets(m)[(b + c) % 6]."""
    n, dim = x.shape
    t = targets(m)
    for c in range(min(STEER, dim)):
        s = 0
        for b in range(n):
            want = t[(b + c) % len(t)]
            if want == 0:                                   # by a sum of exactly +-m (from 0: stay)
                v = m - s if s > 0 else (-m - s if s < 0 else 0)
            else:
                v = want - s
            assert abs(v) <= m - 1, (m, b, c, s, want)
            x[b, c] = v
            s = trem(wrap(s + v), m)
            assert s == want
    return x


def steered_states(m, n, dim, boundary):
    """the states of the steered columns after `boundary` blobs"""
    t = targets(m)
    return [t[(boundary - 1 + c) % len(t)] for c in range(min(STEER, dim))]


# A carried state that was canonicalised (or dropped) only shows in the result if the two trajectories do not meet
# again, and over random signed shares they soon do.  So one witness column per boundary b keeps them apart: -2 from
# blob 0, nothing up to the boundary, -1 from every blob behind it -- the state stays negative and never wraps, and
# the job ends at -2 - (n - b), where a restart ends at -(n - b) and a canonicalised carry at m - 2 - (n - b).
def witness(x, m):
    n, dim = x.shape
    if dim < STEER + len(boundaries(n)):        # dim 1: the one column is a witness of every boundary, in steps
        x[:, 0] = -((m - 1) // 32)              # that 17 blobs do not carry to -m (and that leave int32 when m does)
        return x
    for i, b in enumerate(boundaries(n)):
        x[:, STEER + i] = 0
        x[0, STEER + i] = -2
        x[b:, STEER + i] = -1
    return x


@functools.lru_cache(maxsize=None)
def rows(m, n, dim):
    """[n][dim] int64 shares of case (m, n, dim): random over [-(m - 1), m - 1], the first STEER columns steered,
    the next ones the boundaries' witnesses (dim 1: the witness alone)"""
    rng = np.random.default_rng([m % 2**32, n, dim])
    x = rng.integers(-(m - 1), m - 1, size=(n, dim), dtype=np.int64, endpoint=True)
    return witness(steer(x, m), m)


def is_field(m):
    return m in FIELD_MODULI


def takes_slots(case):
    """Whether the case's one-call job stays on the slot path, which is what gives it the device-length encode.
    The field moduli do -- but for 433 at dim 4097: its shares take at most two bytes, blob 0 lies inside one 16 KiB
    region, and 4097 elements are one more than a region's 4096 slots, so the slot attempt raises its wide flag and
    the count pass takes over (as in sda_clerk_decode_combine_dev)."""
    m, _, dim = case
    return is_field(m) and not (m == 433 and dim == 4097)


LEAD = 16                                          # junk bytes in front of blob 0: offsets need not start at 0


def layout(blobs):
    """(bytes, offsets) of a job's device buffer: LEAD junk bytes, the blobs back to back, 32 bytes of padding"""
    off = np.concatenate([[LEAD], LEAD + np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    return bytes([0x80 | (i * 37 & 0x7F) for i in range(LEAD)]) + b"".join(blobs) + bytes(32), off
