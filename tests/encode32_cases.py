"""The case plan of tests/test_gpu_encode32.py (sda_varint_encode32_dev), built on the CPU: shapes, values, and
the expected payload from oracle.varint_encode of the widened rows.  tests/test_encode32_plan.py holds the plan
against the source (the chunk size) and checks on the CPU what each case is meant to contain.

Values: for byte-size class s = 1..5 the zigzag z is uniform in [2^(7(s-1)), 2^(7s) - 1] (class 1 from 0, class 5 to
2^32 - 1) and v = (z >> 1) ^ -(z & 1) as int32.  A mixed row draws the class per element, and has planted in it
0, -1, INT32_MIN, INT32_MAX, both neighbours of every class boundary, and a 5-byte element followed by a 1-byte
element straddling every chunk boundary of the first three chunks (where the row is long enough).
"""
import functools
from dataclasses import dataclass

import numpy as np

ENC32_CHUNK = 2048         # sda_amd/csrc/codec_encode.hip: SDA_ENC32_CHUNK (kEnc32Chunk), elements per int32 encode block
C = ENC32_CHUNK

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
PAD = 0x5EA7C0DE               # the columns past len: a 5-byte element whose bytes no payload holds (check_classes)
POISON = 0xA5                  # dst before the call
CHAIN_M = 2147482801


def unzigzag(z):
    z = np.asarray(z, dtype=np.uint64)
    return ((z >> np.uint64(1)).astype(np.int64) ^ -(z & np.uint64(1)).astype(np.int64)).astype(np.int32)


def class_bounds(s):
    return (0 if s == 1 else 1 << (7 * (s - 1))), ((1 << 32) - 1 if s == 5 else (1 << (7 * s)) - 1)


def class_values(rng, s, size):
    lo, hi = class_bounds(s)
    return unzigzag(rng.integers(lo, hi + 1, size=size, dtype=np.uint64))


def planted():
    """(value, byte size) of the planted elements, in order."""
    out = [(0, 1), (-1, 1), (INT32_MIN, 5), (INT32_MAX, 5)]
    for s in range(1, 5):              # the last zigzag of class s and the first of class s + 1
        out += [(int(unzigzag((1 << (7 * s)) - 1)), s), (int(unzigzag(1 << (7 * s))), s + 1)]
    return out


def mixed_row(rng, length):
    cls = rng.integers(1, 6, size=length)
    row = np.empty(length, np.int32)
    for s in range(1, 6):
        sel = cls == s
        row[sel] = class_values(rng, s, int(sel.sum()))
    pl = [v for v, _ in planted()]
    if length > len(pl) + 1:
        row[1:1 + len(pl)] = pl
    for c in range(1, 4):              # ... [5 bytes] | chunk boundary | [1 byte] ...
        if c * C < length:
            row[c * C - 1] = INT32_MIN + c
            row[c * C] = c
    return row


@dataclass(frozen=True)
class EncCase:
    name: str
    rows: int
    length: int
    stride: int
    vals_off: int = 0          # int32 elements between a 16-byte boundary and vals
    dst_off: int = 0           # bytes between a 16-byte boundary and dst
    nt0: bool = False          # SDA_ENC_NT=0
    kind: str = "mixed"        # "extremes": row 0 all class 5, row 1 all class 1
    classes: tuple = (1, 2, 3, 4, 5)

    @property
    def id(self):
        return self.name


L3 = 3 * C + 5
S3 = L3 + 4 + (1 - (L3 + 4)) % 4          # stride = 1 (mod 4), >= len: rows 0, 4, 8, 12 bytes off
CASE3 = EncCase("3-four-row-alignments", 4, L3, S3)
CASE2 = EncCase("2-offsets-scan-carry", 1, 257 * C + 5, 257 * C + 5)
CASES = [
    EncCase("1-row-scan-carry", 300, 40, 40),
    CASE2,
    CASE3,
    EncCase("3-vals-4-off", 4, L3, S3, vals_off=1),
    EncCase("4-extremes", 2, 2 * C, 2 * C, kind="extremes", classes=(1, 5)),
    EncCase("5-dst-5-off", 4, L3, S3, dst_off=5),
    EncCase("5-dst-15-off", 4, L3, S3, dst_off=15),
    EncCase("6-case2-nt0", 1, 257 * C + 5, 257 * C + 5, nt0=True),
    EncCase("6-case3-nt0", 4, L3, S3, nt0=True),
]
CHAIN = (64, 2 * C + 7)


@functools.lru_cache(maxsize=None)
def values(rows, length, stride, kind="mixed"):
    """[rows][stride] int32, PAD in the columns past `length`; one array per shape, shared by the cases."""
    rng = np.random.default_rng([0xE32, rows, length])
    v = np.full((rows, stride), PAD, np.int32)
    if kind == "extremes":
        v[0, :length] = class_values(rng, 5, length)
        v[1, :length] = class_values(rng, 1, length)
    else:
        for r in range(rows):
            v[r, :length] = mixed_row(rng, length)
    v.setflags(write=False)
    return v


def case_values(case):
    return values(case.rows, case.length, case.stride, case.kind)


@functools.lru_cache(maxsize=None)
def expected(rows, length, stride, kind="mixed"):
    """(payload bytes, row_bytes) from oracle.varint_encode of each widened row."""
    from oracle import oracle as O
    v = values(rows, length, stride, kind)
    blobs = [O.varint_encode(np.ascontiguousarray(v[r, :length]).astype(np.int64)) for r in range(rows)]
    return b"".join(blobs), np.array([len(b) for b in blobs], np.uint64)


def case_expected(case):
    return expected(case.rows, case.length, case.stride, case.kind)


def element_sizes(payload):
    """Byte size of every element of a LEB128 stream (every element here ends in a terminator byte)."""
    b = np.frombuffer(payload, np.uint8)
    ends = np.flatnonzero((b & 0x80) == 0)
    return np.diff(np.concatenate([[-1], ends]))


def pad_bytes():
    from oracle import oracle as O
    return O.varint_encode(np.array([PAD], np.int64))


def check_classes(case, payload):
    """What every case asserts on the oracle's output before it compares: the byte-size classes it is meant to hold
    all occur (all five; classes 1 and 5 alone for the extremes case), and the padding's bytes do not."""
    got = tuple(sorted(set(element_sizes(payload).tolist())))
    assert got == case.classes, (case.name, got)
    assert pad_bytes() not in payload, case.name


PARTICIPANT_D = 4099        # tests/test_gpu_participant32.py: odd, so the last batch is ragged


@functools.lru_cache(maxsize=None)
def participant_schemes():
    """The schemes of tests/test_gpu_participant32.py by the share-gen route they take at PARTICIPANT_D in BOTH modes
    (tests/test_encode32_plan.py asserts it through tests/packed_dispatch.py): CONFIG_PACKED on the direct int32
    kernels; an n + 1 = 81 scheme with k + t + 1 < 16, which stays on the register kernels at any B, so the int32
    call writes i64 into scratch and narrows; an n + 1 = 243 scheme on the workspace kernels.  The last two come
    from tests/packed_matrix_cases.py."""
    from sda_amd import schemes as S
    from tests import packed_matrix_cases as PM

    def pick(cases, k, t, n):
        return next(c.sch for c in cases
                    if (c.sch.secret_count, c.sch.privacy_threshold(), c.sch.share_count) == (k, t, n))

    # (5, 2, 80): the plan's prime below 2^24 (no lazy truncation); (5, 2, 242): its prime below 2^31
    return {"packed": S.CONFIG_PACKED, "n80-scratch": pick(PM.GEN_CASES, 5, 2, 80),
            "n242-workspace": pick(PM.REVEAL_CASES, 5, 2, 242)}


@functools.lru_cache(maxsize=None)
def chain_values():
    rows, length = CHAIN
    v = np.random.default_rng(0xC4A1).integers(-(CHAIN_M - 1), CHAIN_M, size=(rows, length), dtype=np.int64)
    v.setflags(write=False)
    return v
