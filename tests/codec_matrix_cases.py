"""The plan of tests/test_gpu_codec_matrix.py as data: every case with its inputs (a builder and its RNG seed), the
knobs it runs under and the sda_codec_last_launch record it must report, written out by the rule of the section
of the matrix it belongs to.  No GPU, no product import; the oracle encodes and decodes the payloads.

tests/test_codec_matrix_plan.py holds the plan against the bytes (tests/codec_dispatch.py recomputes every record
from the payloads and checks the edge each case is there for) and against the instantiations in the built library;
tests/test_gpu_codec_matrix.py runs it.

Sections: a slot combine, b fall-backs, c fused, d more than 65,535 blobs, e scan carries, f SDA_DEC_NT,
g the deterministic edge sweep.
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import codec_dispatch as CD

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
M31 = 2147482801
KNOBS = ("SDA_CODEC_PATH", "SDA_CODEC_NARROW", "SDA_CODEC_GROUP", "SDA_SLOT_CPL", "SDA_DC_DEPTH", "SDA_DEC_NT",
         "SDA_ENC_NT")                           # every knob the codec reads: a case runs with exactly its own set

SLOT_MODULI = (1, 2, 433, M31, 2**62, 2**62 + 1, I64_MAX)
SLOT_BLOBS = (1, 7, 8, 9, 17)                    # the 8-blob unroll and its tail
FUSED_DEPTHS = (2, 4, 8)
FUSED_BLOBS = (1, 2, 3, 5, 8, 9, 17)             # below, at and past every prefetch ring
FUSED_DIMS = (1, 1535, 1536, 1537, 3073)
MULTI_BLOBS = (1, 2, 3, 5)
BIG_BLOBS, BIG_DIM = 65_538, 5                   # section d: two grid slices, the second of 3 blobs
CARRY_BLOBS, CARRY_DIM = 3, 900_000              # section e: more than 256 regions per blob
SWEEP_DIM = 7000                                 # section g: 28,000..35,000 bytes per payload
EDGE_SPAN = 17


def slot_dims(cpl):
    return (1, 256 * cpl - 1, 256 * cpl, 256 * cpl + 1, 9000)


# ---------------------------------------------------------------- payload builders (cached: shared by the cases)
def _job(blobs, rows, lead=0):
    """(bytes with `lead` junk bytes in front and 32 of padding behind, offsets, decoded rows)"""
    off = np.concatenate([[lead], lead + np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    return bytes([0x80 | (i * 37 & 0x7F) for i in range(lead)]) + b"".join(blobs) + bytes(32), off, rows


def _encode_rows(x):
    return [O.varint_encode(r) for r in x]


@functools.lru_cache(maxsize=4)
def int32_rows(seed, n, dim, m):
    """section a: signed shares over all of int32 with -2^31, 2^31 - 1 and (where they fit) +-(m - 1) planted"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-(2**31), 2**31, size=(n, dim), dtype=np.int64)
    plants = [-(2**31), 2**31 - 1] + ([m - 1, -(m - 1)] if m - 1 < 2**31 else [])
    for i in range(n):                           # rotated by row, so that a dimension of 1 still gets them all
        for j in range(len(plants)):
            x[i, (i * 5 + 3 * j) % dim] = plants[(i + j) % len(plants)]
    return _job(_encode_rows(x), x)


@functools.lru_cache(maxsize=4)
def kind_rows(seed, kind, n, dim):
    """field: shares of the 31-bit field; onebyte: |v| < 64; wide: 10-byte elements"""
    rng = np.random.default_rng(seed)
    if kind == "field":
        x = rng.integers(-(M31 - 1), M31, size=(n, dim), dtype=np.int64)
    elif kind == "onebyte":
        x = rng.integers(-64, 64, size=(n, dim), dtype=np.int64)
    else:
        x = rng.choice(np.array([I64_MIN, I64_MAX, I64_MIN + 1, -(2**62) - 7, 2**63 - 9], np.int64), size=(n, dim))
    return _job(_encode_rows(x), x)


def mixed_values(rng, shape):
    """values of every encoded length 1..10"""
    bits = rng.integers(0, 64, size=shape)
    mag = rng.integers(0, 2**63, size=shape, dtype=np.uint64) >> (63 - bits).astype(np.uint64)
    v = mag.astype(np.int64)
    return np.where(rng.integers(0, 2, size=shape) == 1, v, -v - 1)


@functools.lru_cache(maxsize=8)
def fallback_job(name):
    """section b"""
    rng = np.random.default_rng(len(name) * 131 + ord(name[0]))
    n, dim = 5, 3001
    x = rng.integers(-(M31 - 1), M31, size=(n, dim), dtype=np.int64)
    if name == "six_bytes":
        x[3, 1700] = 2**35                       # zigzag 2^36: six bytes
    elif name in ("two31", "matrix_wide"):
        x[3, 1700] = 2**31                       # zigzag 2^32: five bytes, the fifth group 16
    elif name == "irregular":                    # blob 2 ends in a run of 12 continuation bytes
        blobs = _encode_rows(x)
        blobs[2] = O.varint_encode(x[2][:-2]) + bytes([0xFF] * 12 + [0x01])
        rows = np.stack([O.varint_decode(b) for b in blobs])
        assert rows.shape == (n, dim)
        return _job(blobs, rows)
    elif name in ("cap_4096", "cap_4097"):
        # 4-byte elements (zigzag in [2^21, 2^28)) fill every region of the region-aligned payloads to exactly
        # kSlotCap; cap_4097: payload 0's last region holds 4097 one-byte elements instead
        dim = 2 * 4096 + (1 if name == "cap_4097" else 0)
        mag = rng.integers(2**20, 2**27, size=(n, dim), dtype=np.int64)
        x = np.where(rng.integers(0, 2, size=(n, dim)) == 1, mag, -mag - 1)
        if name == "cap_4097":
            x[0, 4096:] = rng.integers(-64, 64, size=4097)
    return _job(_encode_rows(x), x)


@functools.lru_cache(maxsize=1)
def big_job():
    """section d: 65,538 payloads of 5 field shares"""
    x = np.random.default_rng(0xD).integers(-(M31 - 1), M31, size=(BIG_BLOBS, BIG_DIM), dtype=np.int64)
    return _job(_encode_rows(x), x)


@functools.lru_cache(maxsize=1)
def big_decode_job():
    """section d, sda_varint_decode_dev: the same payloads with blob 65,536 irregular and blob 65,537 one element
    longer.  rows: {blob: decoded values} for the first, last and slice-edge blobs and 64 random ones."""
    buf, off, x = big_job()
    blobs = [buf[off[i]:off[i + 1]] for i in range(BIG_BLOBS)]
    blobs[65_536] = O.varint_encode(x[65_536][:3]) + bytes([0xFF] * 12 + [0x01])
    blobs[65_537] = O.varint_encode(np.concatenate([x[65_537], [-(M31 - 1)]]))
    pick = sorted({0, 1, 65_533, 65_534, 65_535, 65_536, 65_537} |
                  set(np.random.default_rng(0xD1).integers(0, BIG_BLOBS, size=64).tolist()))
    buf2, off2, _ = _job(blobs, None)
    return buf2, off2, {b: O.varint_decode(blobs[b]) for b in pick}


@functools.lru_cache(maxsize=1)
def carry_job():
    """section e: 3 payloads of 900,000 field shares"""
    x = np.random.default_rng(0xE).integers(-(M31 - 1), M31, size=(CARRY_BLOBS, CARRY_DIM), dtype=np.int64)
    return _job(_encode_rows(x), x)


def bytes_from_lengths(rng, lengths, truncated=False):
    """random varints of the given byte lengths back to back; elements of <= 5 bytes hold int32 values (a fifth
    group of at most 15); truncated: the last element keeps its continuation bit"""
    lengths = np.asarray(lengths, dtype=np.int64)
    ends = np.cumsum(lengths) - 1
    b = rng.integers(0, 128, size=int(lengths.sum()), dtype=np.int64) | 0x80
    b[ends] &= 0x7F
    five = ends[lengths == 5]
    b[five] &= 0x0F
    if truncated:
        b[-1] |= 0x80
    return bytes(b.astype(np.uint8))


def _fill45(rng, total, n):
    """n lengths of 4 and 5 bytes summing to total, shuffled"""
    n5 = total - 4 * n
    assert 0 <= n5 <= n, (total, n)
    return rng.permutation(np.concatenate([np.full(n - n5, 4), np.full(n5, 5)]))


SWEEP_SPLITS = [(L, k) for L in (2, 3, 4, 5) for k in range(1, L)]


@functools.lru_cache(maxsize=1)
def sweep_job():
    """section g: SWEEP_DIM elements per payload, all of 4 and 5 bytes but one, so every payload decodes to the same
    count whatever its byte length in [4 D, 5 D].  Payload boundaries walk through every offset in -17..+17 of a
    16 KiB region edge, then of a 4 KiB sub-region edge that is no region edge; in every payload one element of L
    bytes straddles a region edge with k bytes before it, (L, k) taken in turn from SWEEP_SPLITS."""
    rng = np.random.default_rng(0x6)
    R = CD.REGION
    span = list(range(-EDGE_SPAN, EDGE_SPAN + 1)) + [-EDGE_SPAN]
    targets = [R * (1 + 2 * i) + d for i, d in enumerate(span)]
    base = R * (1 + 2 * (len(span) - 1)) + 7 * CD.SUB_REGION          # 28,672 bytes on: a sub-region edge
    targets += [base + 2 * R * i + d for i, d in enumerate(span)]
    blobs = []
    for j, (pos, end) in enumerate(zip(targets[:-1], targets[1:])):
        L, k = SWEEP_SPLITS[j % len(SWEEP_SPLITS)]
        E = (pos // R + 1) * R
        if E - pos < 64:
            E += R
        s1, s2 = E - k - pos, end - (E - k + L)
        n1 = min(max(round(s1 * (SWEEP_DIM - 1) / (s1 + s2)), -(-s1 // 5)), s1 // 4)
        lengths = np.concatenate([_fill45(rng, s1, n1), [L], _fill45(rng, s2, SWEEP_DIM - 1 - n1)])
        blobs.append(bytes_from_lengths(rng, lengths))
        assert len(blobs[-1]) == end - pos
    rows = np.stack([O.varint_decode(b) for b in blobs])
    return _job(blobs, rows, lead=targets[0])


LONG_SPLITS = [(L, k) for L in (10, 11) for k in range(1, L)]


@functools.lru_cache(maxsize=1)
def long_sweep_job():
    """section g, sda_varint_decode_dev: elements of 10 and 11 bytes straddling a region edge at every split (an
    11-byte element -- ten continuation bytes -- is the longest a regular blob holds), among elements of 1..10
    bytes, and one payload whose truncated tail ends exactly on a region edge.  rows: a list, one array per blob."""
    rng = np.random.default_rng(0x61)
    R = CD.REGION
    blobs, pos = [], 0
    for j, (L, k) in enumerate(LONG_SPLITS + [(3, 3)]):
        head = rng.integers(1, 11, size=400)
        E = ((pos + int(head.sum()) + 16) // R + 1) * R
        pad = E - k - pos - int(head.sum())                            # one-byte elements up to the split
        tail = rng.integers(1, 11, size=150) if L > 3 else []
        lengths = np.concatenate([head, np.ones(pad, np.int64), [L], tail]).astype(np.int64)
        blobs.append(bytes_from_lengths(rng, lengths, truncated=L == 3))  # (3, 3): three continuation bytes end at E
        pos += len(blobs[-1])
        if j == 7:                                                     # an empty blob among them
            blobs.append(b"")
    return _job(blobs, [O.varint_decode(b) for b in blobs])


def encode_values(seed, rows, length, stride):
    """section e: [rows][stride] values of 1..10 encoded bytes (the columns past `length` are never read)"""
    return mixed_values(np.random.default_rng(seed), (rows, stride))


BUILDERS = {"int32_rows": int32_rows, "kind_rows": kind_rows, "fallback_job": fallback_job, "big_job": big_job,
            "carry_job": carry_job, "sweep_job": sweep_job, "big_decode_job": big_decode_job,
            "long_sweep_job": long_sweep_job}


# ---------------------------------------------------------------- the cases
@dataclass(frozen=True)
class CombineCase:
    """one sda_clerk_decode_combine_dev call"""
    section: str
    name: str
    builder: str
    args: tuple
    m: int
    knobs: tuple               # ((name, value), ...): the whole environment of the codec's knobs
    record: tuple              # (path, width, fell_back, passes) sda_codec_last_launch must report

    @property
    def id(self):
        return f"{self.section}-{self.name}"

    def job(self):
        return BUILDERS[self.builder](*self.args)

    def env(self):
        return dict(self.knobs)


@dataclass(frozen=True)
class DecodeCase:
    """one sda_varint_decode_dev call"""
    section: str
    name: str
    builder: str
    knobs: tuple

    @property
    def id(self):
        return f"{self.section}-{self.name}"

    def job(self):
        return BUILDERS[self.builder]()

    def env(self):
        return dict(self.knobs)

    @property
    def kernel(self):
        return CD.decode_dev_kernel(self.env())


@dataclass(frozen=True)
class EncodeCase:
    """one sda_varint_encode_dev call"""
    name: str
    seed: int
    rows: int
    length: int
    stride: int
    knobs: tuple

    @property
    def id(self):
        return f"e-{self.name}"

    def env(self):
        return dict(self.knobs)

    @property
    def kernel(self):
        return CD.write_kernel(self.env())


def _k(**kw):
    return tuple(sorted((k, str(v)) for k, v in kw.items()))


def _combine_cases():
    C, out = CombineCase, []
    # a. slot combine: record SLOTS, width = CPL, nothing abandoned
    for cpl in (1, 2, 4):
        for m in SLOT_MODULI:
            for n in SLOT_BLOBS:
                for dim in slot_dims(cpl):
                    out.append(C("a", f"cpl{cpl}-m{m}-n{n}-d{dim}", "int32_rows", (cpl * 1000 + n, n, dim, m), m,
                                 _k(SDA_CODEC_PATH="slots", SDA_SLOT_CPL=cpl), (CD.SLOTS, cpl, 0, 1)))
    out.append(C("a", "no-knob", "int32_rows", (4017, 17, 9000, M31), M31, (), (CD.SLOTS, 4, 0, 1)))
    for cpl in (1, 2):
        for g, passes in ((1, 17), (3, 6)):
            out.append(C("a", f"group{g}-cpl{cpl}", "int32_rows", (cpl * 1000 + 17, 17, 9000, M31), M31,
                         _k(SDA_CODEC_PATH="slots", SDA_SLOT_CPL=cpl, SDA_CODEC_GROUP=g),
                         (CD.SLOTS_GROUPED, cpl, 0, passes)))
    # b. fall-backs made visible
    W, F, N, Q = CD.FB_SLOT_WIDE, CD.FB_FUSED_IRREGULAR, CD.FB_NARROW_WIDE, CD.FB_SEQUENTIAL
    for name, knobs, rec in (
            ("six_bytes", _k(SDA_CODEC_PATH="slots"), (CD.MATRIX64, 0, W | N, 1)),
            ("two31", _k(SDA_CODEC_PATH="slots"), (CD.MATRIX64, 0, W | N, 1)),
            ("cap_4097", _k(SDA_CODEC_PATH="slots"), (CD.MATRIX32, 0, W, 1)),
            ("cap_4096", _k(SDA_CODEC_PATH="slots"), (CD.SLOTS, 4, 0, 1)),
            ("irregular", _k(SDA_CODEC_PATH="fused"), (CD.MATRIX64, 0, F | Q, 1)),
            ("matrix_wide", _k(SDA_CODEC_PATH="matrix"), (CD.MATRIX64, 0, N, 1)),
            ("narrow0", _k(SDA_CODEC_NARROW=0), (CD.MATRIX64, 0, 0, 1))):
        out.append(C("b", name, "fallback_job", (name,), M31, knobs, rec))
    # c. fused: every prefetch depth below, at and past the number of blobs
    for depth in FUSED_DEPTHS:
        for n in FUSED_BLOBS:
            for dim in FUSED_DIMS:
                for kind in ("field", "onebyte"):
                    out.append(C("c", f"depth{depth}-{kind}-n{n}-d{dim}", "kind_rows", (300 + n, kind, n, dim), M31,
                                 _k(SDA_CODEC_PATH="fused", SDA_DC_DEPTH=depth), (CD.FUSED, depth, 0, 1)))
        for n in MULTI_BLOBS:
            for dim in FUSED_DIMS:
                out.append(C("c", f"depth{depth}-wide-n{n}-d{dim}", "kind_rows", (400 + n, "wide", n, dim), M31,
                             _k(SDA_CODEC_PATH="fused", SDA_DC_DEPTH=depth), (CD.FUSED_MULTI, 2, 0, 1)))
    # d. more than 65,535 blobs: two grid slices
    for name, knobs, rec in (
            ("slots", _k(SDA_CODEC_PATH="slots"), (CD.SLOTS, 4, 0, 2)),
            ("slots-group65535", _k(SDA_CODEC_PATH="slots", SDA_CODEC_GROUP=65535), (CD.SLOTS_GROUPED, 4, 0, 2)),
            ("matrix", _k(SDA_CODEC_PATH="matrix"), (CD.MATRIX32, 0, 0, 2)),
            ("fused", _k(SDA_CODEC_PATH="fused"), (CD.FUSED, 4, 0, 2))):
        out.append(C("d", name, "big_job", (), M31, knobs, rec))
    # e. more than 256 regions per blob; g. the edge sweep
    for sec, builder in (("e", "carry_job"), ("g", "sweep_job")):
        for name, rec in (("slots", (CD.SLOTS, 4, 0, 1)), ("matrix", (CD.MATRIX32, 0, 0, 1)),
                          ("fused", (CD.FUSED, 4, 0, 1))):
            out.append(C(sec, name, builder, (), M31, _k(SDA_CODEC_PATH=name), rec))
    # f. SDA_DEC_NT on the int32 matrix decode and on the slot decode
    for nt in (0, 1):
        out.append(C("f", f"matrix-nt{nt}", "kind_rows", (500, "field", 9, 5003), M31,
                     _k(SDA_CODEC_PATH="matrix", SDA_DEC_NT=nt), (CD.MATRIX32, 0, 0, 1)))
        out.append(C("f", f"slots-nt{nt}", "kind_rows", (500, "field", 9, 5003), M31,
                     _k(SDA_CODEC_PATH="slots", SDA_DEC_NT=nt), (CD.SLOTS, 4, 0, 1)))
    return out


COMBINE_CASES = _combine_cases()

DECODE_CASES = [DecodeCase("d", "decode", "big_decode_job", ()),
                DecodeCase("e", "decode", "carry_job", ()),
                DecodeCase("g", "decode-long", "long_sweep_job", ()),
                DecodeCase("f", "decode-nt0", "long_sweep_job", _k(SDA_DEC_NT=0)),
                DecodeCase("f", "decode-nt1", "long_sweep_job", _k(SDA_DEC_NT=1))]

ENC_LONG = 257 * CD.ENC_CHUNK + 5                # more than 256 chunks per row: varint_offsets_kernel's carry
ENCODE_CASES = [EncodeCase(f"{name}{'-nt0' if knobs else ''}", seed, rows, length, stride, knobs)
                for name, seed, rows, length, stride in (
                    ("300x40", 71, 300, 40, 40),                      # more than 256 rows: varint_rows_kernel's carry
                    ("1xlong", 72, 1, ENC_LONG, ENC_LONG),
                    # an odd stride puts row 1 eight bytes off a 16-byte boundary: it takes the scalar loads while
                    # row 0 takes the paired ones (len + 1 is even here, and would keep both rows aligned)
                    ("2xlong-odd-stride", 73, 2, ENC_LONG, ENC_LONG + 2))
                for knobs in ((), _k(SDA_ENC_NT=0))]


def combine_kernels(case):
    """the kernels CD.predict names for the case"""
    buf, off, _ = case.job()
    return CD.predict(CD.Job(np.frombuffer(buf, np.uint8), off), case.m, case.env())[1]
