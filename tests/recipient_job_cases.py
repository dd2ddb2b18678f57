"""The plan of tests/test_gpu_recipient_job.py as data: every case of the recipient job (sda_recipient_job,
sda_recipient_job_dev) with the opened payloads it runs on.  No GPU, no product import beyond the schemes.

The contract under test: the job returns what sda_recipient_reveal returns on the rows each blob decodes to.  So a
case is a recipient case in payload form -- the mask blobs and the (clerk index, blob) pairs -- and everything
expected of it is computed from the rows the ORACLE decodes from those blobs (rows()): the output by the big-integer
model (tests/pipeline_model.py), the status by the host form's checks restated in tests/pipeline_dispatch.py.

  derived   every RECIPIENT_CASES / RECIPIENT_ZERO / RECIPIENT_STATUS row of tests/pipeline_matrix_cases.py that has
            a host form (host_rows(case), each row encoded with the oracle).  Not expressible as blobs: the NULL rows
            (other arguments; FAULTS below has the job's own) and the `_dev`-only rows, whose subject is the row
            width argument the job does not have (a seed blob has the width it decodes to).
  cross     blobs of 3,277 five-byte values, which cross a 16,384-byte decode region: Additive clerk results and
            Full masks at D = 3,277, CONFIG_PACKED at dimension 8 * 3,277 + 1
  counts    Additive clerk counts 1, 7, 8, 9, 17 (the combine's unroll of 8) over D in (1, 255, 256, 257)
  packed    packed_dims(ss) with clerk results of exactly B values, of B + ragged extras, and one result short of B
  seeds     seed blobs of 0, 1, 4, 8 and 9 values; values >= 2^32 and negative (`as u32` truncates them); a blob with
            a run of 11 continuation bytes and one that ends inside a varint; 1, 255, 256 and 257 seeds
  late      the golden late-rejecting seed: the unmask runs twice
  faults    the engine's own argument checks (FAULTS): misaligned byte pointers, decreasing offsets, NULLs

A job's device buffers are laid out as tests/clerk_job_cases.layout lays a clerk job out: LEAD junk bytes, the blobs
back to back, padding.
"""
import functools
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from sda_amd import schemes as S
from tests import clerk_job_cases as CJ
from tests import pipeline_dispatch as PD
from tests import pipeline_matrix_cases as PC
from tests import pipeline_model as PM

P = PC.P
FL, CP = PC.FL, PC.CP
EXACT, CANONICAL = PD.EXACT, PD.CANONICAL
I64_MIN, I64_MAX = PD.I64_MIN, PD.I64_MAX
LEAD = CJ.LEAD
REGION = CJ.REGION
CROSS = CJ.REGION_CROSS_FROM                  # 3,277 five-byte values are 16,385 bytes
CLERK_COUNTS = CJ.BLOBS                       # 1, 7, 8, 9, 17
SEED_COUNTS = (1, 255, 256, 257)              # one lane per seed blob, 256 lanes per workgroup
SEED_LENS = (0, 1, 4, 8, 9)                   # values per seed blob: the key is the first 8, zero padded

# sda_recipient_job_last_launch
MASK_NONE, MASK_FULL_COMBINED, MASK_FULL_STREAMED, MASK_CHACHA, MASK_CHACHA_SPLIT = 0, 1, 2, 3, 4
SHARE_ADDITIVE, SHARE_PACKED = 1, 2

layout = CJ.layout


@dataclass(frozen=True)
class JobCase:
    group: str
    name: str
    ms: object
    ss: object
    dimension: int                            # the reconstructor's dimension (0 for Additive: it ignores it)
    m_out: int
    mode: int = EXACT
    out_slack: int = 0                        # out_cap = D + out_slack
    base: Optional[object] = None             # derived: the RecipientCase whose host rows these are
    mask_rows: Optional[Tuple[Tuple[int, ...], ...]] = None      # explicit rows, encoded with the oracle
    raw_mask_blobs: Optional[Tuple[bytes, ...]] = None           # or the blobs themselves (malformed seeds)
    share_rows: Optional[Tuple[Tuple[int, Tuple[int, ...]], ...]] = None
    tags: frozenset = field(default_factory=frozenset)

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    @property
    def packed(self):
        return PD.is_packed(self.ss)


def _rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


@functools.lru_cache(maxsize=None)
def blobs(case):
    """(mask blobs, [(clerk index, blob)]) of the case: its rows encoded by the oracle."""
    from oracle import oracle as O

    def enc(row):
        return O.varint_encode(np.asarray(row, np.int64)) if len(row) else b""

    if case.base is not None:
        masks, indexed = PC.host_rows(case.base)
    else:
        masks, indexed = case.mask_rows or (), case.share_rows or ()
    mask_blobs = list(case.raw_mask_blobs) if case.raw_mask_blobs is not None else [enc(r) for r in masks]
    return mask_blobs, [(i, enc(r)) for i, r in indexed]


@functools.lru_cache(maxsize=None)
def rows(case):
    """(mask rows, [(clerk index, row)]) as Python integer lists: what the ORACLE decodes from the case's blobs --
    the rows sda_recipient_reveal is called with in the contract."""
    from oracle import oracle as O
    mask_blobs, indexed = blobs(case)
    return ([[int(v) for v in O.varint_decode(b)] for b in mask_blobs],
            [(i, [int(v) for v in O.varint_decode(b)]) for i, b in indexed])


def out_len(case):
    """D of a successful call."""
    _, indexed = rows(case)
    if case.packed:
        return case.dimension
    return len(indexed[0][1]) if indexed else 0


def expected_status(case):
    """(status, message class) of the call, or None: sda_recipient_reveal's checks on the decoded rows."""
    masks, indexed = rows(case)
    st, _ = PD.recipient_host_status(case.ms, [len(r) for r in masks], case.ss, case.dimension,
                                     [len(r) for _, r in indexed], case.m_out, case.mode,
                                     out_len(case) + case.out_slack)
    return st


def expected_output(case):
    masks, indexed = rows(case)
    return PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, case.mode)


def expected_records(case, form, multi=False):
    """(sda_recipient_job_last_launch, sda_recipient_last_launch) of a successful call with a non-empty output."""
    masks, indexed = rows(case)
    return records(case.ms, len(masks), case.ss, case.dimension, [i for i, _ in indexed],
                   [len(r) for _, r in indexed], case.m_out, case.mode, form, multi=multi, late="late" in case.tags)


def records(ms, n_masks, ss, dimension, indices, lens, m_out, mode, form, multi=False, late=False):
    """expected_records from the call's shape alone: n_masks mask blobs, clerk results of `lens` values at clerk
    `indices`."""
    packed = PD.is_packed(ss)
    if isinstance(ms, S.NoMasking):
        route = MASK_NONE
    elif isinstance(ms, S.FullMasking):
        route = MASK_FULL_STREAMED if form == "host" else MASK_FULL_COMBINED
    else:
        route = MASK_CHACHA_SPLIT if multi and PD.multi_mask(ms, n_masks) else MASK_CHACHA
    job = (route, SHARE_PACKED if packed else SHARE_ADDITIVE, n_masks if isinstance(ms, S.ChaChaMasking) else 0)
    # the i64 rows of packed clerk results have the longest result's length: compacted unless that is B
    share_len = max(lens) if packed else (lens[0] if lens else 0)
    rec = PD.recipient_record(ms, ss, dimension, list(indices), share_len, m_out, mode,
                              late_resolve=late and route != MASK_CHACHA_SPLIT, multi_mask=route == MASK_CHACHA_SPLIT)
    return job, rec


# ---------------------------------------------------------------- derived cases
def _derived():
    out = []
    for c in PC.RECIPIENT_CASES + PC.RECIPIENT_ZERO + PC.RECIPIENT_STATUS:
        if "host" not in c.forms or c.null is not None:
            continue
        out.append(JobCase("derived", c.id, c.ms, c.ss, c.dimension, c.m_out, mode=c.mode, out_slack=c.out_slack,
                           base=c, tags=c.tags))
    return out


# ---------------------------------------------------------------- the shapes only payloads reach
def five_byte(rng, length, m, signed):
    """values of magnitude in [2^27, m): zigzag >= 2^28, five bytes each"""
    v = rng.integers(2**27, m, size=length, dtype=np.int64)
    if signed:
        v = v * rng.choice(np.asarray([-1, 1], np.int64), size=length)
    return tuple(int(x) for x in v)


def _seed_rows(rng, lens):
    return tuple(tuple(int(x) for x in rng.integers(0, 2**32, size=n, dtype=np.uint64)) for n in lens)


def _added():
    out = []
    J = JobCase
    full, chacha, none = S.FullMasking, S.ChaChaMasking, S.NoMasking()

    # ---- cross: a clerk result and a Full mask blob that cross a decode region
    rng = _rng("cross-add")
    out.append(J("cross", f"add2-full-D{CROSS}", full(P), S.Additive(2, P), 0, P,
                 mask_rows=tuple(five_byte(rng, CROSS, P, False) for _ in range(2)),
                 share_rows=tuple((i, five_byte(rng, CROSS, P, True)) for i in range(2))))
    rng = _rng("cross-cp")
    dim = CP.secret_count * CROSS + 1                    # B = 3,278
    B = PD.batches(CP, dim)
    out.append(J("cross", f"cp-full-D{dim}", full(P), CP, dim, P,
                 mask_rows=tuple(five_byte(rng, dim, P, False) for _ in range(2)),
                 share_rows=tuple((i, five_byte(rng, B, P, True)) for i in range(CP.reconstruction_threshold())),
                 tags=frozenset({"residue_only"})))

    # ---- counts: Additive clerk counts around the combine's unroll x the elementwise tail
    for i, n in enumerate(CLERK_COUNTS):
        D = PC.ELEMENTWISE_D[i % 4]
        rng = _rng(f"counts-{n}")
        ms = (none, full(P + 2), chacha(P, D, 128))[i % 3]
        if isinstance(ms, S.FullMasking):
            masks = tuple(tuple(PC.canonical(rng, D, P + 2, False)) for _ in range(3))
        else:
            masks = _seed_rows(rng, (4, 4)) if isinstance(ms, S.ChaChaMasking) else ()
        out.append(J("counts", f"add{n}-D{D}", ms, S.Additive(n, P), 0, P, mask_rows=masks,
                     share_rows=tuple((c, tuple(PC.canonical(rng, D, P, True))) for c in range(n))))

    # ---- packed: exactly B values, B + ragged extras, one result short of B
    for ss, tag in ((FL, "fl"), (CP, "cp")):
        p, r = ss.prime_modulus, ss.reconstruction_threshold()
        for i, L in enumerate(PC.packed_dims(ss)):
            B = PD.batches(ss, L)
            rng = _rng(f"packed-{tag}-{L}")
            base = [tuple(PC.canonical(rng, B, p, True)) for _ in range(r)]
            ms = (full(p), none, chacha(p + 2, L, 128))[i % 3]
            if isinstance(ms, S.FullMasking):
                masks = tuple(tuple(PC.canonical(rng, L, p, False)) for _ in range(2))
            else:
                masks = _seed_rows(rng, (4, 4)) if isinstance(ms, S.ChaChaMasking) else ()
            eq = isinstance(ms, S.NoMasking) or ms.modulus == p
            tags = frozenset({"residue_only"} if eq else ())
            out.append(J("packed", f"{tag}-B-D{L}", ms, ss, L, p, mask_rows=masks,
                         share_rows=tuple((c, row) for c, row in enumerate(base)), tags=tags))
            ragged = tuple((c, row + (11,) * ((c * 2 + 1) % 5)) for c, row in enumerate(base))
            out.append(J("packed", f"{tag}-B+ragged-D{L}", ms, ss, L, p, mask_rows=masks, share_rows=ragged, tags=tags))
            short = tuple((c, row[:B - 1] if c == r - 1 else row) for c, row in enumerate(base))
            out.append(J("packed", f"{tag}-short-D{L}", ms, ss, L, p, mask_rows=masks, share_rows=short, tags=tags))

    # ---- seeds
    add = S.Additive(2, P)

    def shares(rng, D):
        return tuple((c, tuple(PC.canonical(rng, D, P, True))) for c in range(2))

    rng = _rng("seeds-lens")
    out.append(J("seeds", "lens-0-1-4-8-9-D256", chacha(P, 256, 288), add, 0, P, mask_rows=_seed_rows(rng, SEED_LENS),
                 share_rows=shares(rng, 256)))
    # `as u32` truncates: values >= 2^32, negative ones, the ends of i64
    trunc = ((2**32 + 5, -1, -(2**31), I64_MAX), (I64_MIN, 2**32, -(2**32) - 7, 2**40 + 3, 1, 2, 3, 2**63 - 2**32))
    out.append(J("seeds", "truncated-values-D255", chacha(PC.CHACHA_FAST, 255, 256), add, 0, P, mask_rows=trunc,
                 share_rows=shares(rng, 255)))
    # malformed blobs: a run of 11 continuation bytes is one element; a blob ending inside a varint yields the
    # partial value
    long_run = bytes([0x81] * 11) + bytes([0x05, 0x8E, 0x02])
    cut = bytes([0x04, 0x06, 0x85])
    cut_long = bytes([0x02]) + bytes([0xFF] * 4)
    out.append(J("seeds", "malformed-D257", chacha(P, 257, 128), add, 0, P,
                 raw_mask_blobs=(long_run, cut, cut_long, bytes([0x80] * 23)), share_rows=shares(rng, 257)))
    for n in SEED_COUNTS:
        rng = _rng(f"seeds-n{n}")
        lens = tuple((4, 8, 1, 0, 9)[i % 5] for i in range(n))
        out.append(J("seeds", f"n{n}-fl-D4", chacha(433, 4, 128), FL, 4, 433, mask_rows=_seed_rows(rng, lens),
                     share_rows=tuple((c, tuple(PC.canonical(rng, 2, 433, True)))
                                      for c in range(FL.reconstruction_threshold())),
                     tags=frozenset({"residue_only"})))

    # ---- late: the mask's rejection is resolved after the reveal was queued
    rng = _rng("late")
    m = PC.CHACHA_FAST
    out.append(J("late", f"m{m}-add-D{PC.LATE_D}", chacha(m, PC.LATE_D, 128), S.Additive(2, m), 0, m,
                 mask_rows=(tuple(PC.LATE_SEED),),
                 share_rows=tuple((c, tuple(PC.canonical(rng, PC.LATE_D, m, True))) for c in range(2)),
                 tags=frozenset({"late"})))
    return out


DERIVED = _derived()
ADDED = _added()
CASES = DERIVED + ADDED


# ---------------------------------------------------------------- the engine's own argument checks
# (name, form, masking kind, the argument made faulty, message class).  Each runs on FAULT_CASE's payloads.
ALIGN, OFFSETS, NULL = "16-byte aligned", "non-decreasing", "NULL argument"
FAULTS = [
    ("align-clerk", "dev", "chacha", "clerk_bytes+8", ALIGN),
    ("align-seed", "dev", "chacha", "seed_bytes+8", ALIGN),
    ("offsets-clerk", "dev", "chacha", "clerk_off-decreasing", OFFSETS),
    ("offsets-seed", "dev", "chacha", "seed_off-decreasing", OFFSETS),
] + [(f"null-{a}", "dev", kind, a, NULL)
     for kind, args in (("chacha", ("ms", "ss", "out_len", "clerk_bytes", "clerk_off", "indices", "seed_bytes",
                                    "seed_off")), ("full", ("mask",)))
     for a in args] + \
    [(f"null-{a}", "host", "chacha", a, NULL)
     for a in ("ms", "ss", "out_len", "mask_blobs", "mask_lens", "clerk_blobs", "clerk_lens", "indices", "mask_blob_0",
               "clerk_blob_1")]


def fault_case(kind):
    rng = _rng("fault-" + kind)
    D = 9
    if kind == "full":
        ms, masks = S.FullMasking(433), tuple(tuple(PC.canonical(rng, D, 433, False)) for _ in range(2))
    else:
        ms, masks = S.ChaChaMasking(433, D, 128), _seed_rows(rng, (4, 4, 4))
    return JobCase("faults", kind, ms, S.Additive(2, 433), 0, 433, mask_rows=masks,
                   share_rows=tuple((c, tuple(PC.canonical(rng, D, 433, True))) for c in range(2)))
