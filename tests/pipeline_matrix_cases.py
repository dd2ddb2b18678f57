"""The plan of tests/test_gpu_pipeline_matrix.py as data: every case of the two role pipelines
(sda_amd/csrc/engine_recipient.cpp, engine_participant.cpp) with the inputs it runs on.  No GPU, no product import
beyond the schemes.

tests/test_pipeline_matrix_plan.py holds the tables against tests/pipeline_dispatch.py (every decision value is taken
by a case), against the model and the oracle (tests/pipeline_model.py, tests/oracle_backend.py) and against what each
case's tags promise; tests/test_gpu_pipeline_matrix.py runs them.

A case is a small frozen record.  Its inputs are generated from its id (a CRC of the id seeds the generator), and
are steered: Full-mask rows, Additive clerk rows and participant secrets marked "raw" carry I64_MIN, I64_MAX, +-m,
+-(m - 1) and 0 at fixed positions (rotated by the id where the dimension cannot hold them all), and a "wrap" case
plants a pair whose wrapping difference (recipient: masked - mask) or sum (participant: secret + mask) leaves i64.

Tags:  representative  "representative matters": the canonical and the exact reveal give different outputs
       residue_only    the pipeline substitutes the canonical reveal for the EXACT request
       wrap            an element's masked - mask or secret + mask leaves the i64 range before wrapping
       zero_rows       ChaCha masking with no participation (the mask is `dimension` zeros for any modulus)
       late            a golden rejecting seed: the mask is resolved late and the step after it redone
"""
import functools
import json
import os
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from sda_amd import schemes as S
from tests import draws_model as DM
from tests import pipeline_dispatch as PD
from tests.combine_matrix_cases import BIG_MODULI, P, SMALL_MODULI

I64_MIN, I64_MAX = PD.I64_MIN, PD.I64_MAX
EXACT, CANONICAL = PD.EXACT, PD.CANONICAL
GUARD = 16                                    # guard words before and after every device output
POISON = 0x5A5A5A5A5A5A5A5A
POISON32 = 0x5A5A5A5A
POISON8 = 0xA5

MODULI = SMALL_MODULI + BIG_MODULI            # 1, 2, 433, P, 2^31 - 1, 2^40 + 7, 2^62 | 2^62 + 1, 2^63 - 25, 2^63 - 1
NEGATIVE_MODULI = (-P, -(2**62 + 1))          # recipient side only: Rust's `%` ignores the divisor's sign
# ChaCha masking moduli, named as tests/test_gpu_chacha_matrix.py classifies them (the plan test checks it)
CHACHA_FAST = 68719676673                     # BARRETT, a fast-path modulus with golden rejecting seeds
CHACHA_HIGH_REJECTION = 2**40 + 7             # 2^40 rejected values: the stream path
CHACHA_ABOVE_2_62 = 2**62 + 1                 # wrapping signed sums: the stream path
ELEMENTWISE_D = (1, 255, 256, 257)            # 256 lanes per workgroup; 257: two workgroups, a one-lane tail
KEY = DM.TEST_KEY
STREAM = DM.TEST_STREAM

FL, CP = S.FULL_LOOP_PACKED, S.CONFIG_PACKED


def wide_scheme():
    """One workspace-kernel scheme (n + 1 = 243) of tests/packed_matrix_cases.py."""
    from tests import encode32_cases as EC
    return EC.participant_schemes()["n242-workspace"]


def packed_dims(ss):
    k = ss.secret_count
    return (1, k - 1, k, k + 1, 8 * k + 5)     # one batch, ragged, full, two batches, several + ragged tail


def _rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def specials(m):
    m = abs(m)
    return [I64_MIN, I64_MAX, m, -m, m - 1, -(m - 1), 0]


def steered(rng, length, m, rot):
    """`length` values over all of i64 with the specials of m at the front (rotated by `rot` so that a dimension
    of 1 still meets each of them over the cases) and again at the tail."""
    v = [int(x) for x in rng.integers(I64_MIN, I64_MAX, size=length, dtype=np.int64, endpoint=True)]
    sp = specials(m)
    sp = sp[rot % len(sp):] + sp[:rot % len(sp)]
    for i, x in enumerate(sp[:length]):
        v[i] = x
    if length >= 2 * len(sp):
        v[length - len(sp):] = sp
    return v


def canonical(rng, length, m, signed):
    m = abs(m) or 433                         # a status row's modulus 0: any values do
    lo = -(m - 1) if signed else 0
    if m - 1 > I64_MAX - 1:
        return [int(x) for x in rng.integers(lo, I64_MAX, size=length, dtype=np.int64, endpoint=True)]
    return [int(x) for x in rng.integers(lo, m, size=length, dtype=np.int64)]


# ================================================================ recipient
@dataclass(frozen=True)
class RecipientCase:
    group: str
    name: str
    ms: object
    ss: object
    length: int                               # Additive: the clerk rows' length; PackedShamir: the dimension
    subset: Tuple[int, ...]                   # clerk indices, in call order
    m_out: int
    mode: int = EXACT
    n_masks: int = 2
    seed_words: int = 4                       # ChaCha: words per seed row
    raw: bool = False                         # Full-mask rows / Additive clerk rows over all of i64, steered
    share_extra: int = 0                      # the clerk rows are this much longer than the batch count
    out_slack: int = 0                        # out_cap = D + out_slack
    forms: Tuple[str, ...] = ("host", "dev")
    host_mask_lens: Optional[Tuple[int, ...]] = None      # host form only: ragged seed rows
    host_share_extra: Optional[Tuple[int, ...]] = None    # host form only: ragged clerk rows (extra per row)
    tags: frozenset = field(default_factory=frozenset)
    # status rows only
    null: Optional[str] = None                # the argument passed as NULL
    mask_width: Optional[int] = None          # overrides the mask rows' width (Full: != D, None: > 0, ChaCha: 0 / 9)
    row_lens: Optional[Tuple[int, ...]] = None            # overrides every clerk row's length

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    @property
    def packed(self):
        return PD.is_packed(self.ss)

    @property
    def dimension(self):
        return self.length if self.packed else 0           # the Additive reconstructor ignores its dimension

    @property
    def base_len(self):
        return PD.batches(self.ss, self.length) if self.packed else self.length

    @property
    def share_len(self):
        return self.base_len + self.share_extra

    @property
    def D(self):
        """The output length of a successful call."""
        return self.length if self.packed else (self.share_len if self.subset else 0)


@functools.lru_cache(maxsize=None)
def recipient_inputs(case):
    """(mask rows, [(clerk index, row)]) as Python integer lists, for the `_dev` form's uniform rows; the host form's
    ragged variants are cut from / padded onto these by host_rows()."""
    rng = _rng(case.id)
    rot = zlib.crc32(case.id.encode()) >> 8
    ms, ss = case.ms, case.ss
    # clerk rows
    if case.packed:
        p = ss.prime_modulus
        rows = {c: canonical(rng, case.share_len, p, signed=True) for c in sorted(set(case.subset))}
    else:
        m = ss.modulus
        rows = {c: (steered(rng, case.share_len, m, rot + c) if case.raw else canonical(rng, case.share_len, m, True))
                for c in sorted(set(case.subset))}
    if case.row_lens is not None:
        rows = {c: rows[c][:n] + [1] * max(0, n - len(rows[c]))
                for c, n in zip(sorted(set(case.subset)), case.row_lens)}
    # mask rows
    if isinstance(ms, S.NoMasking):
        w = case.mask_width or 0
        masks = [[7] * w for _ in range(case.n_masks)]
    elif isinstance(ms, S.FullMasking):
        w = case.D if case.mask_width is None else case.mask_width
        q = ms.modulus if ms.modulus not in (0, I64_MIN) else P
        masks = [(steered(rng, w, q, rot + 3 + i) if case.raw else canonical(rng, w, q, False))
                 for i in range(case.n_masks)]
    else:
        w = case.seed_words if case.mask_width is None else case.mask_width
        if "late" in case.tags:
            masks = [list(LATE_SEED)[:w] for _ in range(case.n_masks)]
        else:
            masks = [[int(x) for x in rng.integers(0, 2**32, size=w, dtype=np.uint64)] for _ in range(case.n_masks)]
    if "wrap" in case.tags:
        # masked[0] = m - 1 (the first clerk row alone carries it) and mask[0] = -(q - 1): the difference is
        # m + q - 2 >= 2^63 for both moduli above 2^62
        m, q = abs(ss.modulus), abs(ms.modulus)
        for i, c in enumerate(sorted(set(case.subset))):
            rows[c][0] = m - 1 if i == 0 else 0
        for i, r in enumerate(masks):
            r[0] = -(q - 1) if i == 0 else 0
    return masks, [(c, rows[c]) for c in case.subset]


def host_rows(case):
    """The host form's rows: ragged where the case says so (seed rows cut or zero-extended, clerk rows extended)."""
    masks, indexed = recipient_inputs(case)
    if case.host_mask_lens is not None:
        rng = _rng(case.id + "/host")
        masks = [r[:n] + [int(x) for x in rng.integers(0, 2**32, size=max(0, n - len(r)), dtype=np.uint64)]
                 for r, n in zip(masks, case.host_mask_lens)]
    if case.host_share_extra is not None:
        indexed = [(c, r + [11] * e) for (c, r), e in zip(indexed, case.host_share_extra)]
    return masks, indexed


def _threshold(ss):
    return tuple(range(ss.reconstruction_threshold()))


def _all(ss):
    return tuple(range(ss.share_count))


def _recipient_cases():
    out = []
    R = RecipientCase
    full, chacha, none = S.FullMasking, S.ChaChaMasking, S.NoMasking()

    # ---- kinds: masking kind x sharing kind x equal / different moduli x mode
    for si, ss in enumerate((S.Additive(3, P), FL, CP)):
        p = ss.modulus
        dims = packed_dims(ss) if PD.is_packed(ss) else ELEMENTWISE_D
        modes = (EXACT, CANONICAL) if PD.is_packed(ss) else (EXACT,)
        subset = _threshold(ss)
        i = 0
        for kind in ("none", "full", "chacha"):
            for equal in (True, False):
                if kind == "none" and not equal:
                    continue
                for mode in modes:
                    L = dims[i % len(dims)]
                    i += 1
                    q = p if equal else p + 2
                    D = L
                    ms = none if kind == "none" else full(q) if kind == "full" else chacha(q, D, 128)
                    tags = set()
                    if PD.is_packed(ss) and mode == EXACT and equal:
                        tags.add("residue_only")
                    elif PD.is_packed(ss) and mode == EXACT and L >= 8:    # a few elements may all be non-negative
                        tags.add("representative")
                    out.append(R("kinds", f"{kind}-{'add' if si == 0 else 'fl' if si == 1 else 'cp'}-"
                                 f"{'eq' if equal else 'ne'}-{'canon' if mode else 'exact'}-D{L}", ms, ss, L, subset, p,
                                 mode=mode, n_masks=0 if kind == "none" else 2, tags=frozenset(tags)))

    # ---- moduli: Additive n in {1, 2, 3} x every sharing modulus, raw i64 clerk rows, a Full mask of another
    # modulus (negative ones included), output moduli in turn
    qs = MODULI + NEGATIVE_MODULI
    for i, m in enumerate(MODULI + NEGATIVE_MODULI):
        n = 1 + i % 3
        q = qs[(i + 5) % len(qs)]
        L = ELEMENTWISE_D[i % 4]
        m_out = (abs(m), abs(m) + 2, 2**40, 0, -abs(m), I64_MAX)[i % 6]
        out.append(R("moduli", f"add{n}-m{m}-full-q{q}-out{m_out}-D{L}", full(q), S.Additive(n, m), L,
                     tuple(range(n)), m_out, raw=True, n_masks=1 + i % 2))
    # no mask: the unmask is skipped, positive() still runs on raw combine results
    for i, m in enumerate((1, 2, 2**62, I64_MAX)):
        out.append(R("moduli", f"add2-m{m}-none-out{-m}-D{ELEMENTWISE_D[i]}", none, S.Additive(2, m),
                     ELEMENTWISE_D[i], (0, 1), -m, raw=True, n_masks=0))

    # ---- wrap: masked - mask leaves i64 (both moduli above 2^62)
    for i, (m, q) in enumerate(((2**62 + 1, I64_MAX), (I64_MAX, -(2**62 + 1)), (2**63 - 25, 2**63 - 25))):
        out.append(R("wrap", f"add2-m{m}-full-q{q}-D{ELEMENTWISE_D[1 + i]}", full(q), S.Additive(2, m),
                     ELEMENTWISE_D[1 + i], (0, 1), (I64_MAX, 0, m)[i], raw=True, tags=frozenset({"wrap"})))

    # ---- nmasks: 0, 1, 5 participations
    for nm in (1, 5):
        out.append(R("nmasks", f"full-{nm}-add-D257", full(433), S.Additive(3, 433), 257, (0, 1, 2), 433, n_masks=nm))
        out.append(R("nmasks", f"full-{nm}-cp-D69", full(P), CP, 69, _threshold(CP), P, n_masks=nm,
                     tags=frozenset({"residue_only"})))
    for nm in (0, 1, 5):
        out.append(R("nmasks", f"chacha-{nm}-add-D256", chacha(P, 256, 128), S.Additive(2, P), 256, (0, 1), P,
                     n_masks=nm, tags=frozenset({"zero_rows"} if nm == 0 else ())))
        out.append(R("nmasks", f"chacha-{nm}-fl-D4", chacha(433, 4, 128), FL, 4, _threshold(FL), 433, n_masks=nm,
                     tags=frozenset({"residue_only"} | ({"zero_rows"} if nm == 0 else set()))))
    # no participation and a negative (or, for Full, any) modulus: chacha.rs:58 returns the zeros untouched
    out.append(R("nmasks", "chacha-0-negative-add-D257", chacha(-P, 257, 128), S.Additive(2, P), 257, (0, 1), P,
                 n_masks=0, tags=frozenset({"zero_rows"})))
    out.append(R("nmasks", "chacha-0-negative-cp-D9", chacha(-P, 9, 128), CP, 9, _threshold(CP), P, n_masks=0,
                 tags=frozenset({"zero_rows", "residue_only"})))
    out.append(R("nmasks", "chacha-0-negbig-add-D1", chacha(-(2**62 + 1), 1, 128), S.Additive(1, 433), 1, (0,), 433,
                 n_masks=0, raw=True, tags=frozenset({"zero_rows"})))

    # ---- seeds: 1, 4, 8 words on both forms; ragged rows and rows past 8 words on the host form
    for w in (1, 4, 8):
        out.append(R("seeds", f"w{w}-add-D255", chacha(P, 255, 32 * w), S.Additive(2, P), 255, (1, 0), P, n_masks=3,
                     seed_words=w))
    out.append(R("seeds", "host-ragged-add-D256", chacha(433, 256, 128), S.Additive(2, 433), 256, (0, 1), 433,
                 n_masks=4, seed_words=8, forms=("host",), host_mask_lens=(0, 3, 8, 5)))
    out.append(R("seeds", "host-long-add-D257", chacha(P, 257, 384), S.Additive(2, P), 257, (0, 1), P, n_masks=3,
                 seed_words=8, forms=("host",), host_mask_lens=(12, 9, 8)))
    out.append(R("seeds", "host-long-fl-D5", chacha(433, 5, 384), FL, 5, _threshold(FL), 433, n_masks=2,
                 seed_words=8, forms=("host",), host_mask_lens=(9, 2), tags=frozenset({"residue_only"})))

    # ---- subsets: exactly the threshold, all, reversed, one duplicate index
    for ss, tag in ((FL, "fl"), (CP, "cp")):
        p, n, r = ss.prime_modulus, ss.share_count, ss.reconstruction_threshold()
        L = packed_dims(ss)[4]
        subsets = {"threshold": _threshold(ss), "all": _all(ss), "reversed": tuple(reversed(_all(ss))),
                   "tail": tuple(range(n - r, n)), "duplicate": _threshold(ss) + (2,)}
        for name, sub in subsets.items():
            out.append(R("subsets", f"{tag}-{name}-eq", full(p), ss, L, sub, p, tags=frozenset({"residue_only"})))
            # (a canonical reveal of repeated points does not exist: nothing to compare that case with)
            out.append(R("subsets", f"{tag}-{name}-ne", full(p + 2), ss, L, sub, p,
                         tags=frozenset(() if name == "duplicate" else {"representative"})))
        out.append(R("subsets", f"{tag}-duplicate-none", none, ss, L, subsets["duplicate"], p, n_masks=0,
                     tags=frozenset({"residue_only"})))

    # ---- sharelen: clerk rows longer than the batch count (the compact copy); ragged on the host form
    for ss, tag in ((FL, "fl"), (CP, "cp")):
        p = ss.prime_modulus
        for L in packed_dims(ss)[1:]:
            out.append(R("sharelen", f"{tag}-B+3-D{L}", full(p), ss, L, _threshold(ss), p, share_extra=3,
                         forms=("dev",), tags=frozenset({"residue_only"})))
        out.append(R("sharelen", f"{tag}-B+3-ne", chacha(p + 2, packed_dims(ss)[4], 128), ss, packed_dims(ss)[4],
                     _all(ss), p, share_extra=3, forms=("dev",), tags=frozenset({"representative"})))
        r = ss.reconstruction_threshold()
        out.append(R("sharelen", f"{tag}-host-ragged", full(p + 2), ss, packed_dims(ss)[4], _threshold(ss), p,
                     forms=("host",), host_share_extra=tuple((i * 2) % 5 for i in range(r)),
                     tags=frozenset({"representative"})))
        out.append(R("sharelen", f"{tag}-host-longer", none, ss, packed_dims(ss)[3], _threshold(ss), p, n_masks=0,
                     forms=("host",), host_share_extra=tuple(2 + i % 3 for i in range(r)),
                     tags=frozenset({"residue_only"})))

    # ---- outcap: D and D + 8 (D - 1 is a status row)
    out.append(R("outcap", "add-D257+8", full(P), S.Additive(2, P), 257, (0, 1), P, out_slack=8))
    out.append(R("outcap", "cp-D69+8", full(P), CP, 69, _threshold(CP), P, out_slack=8,
                 tags=frozenset({"residue_only"})))
    out.append(R("outcap", "fl-D13+8-ne", none, FL, 13, _threshold(FL), 435, n_masks=0, out_slack=8,
                 tags=frozenset({"representative"})))

    # ---- chachamod: the ChaCha moduli by path
    for i, m in enumerate((CHACHA_FAST, CHACHA_HIGH_REJECTION, CHACHA_ABOVE_2_62, 1, 2)):
        L = ELEMENTWISE_D[i % 4]
        out.append(R("chachamod", f"m{m}-add-D{L}", chacha(m, L, 128), S.Additive(2, MODULI[(i + 3) % len(MODULI)]), L,
                     (0, 1), (m, 0, -m)[i % 3], n_masks=3, raw=True))
    out.append(R("chachamod", f"m{CHACHA_HIGH_REJECTION}-cp-D69", chacha(CHACHA_HIGH_REJECTION, 69, 128), CP, 69,
                 _threshold(CP), P, tags=frozenset({"representative"})))

    # ---- outmod: output moduli p, p + 2, 2^40, 0, -p, 2^63 - 1 over signed reveals
    for ss, tag in ((FL, "fl"), (CP, "cp")):
        p = ss.prime_modulus
        for i, m_out in enumerate((p, p + 2, 2**40, 0, -p, I64_MAX)):
            L = packed_dims(ss)[i % 5] if m_out == p else packed_dims(ss)[4]
            tags = {"residue_only"} if m_out == p else {"representative"}
            out.append(R("outmod", f"{tag}-full-out{m_out}-D{L}", full(p), ss, L, _threshold(ss), m_out,
                         tags=frozenset(tags)))
        out.append(R("outmod", f"{tag}-none-out{p + 2}", none, ss, packed_dims(ss)[4], _all(ss), p + 2, n_masks=0,
                     tags=frozenset({"representative"})))
        out.append(R("outmod", f"{tag}-negq-out{p}", full(-p), ss, packed_dims(ss)[4], _threshold(ss), p,
                     tags=frozenset({"residue_only"})))

    # ---- wide: one workspace-kernel scheme, one shape (tests/test_gpu_packed_matrix.py owns that kernel)
    W = wide_scheme()
    out.append(R("wide", "n242-all-D22", chacha(W.prime_modulus, 22, 128), W, 22, _all(W), W.prime_modulus,
                 tags=frozenset({"residue_only"})))

    # ---- late: the mask's rejection is resolved after the reveal was queued
    out.append(R("late", f"m{CHACHA_FAST}-add-D{LATE_D}", chacha(CHACHA_FAST, LATE_D, 128),
                 S.Additive(2, CHACHA_FAST), LATE_D, (0, 1), CHACHA_FAST, n_masks=1, forms=("dev",),
                 tags=frozenset({"late"})))
    return out


def _golden_late():
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chacha_rejects.json")))
    s, pair = min(g["moduli"][str(CHACHA_FAST)], key=lambda h: h[1])
    return (s, 0x5DA, 7, 11), pair


LATE_SEED, LATE_PAIR = _golden_late()        # the golden seed of CHACHA_FAST whose first rejected pair comes first
LATE_D = (LATE_PAIR // 256 + 1) * 256 + 1    # past that pair, a one-lane tail

RECIPIENT_CASES = _recipient_cases()

# ---------------------------------------------------------------- recipient: zero-length successes
RECIPIENT_ZERO = [
    RecipientCase("zero", "cp-D0", S.FullMasking(P), CP, 0, _threshold(CP), P, n_masks=0),
    RecipientCase("zero", "cp-D0-no-shares", S.NoMasking(), CP, 0, (), P, n_masks=0),
    RecipientCase("zero", "add-no-shares", S.NoMasking(), S.Additive(3, 433), 5, (), 433, n_masks=0),
    RecipientCase("zero", "add-no-shares-chacha0", S.ChaChaMasking(-7, 0, 128), S.Additive(3, 0), 5, (), 0, n_masks=2),
    RecipientCase("zero", "add-empty-rows-full0", S.FullMasking(0), S.Additive(2, 0), 0, (0, 1), 0, n_masks=0),
]


# ---------------------------------------------------------------- recipient: every early return, once
def _recipient_status_cases():
    R = RecipientCase
    add, none = S.Additive(2, 433), S.NoMasking()
    g = "status"
    both = ("host", "dev")
    rows = [
        R(g, "none-with-mask", none, add, 4, (0, 1), 433, n_masks=2, mask_width=3),
        R(g, "chacha-width0", S.ChaChaMasking(433, 4, 128), add, 4, (0, 1), 433, mask_width=0, forms=("dev",)),
        R(g, "chacha-width9", S.ChaChaMasking(433, 4, 288), add, 4, (0, 1), 433, mask_width=9, forms=("dev",)),
        R(g, "chacha-m0-masks", S.ChaChaMasking(0, 4, 128), add, 4, (0, 1), 433),
        R(g, "chacha-negative-masks", S.ChaChaMasking(-433, 4, 128), add, 4, (0, 1), 433),
        R(g, "chacha-m0-no-masks", S.ChaChaMasking(0, 4, 128), add, 4, (0, 1), 433, n_masks=0),
        R(g, "full-m0", S.FullMasking(0), add, 4, (0, 1), 433),
        R(g, "full-i64min", S.FullMasking(I64_MIN), add, 4, (0, 1), 433),
        R(g, "chacha-i64min-no-masks", S.ChaChaMasking(I64_MIN, 4, 128), add, 4, (0, 1), 433, n_masks=0),
        R(g, "add-m0", none, S.Additive(2, 0), 4, (0, 1), 433, n_masks=0),
        R(g, "add-i64min", none, S.Additive(2, I64_MIN), 4, (0, 1), 433, n_masks=0),
        R(g, "add-mismatching", none, add, 4, (0, 1), 433, n_masks=0, row_lens=(4, 3), forms=("host",)),
        R(g, "add-mismatching-after-none-mask", none, add, 4, (0, 1), 433, n_masks=1, mask_width=2, row_lens=(4, 3),
          forms=("host",)),
        R(g, "add-mismatching-after-m0", none, S.Additive(2, 0), 4, (0, 1), 433, n_masks=0, row_lens=(4, 3),
          forms=("host",)),
        R(g, "full-ragged-masks", S.FullMasking(433), add, 4, (0, 1), 433, forms=("host",), host_mask_lens=(4, 3)),
        R(g, "packed-short-enough", none, FL, 7, _threshold(FL), 433, n_masks=0, share_extra=-1),
        R(g, "packed-empty-rows-few", none, FL, 7, (0, 1), 433, n_masks=0, share_extra=-3),
        R(g, "packed-too-few", none, FL, 7, _threshold(FL)[:-1], 433, n_masks=0),
        R(g, "packed-too-many", none, FL, 2, tuple(i % 8 for i in range(PD.REVEAL_MAX_SHARES + 1)), 433, n_masks=0),
        R(g, "packed-bad-mode", none, FL, 7, _threshold(FL), 433, n_masks=0, mode=7),
        R(g, "full-mask-len", S.FullMasking(433), add, 4, (0, 1), 433, mask_width=5),
        R(g, "full-no-masks", S.FullMasking(433), add, 4, (0, 1), 433, n_masks=0),
        R(g, "chacha-dimension", S.ChaChaMasking(433, 5, 128), FL, 7, _threshold(FL), 433),
        R(g, "out-cap", none, add, 4, (0, 1), 433, n_masks=0, out_slack=-1),
        R(g, "out-cap-packed", S.FullMasking(433), FL, 7, _threshold(FL), 433, out_slack=-1),
    ]
    for null in ("ms", "ss", "out_len", "shares", "indices", "masks"):
        rows.append(R(g, f"null-{null}", S.FullMasking(433), add, 4, (0, 1), 433, null=null, forms=both))
    return rows


RECIPIENT_STATUS = _recipient_status_cases()


def recipient_expected_status(case, form):
    """The (status, message class) tests/pipeline_dispatch.py predicts for a status row."""
    if case.null:
        return (PD.INVALID_ARGUMENT, "NULL argument")
    masks, indexed = host_rows(case) if form == "host" else recipient_inputs(case)
    if form == "host":
        st, _ = PD.recipient_host_status(case.ms, [len(r) for r in masks], case.ss, case.dimension,
                                         [len(r) for _, r in indexed], case.m_out, case.mode, case.D + case.out_slack)
    else:
        width = len(masks[0]) if masks else (case.mask_width or 0)
        if isinstance(case.ms, S.ChaChaMasking):
            width = case.seed_words if case.mask_width is None else case.mask_width
        share_len = len(indexed[0][1]) if indexed else 0
        st, _ = PD.recipient_status(case.ms, len(masks), width, case.ss, case.dimension, len(indexed), share_len,
                                    case.m_out, case.mode, case.D + case.out_slack)
    return st


# ================================================================ participant
@dataclass(frozen=True)
class ParticipantCase:
    group: str
    name: str
    entry: str                                # PD.ENTRIES
    ms: object
    ss: object
    D: int
    secrets: str = "inside"                   # "inside": (-m, m) of the masking (else sharing) modulus; "i64": steered
    mode: int = EXACT
    payload: bool = True
    tags: frozenset = field(default_factory=frozenset)
    # status rows only
    null: Optional[str] = None
    seed_words: Optional[int] = None          # overrides the scheme's seed word count
    payload_short: bool = False

    @property
    def id(self):
        return f"{self.group}-{self.entry}-{self.name}"

    @property
    def keyed(self):
        return self.entry in ("keyed", "keyed32")

    @property
    def narrow(self):
        return self.entry in ("dev32", "keyed32")

    @property
    def B(self):
        return PD.batches(self.ss, self.D) if PD.is_packed(self.ss) else self.D


@functools.lru_cache(maxsize=None)
def participant_inputs(case):
    """(secrets, seed words or None, full masks or None, draws) as Python integer lists; a keyed case's draws are
    those of (KEY, STREAM) under the engine's documented rule (tests/draws_model.py)."""
    rng = _rng(case.id)
    rot = zlib.crc32(case.id.encode()) >> 8
    ms, ss, D = case.ms, case.ss, case.D
    bound = ss.modulus if isinstance(ms, S.NoMasking) else ms.modulus
    bound = bound if bound > 0 else P
    secrets = steered(rng, D, bound, rot) if case.secrets == "i64" else canonical(rng, D, bound, True)
    seed = full = None
    if isinstance(ms, S.FullMasking):
        full = canonical(rng, D, bound, False)
        if "wrap" in case.tags:
            secrets[0], full[0] = I64_MAX, bound - 1
    elif isinstance(ms, S.ChaChaMasking):
        w = ms.seed_words() if case.seed_words is None else case.seed_words
        seed = list(LATE_SEED) if "late" in case.tags else [int(x) for x in
                                                            rng.integers(0, 2**32, size=w, dtype=np.uint64)]
    if PD.is_packed(ss):
        count, dbound = case.B * ss.privacy_threshold(), ss.prime_modulus - 1
    else:
        count, dbound = D * max(ss.share_count - 1, 0), ss.modulus
    if dbound <= 0:
        draws = [0] * count
    elif case.keyed:
        draws = [int(x) for x in DM.draws(KEY, STREAM, 0, count, dbound)]
    else:
        draws = canonical(rng, count, dbound, False)
    return secrets, seed, full, draws


def _participant_cases():
    out = []
    C = ParticipantCase
    none, full, chacha = S.NoMasking(), S.FullMasking, S.ChaChaMasking
    W = wide_scheme()

    def entries(ss):
        if PD.is_packed(ss):
            return PD.ENTRIES
        return ("dev", "keyed", "keyed32") if ss.modulus <= 2**31 else ("dev", "keyed")

    # ---- routes: masking kind x mask route x secrets variant x sharing scheme x mode, over the entry points
    i = 0
    for ss, tag in ((S.Additive(1, 433), "add1"), (S.Additive(2, P), "add2"), (S.Additive(3, 2**31), "add3"),
                    (S.Additive(3, 2**40 + 7), "add3big"), (S.Additive(2, I64_MAX), "add2max"), (FL, "fl"), (CP, "cp")):
        packed = PD.is_packed(ss)
        p = ss.modulus
        dims = packed_dims(ss) if packed else ELEMENTWISE_D
        # a packed scheme's secrets are its field's: the masking modulus is the sharing prime there
        maskings = [("none", lambda D: none), ("full", lambda D: full(p)),
                    ("chachafast", lambda D: chacha(p if packed or p <= 2**31 else CHACHA_FAST, D, 128))]
        if not packed:
            maskings += [("chachahigh", lambda D: chacha(CHACHA_HIGH_REJECTION, D, 128)),
                         ("chachabig", lambda D: chacha(CHACHA_ABOVE_2_62, D, 128)),
                         ("fullbig", lambda D: full(I64_MAX))]
        for mname, mk in maskings:
            for entry in entries(ss):
                D = dims[i % len(dims)]
                ms = mk(D)
                masked_bound = p if isinstance(ms, S.NoMasking) else ms.modulus
                if not packed and entry == "keyed32" and ss.share_count == 1 and masked_bound > 2**31:
                    continue                  # n = 1 hands the masked secret out unreduced: it has to fit int32
                for sv in ("inside", "i64"):
                    # secrets over all of i64 need the mask to bring them back into what the shares can hold: a
                    # packed scheme's field, and int32 for the one-share Additive rows
                    if sv == "i64" and isinstance(ms, S.NoMasking) and (packed or (entry == "keyed32" and
                                                                                   ss.share_count == 1)):
                        continue
                    mode = (EXACT, CANONICAL)[i % 2] if packed else EXACT
                    tags = set()
                    if sv == "i64" and isinstance(ms, S.FullMasking) and ms.modulus >= 433:
                        tags.add("wrap")
                    out.append(C("routes", f"{tag}-{mname}-{sv}-{'canon' if mode else 'exact'}-D{D}", entry, ms, ss, D,
                                 secrets=sv, mode=mode, payload=(i % 3 != 0), tags=frozenset(tags)))
                    i += 1
    # ---- wide: the workspace kernels once per entry point
    for entry in PD.ENTRIES:
        out.append(C("wide", "n242-full-D22", entry, full(W.prime_modulus), W, 22))
    # ---- seeds: 0 (seed_bitsize 0), 1, 8 and 9 words
    for bits in (0, 32, 256, 288):
        for entry, ss in (("dev", S.Additive(2, P)), ("keyed32", CP)):
            D = 257 if entry == "dev" else 69
            out.append(C("seeds", f"bits{bits}-D{D}", entry, chacha(P, D, bits), ss, D, secrets="i64"))
    # ---- small moduli on the masks: 1 and 2
    for m in (1, 2):
        out.append(C("smallm", f"full-m{m}-add-D256", "dev", full(m), S.Additive(2, m), 256, secrets="i64"))
        out.append(C("smallm", f"chacha-m{m}-add-D255", "keyed", chacha(m, 255, 128), S.Additive(3, m), 255,
                     secrets="i64"))
    # ---- late: a rejecting seed, the mask and every later step redone
    out.append(C("late", f"m{CHACHA_FAST}-add-D{LATE_D}", "dev", chacha(CHACHA_FAST, LATE_D, 128),
                 S.Additive(2, CHACHA_FAST), LATE_D, tags=frozenset({"late"})))
    out.append(C("late", f"m{CHACHA_FAST}-add-D{LATE_D}", "keyed", chacha(CHACHA_FAST, LATE_D, 128),
                 S.Additive(2, CHACHA_FAST), LATE_D, tags=frozenset({"late"})))
    return out


PARTICIPANT_CASES = _participant_cases()

PARTICIPANT_ZERO = [ParticipantCase("zero", f"{tag}-D0", entry, ms, ss, 0)
                    for entry in PD.ENTRIES
                    for tag, ms, ss in (("none-cp", S.NoMasking(), CP), ("chacha-cp", S.ChaChaMasking(P, 0, 128), CP),
                                        ("full0-cp", S.FullMasking(0), CP))] + \
                   [ParticipantCase("zero", "full-add-D0", "dev", S.FullMasking(-5), S.Additive(2, 433), 0),
                    ParticipantCase("zero", "none-add-D0", "keyed", S.NoMasking(), S.Additive(1, 433), 0)]


def _participant_status_cases():
    C = ParticipantCase
    g = "status"
    add = S.Additive(2, 433)
    rows = []
    for entry in PD.ENTRIES:
        ss = CP if entry == "dev32" else add
        rows += [C(g, "full-m0", entry, S.FullMasking(0), ss, 8), C(g, "chacha-negative", entry,
                                                                    S.ChaChaMasking(-433, 8, 128), ss, 8),
                 C(g, "seed-words", entry, S.ChaChaMasking(433, 8, 128), ss, 8, seed_words=3),
                 C(g, "chacha-dimension", entry, S.ChaChaMasking(433, 9, 128), ss, 8),
                 C(g, "chacha-dimension-D0", entry, S.ChaChaMasking(433, 9, 128), ss, 0),
                 C(g, "bad-mode", entry, S.NoMasking(), ss, 8, mode=7),
                 C(g, "null-full-masks", entry, S.FullMasking(433), ss, 8, null="full_masks"),
                 C(g, "null-seed", entry, S.ChaChaMasking(433, 8, 128), ss, 8, null="seed"),
                 C(g, "null-secrets", entry, S.NoMasking(), ss, 8, null="secrets"),
                 C(g, "null-shares", entry, S.NoMasking(), ss, 8, null="shares"),
                 C(g, "null-row-bytes", entry, S.NoMasking(), ss, 8, null="payload_row_bytes"),
                 C(g, "payload-cap", entry, S.NoMasking(), ss, 8, payload_short=True)]
    rows += [C(g, "null-draws", "dev", S.NoMasking(), add, 8, null="draws"),
             C(g, "null-draws", "dev32", S.NoMasking(), CP, 8, null="draws"),
             C(g, "null-key", "keyed", S.NoMasking(), add, 8, null="key"),
             C(g, "null-key", "keyed32", S.NoMasking(), CP, 8, null="key"),
             C(g, "additive", "dev32", S.NoMasking(), add, 8),
             C(g, "additive-above-2^31", "keyed32", S.NoMasking(), S.Additive(2, 2**31 + 1), 8),
             C(g, "share-count-0", "dev", S.NoMasking(), S.Additive(0, 433), 8),
             C(g, "share-count-0", "keyed", S.NoMasking(), S.Additive(0, 433), 8),
             C(g, "additive-m0", "dev", S.NoMasking(), S.Additive(2, 0), 8),
             C(g, "additive-negative", "keyed", S.NoMasking(), S.Additive(2, -433), 8)]
    return rows


PARTICIPANT_STATUS = _participant_status_cases()


def participant_expected_status(case):
    if case.null in ("secrets", "shares", "payload_row_bytes", "key"):
        return (PD.INVALID_ARGUMENT, "NULL argument")
    words = case.ms.seed_words() if isinstance(case.ms, S.ChaChaMasking) and case.seed_words is None else \
        (case.seed_words or 0)
    return PD.participant_status(case.ms, case.ss, case.entry, case.D, words, case.mode,
                                 has_seed=case.null != "seed", has_full_masks=case.null != "full_masks",
                                 has_draws=case.null != "draws", payload_cap=0 if case.payload_short else None,
                                 payload_need=1)


ALL_CASES = (RECIPIENT_CASES + RECIPIENT_ZERO + RECIPIENT_STATUS + PARTICIPANT_CASES + PARTICIPANT_ZERO +
             PARTICIPANT_STATUS)
