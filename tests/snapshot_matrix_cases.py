"""The snapshot transposition's steered copy matrix: the cases of tests/test_gpu_snapshot_matrix.py (GPU) and
tests/test_snapshot_matrix_plan.py (CPU), built for a chunk size C (sda_snapshot_last_launch reports it).

Blob geometry is steered through the offsets alone.  Clerk c's blob p lands at clerk_base[c] + the lengths of the
clerk's earlier blobs, and comes from part_off[0] + everything before it in participation-major order.  So the
target clerk's own lengths (spacer blobs between the stated ones) set each blob's destination start mod 16 and its
length; the other clerk's filler blobs and part_off[0] move the source, which sets the shift (src - dst) mod 16
without moving the destination.  Two layouts alternate: the filler as clerk 0 in front of the target (its first
blob carries the shift, the rest are multiples of 16), or the target as clerk 0 (part_off[0] carries the shift).

Every case states the (shift, dst start mod 16, len) triples it was built to contain (`claims`); the plan test
finds them in plan()'s blob list.

  Q  one-chunk blobs: one case per shift, every dst start mod 16, the lengths of q_lengths()
  L  lane guards: body quad counts 1, 255, 256, 257, 2047, 2048 of one chunk
  C  chunk boundaries: lengths around C, 2C and 4C at every shift
  W  the workgroup walk: chunk counts per blob that produce each named event
  Z  empty blobs
  R  (GPU file) plan buffer reuse on one handle
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests import snapshot_dispatch as SD

Q_FIXED = (1, 16, 17, 31, 32, 33, 47, 48, 49)
L_QUADS = (1, 255, 256, 257, 2047, 2048)
L_ODD = (7, 5)                      # the L group at an odd shift and a dst start off the quad
L_ODD_ALIGNED = (9, 0)              # an odd shift at dst start 0: the one place 2048 unaligned quads fit one chunk
C_SHIFTS_OFF = (0, 1, 8, 15)        # the shifts that also run at dst starts 1 and 15
W_EVENTS = ("first_chunk_mid_blob", "first_chunk_last_of_blob", "switch_at_step_1", "switch_at_step_2",
            "switch_at_step_3", "four_one_chunk_blobs_in_a_walk", "search_lands_on_blob_0",
            "search_lands_on_last_blob", "search_lands_on_exact_start", "search_lands_inside_a_blob")
Z_SHAPES = ("first_blob_of_a_clerk_empty", "last_blob_of_a_clerk_empty", "run_of_empties_between",
            "whole_clerk_empty", "every_blob_empty", "P1_n1")


def inside_len(r):
    """the largest length from dst start r that stays inside one quad"""
    return 16 - r


def straddle_len(r):
    """a length below 16 from dst start r that ends inside the next quad (head + tail, no body): none for r < 2"""
    return 16 - r + 1 + (r - 2) // 2 if r >= 2 else None


def head_quad_tail_len(r):
    """head (none at r = 0) + exactly one body quad + a tail of 1..15 bytes"""
    return (16 - r if r else 0) + 16 + 1 + (r * 7) % 15


def c_lengths(C):
    """name -> length of the C family"""
    return {"C-17": C - 17, "C-16": C - 16, "C-1": C - 1, "C": C, "C+1": C + 1, "C+15": C + 15, "C+16": C + 16,
            "C+17": C + 17, "2C-1": 2 * C - 1, "2C": 2 * C, "2C+1": 2 * C + 1, "4C+1": 4 * C + 1}


C_HALVES = {"a": ("C-17", "C-16", "C-1", "C", "C+1", "C+15", "C+16", "C+17"), "b": ("2C-1", "2C", "2C+1", "4C+1")}


def q_lengths(r):
    """the Q lengths at dst start r: 1, the largest inside one quad, one less than that (the largest that leaves the
    quad's end alone; the chunk-inside-one-quad collapse for r >= 1), the straddle, 16, 17, head + one quad + tail,
    and 31..49"""
    out = [1, inside_len(r), head_quad_tail_len(r), *Q_FIXED]
    if inside_len(r) - 1 >= 2:
        out.append(inside_len(r) - 1)
    if straddle_len(r) is not None:
        out.append(straddle_len(r))
    return sorted(set(out))


@dataclass
class Case:
    id: str
    family: str
    lens: list                      # [P][n] blob lengths
    pad: int                        # part_off[0]
    shift: int = None               # the steered shift of the target clerk's blobs (Q, L, C)
    target: int = 0                 # the target clerk
    claims: set = field(default_factory=set)          # (shift, dst start mod 16, len)
    quads: set = field(default_factory=set)           # L: (shift, dst start mod 16, body quads of one chunk)
    events: tuple = ()              # W
    shapes: tuple = ()              # Z
    chunk_counts: tuple = ()        # W

    @property
    def P(self):
        return len(self.lens)

    @property
    def n(self):
        return len(self.lens[0])

    def part_off(self):
        flat = [x for row in self.lens for x in row]
        return np.concatenate([[self.pad], self.pad + np.cumsum(flat, dtype=np.uint64)]).astype(np.uint64)

    def src(self):
        """seeded random bytes: part_off[0] of padding, the blobs, the 32 readable bytes the header asks for"""
        size = int(self.part_off()[-1]) + 32
        seed = int.from_bytes(self.id.encode(), "little") % (1 << 63)
        return np.random.default_rng(seed).integers(0, 256, size=size, dtype=np.uint8)

    def blobs(self):
        """[participation][clerk] bytes, what oracle.snapshot_transpose takes"""
        raw, off = self.src().tobytes(), self.part_off()
        return [[raw[int(off[p * self.n + c]):int(off[p * self.n + c + 1])] for c in range(self.n)]
                for p in range(self.P)]


def place(shift, wanted):
    """the target clerk's lengths holding a blob of length L at dst start r for every (r, L) of `wanted`, in that
    order, with a spacer blob wherever the running offset does not already sit at r; and the claims"""
    lens, claims, cur = [], set(), 0
    for r, L in wanted:
        gap = (r - cur) % 16
        if gap:
            lens.append(gap)
            cur += gap
        lens.append(L)
        claims.add((shift, r, L))
        cur = (cur + L) % 16
    return lens, claims


def steer(target_lens, shift, filler_first):
    """[P][2] lengths and part_off[0] that give every blob of the target clerk the shift"""
    P = len(target_lens)
    if filler_first:                                 # target = clerk 1: shift = pad + f[0] + ... + f[p]  (mod 16)
        pad = (5 * shift + 3) % 16
        f = [(shift - pad) % 16 or 16] + [16 * (1 + p % 2) for p in range(1, P)]
        return [[f[p], target_lens[p]] for p in range(P)], pad, 1
    pad = shift + 16 * (shift % 3)                   # target = clerk 0: shift = pad + f[0] + ... + f[p - 1]
    f = [16 * (1 + (p + shift) % 2) for p in range(P)]
    return [[target_lens[p], f[p]] for p in range(P)], pad, 0


def _steered(cid, family, shift, wanted, **kw):
    tl, claims = place(shift, wanted)
    lens, pad, target = steer(tl, shift, filler_first=shift % 2 == 0)
    return Case(cid, family, lens, pad, shift=shift, target=target, claims=claims, **kw)


def q_cases():
    # the clerk's last blob is one more quad-inside collapse: a byte written past its end lands in padding, which
    # nothing rewrites
    return [_steered(f"Q-s{s}", "Q", s, [(r, L) for r in range(16) for L in q_lengths(r)] + [(3, 12)])
            for s in range(16)]


def l_cases(C):
    q1 = C // 16                                     # the quads of one chunk (2048 as shipped)
    assert q1 == L_QUADS[-1], "the lane-guard counts are those of 256 lanes x 8 quads"
    out = [_steered("L-s0-d0", "L", 0, [(0, 16 * q) for q in L_QUADS], quads={(0, 0, q) for q in L_QUADS})]
    s, r = L_ODD
    # from dst start 5 a chunk holds at most 2047 whole quads (the head takes part of one): the 2048-quad length
    # is there all the same; the chunk boundary cuts its last quad into 5 tail bytes and 11 head bytes
    out.append(_steered(f"L-s{s}-d{r}", "L", s, [(r, 16 - r + 16 * q + 3) for q in L_QUADS],
                        quads={(s, r, q) for q in L_QUADS[:-1]}))
    s, r = L_ODD_ALIGNED
    out.append(_steered(f"L-s{s}-d{r}", "L", s, [(r, 16 * q) for q in L_QUADS], quads={(s, r, q) for q in L_QUADS}))
    return out


def c_plan():
    return [(s, 0) for s in range(16)] + [(s, r) for s in C_SHIFTS_OFF for r in (1, 15)]


def c_cases(C):
    lens = c_lengths(C)
    return [_steered(f"C-s{s}-d{r}-{half}", "C", s, [(r, lens[name]) for name in names])
            for s, r in c_plan() for half, names in C_HALVES.items()]


# W: chunks per planned blob, part_off[0], the events the case was chosen for
W_PLAN = (
    ("W-1", (1,), 0, ("search_lands_on_blob_0", "search_lands_on_last_blob")),
    ("W-2", (1, 1), 3, ("switch_at_step_1",)),
    ("W-3", (1, 2), 6, ("switch_at_step_1",)),
    ("W-4", (1, 1, 1, 1), 9, ("four_one_chunk_blobs_in_a_walk", "switch_at_step_1", "switch_at_step_2",
                              "switch_at_step_3")),
    ("W-5", (5,), 12, ("first_chunk_mid_blob", "search_lands_inside_a_blob")),
    ("W-7", (4, 3), 15, ("first_chunk_last_of_blob", "switch_at_step_1")),
    ("W-8", (2, 2, 1, 3), 2, ("switch_at_step_2", "search_lands_on_exact_start")),
    ("W-9", (1, 4, 1, 3), 5, ("first_chunk_mid_blob", "switch_at_step_2", "search_lands_on_last_blob",
                              "search_lands_on_exact_start")),
    ("W-13a", (3, 3, 3, 3, 1), 8, ("switch_at_step_3", "search_lands_on_exact_start")),
    ("W-13b", (1,) * 13, 11, ("four_one_chunk_blobs_in_a_walk",)),
)


def w_cases(C):
    """the planned blob list is clerk-major, so the first half of the counts goes to clerk 0 and the rest to clerk 1
    (its missing participations are empty blobs): the source interleaves the two clerks, and neither the source nor
    the destination of consecutive planned blobs is contiguous"""
    out = []
    for cid, counts, pad, events in W_PLAN:
        blob_lens = []
        for i, k in enumerate(counts):               # k chunks: k - 1 whole ones and 1..C bytes more
            rem = C if i % 3 == 0 else 1 + (i * 9973 + 17 * k) % C
            blob_lens.append((k - 1) * C + rem)
        h = (len(counts) + 1) // 2
        c0, c1 = blob_lens[:h], blob_lens[h:] + [0] * (2 * h - len(counts))
        out.append(Case(cid, "W", [[c0[p], c1[p]] for p in range(h)], pad, events=events, chunk_counts=counts))
    return out


def z_cases():
    return [
        #            clerk 0  1  2
        Case("Z-mixed", "Z", [[0, 0, 7],
                              [5, 0, 0],
                              [0, 0, 0],
                              [0, 0, 20],
                              [9, 0, 0]], 4,
             shapes=("first_blob_of_a_clerk_empty", "last_blob_of_a_clerk_empty", "run_of_empties_between",
                     "whole_clerk_empty")),
        Case("Z-edges", "Z", [[0, 0, 0], [0, 33, 0], [0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]], 0,
             shapes=("first_blob_of_a_clerk_empty", "last_blob_of_a_clerk_empty", "run_of_empties_between",
                     "whole_clerk_empty")),
        Case("Z-all-empty", "Z", [[0, 0], [0, 0], [0, 0]], 7, shapes=("every_blob_empty", "whole_clerk_empty")),
        Case("Z-one-empty", "Z", [[0]], 0, shapes=("every_blob_empty", "whole_clerk_empty", "P1_n1")),
        Case("Z-one", "Z", [[40]], 3, shapes=("P1_n1",)),
    ]


@functools.lru_cache(maxsize=2)
def build(C=SD.CHUNK):
    """every case of the matrix for chunk size C, by id"""
    cases = q_cases() + l_cases(C) + c_cases(C) + w_cases(C) + z_cases()
    out = {c.id: c for c in cases}
    assert len(out) == len(cases)
    return out


IDS = tuple(build())                # the ids do not depend on C
ALL_EMPTY = "Z-all-empty"
R_SMALL, R_LARGE = "Z-one", "Q-s3"  # case R: a 1-blob plan, a plan of ~900 blobs, the 1-blob plan again


@functools.lru_cache(maxsize=None)
def model(cid, C=SD.CHUNK):
    """(plan, the whole dst buffer the kernel must leave) of a case; computed once, never written to"""
    case = build(C)[cid]
    buf = SD.transpose_model(case.src(), case.part_off(), case.P, case.n, C=C)
    buf.setflags(write=False)
    return SD.plan(case.part_off(), case.P, case.n, C), buf
