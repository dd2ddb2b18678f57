"""CPU: the plan of tests/test_gpu_packed_keyed.py (packed-Shamir share generation with in-kernel draws), held to
what it claims -- no GPU and no product import beyond the schemes.

A keyed tile of BS = 256 batches (packed_gen.hip: gen_block, every keyed kernel has k + t + 1 <= 16) owns draw
elements [E0, E0 + nb t), E0 = (first_batch + vec B + b0) t, and makes them in ChaCha blocks of 8: E0 mod 8 says how
many elements of the tile's first block belong to the batch before it.  The slice list below moves that residue, and
the planted batches of the fix-up test sit in the tiles the GPU test names.
"""
from sda_amd import schemes as S
from tests import draws_model as DM
from tests import packed_dispatch as PD
from tests import packed_matrix_cases as PM

KEY, STREAM = DM.TEST_KEY, DM.TEST_STREAM
BS = 256                                   # batches per keyed tile
ODD_FIRST = 12345                          # the kernel matrix's odd first_batch

# ---- first_batch is a batch slice: one vector of SLICE_B batches, cut into (first_batch, width) slices ----
SLICE_B = 1100
SLICE_SCHEMES = (S.CONFIG_PACKED, PM.scheme_for(5, 2, 26))          # t = 7 and t = 2
SLICES = ((0, 1), (1, 2), (3, 297), (300, 257), (557, 301), (858, 242))

# ---- the fix-up test: raw secrets planted at {(vec, batch)} of a V x FIX_B launch ----
FIX_B = PM.B_EVEN
FIX_PLANTS = ((0, 0), (PM.V - 1, FIX_B - 1), (1, 520))


def tile_of(b):
    return b // BS


def tile_is_ragged(tile, B):
    return (tile + 1) * BS > B


def start_residue(first_batch, t):
    return first_batch * t % 8


def test_keyed_kernels_run_256_batch_tiles():
    for N3, Ls in PD.GEN_PARTS.items():
        if N3 <= 27:
            assert all(PD.gen_block(L) == BS for L in Ls)


def test_slices_tile_the_job_with_ragged_widths():
    assert SLICES[0][0] == 0 and sum(w for _, w in SLICES) == SLICE_B
    for (f, w), (g, _) in zip(SLICES, SLICES[1:]):
        assert f + w == g
    assert all(w % BS for _, w in SLICES)
    assert any(w > BS for _, w in SLICES)                     # a slice of more than one tile


def test_slices_reach_the_residues_they_claim():
    t7, t2 = (s.privacy_threshold() for s in SLICE_SCHEMES)
    assert (t7, t2) == (7, 2)
    assert {start_residue(f, t7) for f, _ in SLICES} == {0, 7, 5, 4, 3, 6}
    assert {start_residue(f, t2) for f, _ in SLICES} == {0, 2, 4, 6}       # every residue an even t can reach
    # the multi-vector split: vector v of a V-vector call starts at first_batch = v B
    assert len({start_residue(v * SLICE_B, t7) for v in range(PM.V)}) == 2


def test_odd_first_batch_starts_inside_a_block():
    """Every matrix scheme that draws (t > 0) starts its first tile inside a ChaCha block at ODD_FIRST: an odd
    residue with an odd t, an even nonzero one with t = 2 or 4."""
    assert ODD_FIRST % 4 == 1
    seen = set()
    for case in PM.GEN_CASES:
        t = case.sch.privacy_threshold()
        if case.sch.share_count + 1 > 27 or t == 0:
            continue
        assert start_residue(ODD_FIRST, t) != 0, case.id
        seen.add(t)
    assert {1, 2, 4, 7} <= seen


def test_planted_batches_land_in_the_tiles_named():
    B, V = FIX_B, PM.V
    first, last, ragged = FIX_PLANTS
    assert first == (0, 0) and tile_of(first[1]) == 0 and not tile_is_ragged(0, B)
    assert last == (V - 1, B - 1) and tile_is_ragged(tile_of(last[1]), B)
    assert tile_is_ragged(tile_of(ragged[1]), B) and 0 < ragged[0] < V - 1 and ragged[1] < B - 2
    assert B // BS == 2                                        # two full tiles, then the ragged one
    # each plant logs its batch and the store-pair partner
    assert PD.gen_fixup_count("packed_gen_kernel<16, 27, true, false, true, true>", frozenset(FIX_PLANTS), B) == 6
