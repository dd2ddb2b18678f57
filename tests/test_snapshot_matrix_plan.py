"""CPU: the plan of tests/test_gpu_snapshot_matrix.py against the oracle and against itself.

The numpy restatement of the snapshot transposition's host plan and copy kernel (tests/snapshot_dispatch.py) must
agree with oracle.snapshot_transpose on every case of tests/snapshot_matrix_cases.py and leave every byte outside
the blobs alone; the union of the cases must contain every geometry the matrix is there for, written out as sets;
the sda_snapshot_last_launch record each case predicts must be consistent with its own plan; and each named mistake
in the kernel's index arithmetic (snapshot_dispatch.FAULTS), injected into the model, must change the full dst
buffer of at least one case -- a fault no case catches is a hole in the matrix.
"""
import numpy as np
import pytest

from tests import snapshot_dispatch as SD
from tests import snapshot_matrix_cases as CM

C = SD.CHUNK
CASES = CM.build(C)


def _triples(pl):
    return {((s - d) & 15, d & 15, ln) for s, d, ln in pl.blobs}


def _target_blobs(case, pl):
    """the target clerk's planned blobs"""
    lo = pl.clerk_base[case.target]
    hi = lo + pl.clerk_off[case.target][case.P]
    return [b for b in pl.blobs if lo <= b[1] < hi]


def _body_quads(blob, k):
    a, A, E, e = SD.chunk_geometry(blob, k, C)
    return (E - A) // 16 if A < E else 0


def _n_chunks(blob):
    return (blob[2] + C - 1) // C


# ---------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("cid", CM.IDS)
def test_model_matches_oracle_and_leaves_the_rest(oracle, cid):
    case = CASES[cid]
    pl, buf = CM.model(cid, C)
    assert buf.size == pl.dst_len + SD.GUARD
    assert SD.clerk_slices(buf, pl) == oracle.snapshot_transpose(case.blobs())
    outside = ~SD.blob_mask(pl, buf.size)
    assert outside[pl.dst_len:].all() and outside.sum() >= SD.GUARD + 16 * case.n
    assert (buf[outside] == SD.fill_pattern(buf.size)[outside]).all(), "the model wrote outside the blobs"
    assert all(b % 16 == 0 for b in pl.clerk_base)


@pytest.mark.parametrize("cid", CM.IDS)
def test_case_contains_what_it_states(cid):
    """the (shift, dst start mod 16, len) triples, read back from plan()'s blob list"""
    case = CASES[cid]
    pl = CM.model(cid, C)[0]
    assert case.claims <= _triples(pl), sorted(case.claims - _triples(pl))
    if case.family in "QLC":
        mine = _target_blobs(case, pl)
        assert mine and {(s - d) & 15 for s, d, _ in mine} == {case.shift}
        assert pl.record[4] >> case.shift & 1
    if case.family == "W":
        assert tuple(_n_chunks(b) for b in pl.blobs) == case.chunk_counts
    assert int(case.part_off()[-1]) + 32 == case.src().size <= 512 * 1024


# ---------------------------------------------------------------- coverage, written out
def _union(family):
    out = set()
    for cid, case in CASES.items():
        if case.family == family:
            out |= _triples(CM.model(cid, C)[0]) & case.claims
    return out


def test_coverage_Q():
    want = set()
    for s in range(16):
        for r in range(16):
            lens = {1, 16 - r, 16, 17, CM.head_quad_tail_len(r), 31, 32, 33, 47, 48, 49}
            if r >= 2:
                lens.add(CM.straddle_len(r))         # no length below 16 straddles two quads from r = 0 or 1
            if r <= 13:
                lens.add(15 - r)
            want |= {(s, r, L) for L in lens}
    assert _union("Q") == want
    # what the lengths are there for, from the chunk's own geometry
    for r in range(16):
        a, A, E, e = SD.chunk_geometry((0, r, 16 - r), 0, C)
        assert (a, e) == (r, 16) and ((A == E == e) if r else (A, E) == (0, 16))   # a head up to the quad's end
        if 1 <= r <= 13:
            a, A, E, e = SD.chunk_geometry((0, r, 15 - r), 0, C)
            assert (a + 15) & ~15 > e & ~15 and A == E == e == 15        # the A > E collapse
        if r >= 2:
            L = CM.straddle_len(r)
            a, A, E, e = SD.chunk_geometry((0, r, L), 0, C)
            assert L < 16 and a < A == E == 16 < e                       # head and tail, no body
        a, A, E, e = SD.chunk_geometry((0, r, CM.head_quad_tail_len(r)), 0, C)
        assert E - A == 16 and e > E and (a < A) == (r > 0)


def test_coverage_C():
    lens = CM.c_lengths(C)
    assert sorted(lens) == sorted(["C-17", "C-16", "C-1", "C", "C+1", "C+15", "C+16", "C+17", "2C-1", "2C", "2C+1",
                                   "4C+1"])
    want = {(s, 0, L) for s in range(16) for L in lens.values()}
    want |= {(s, r, L) for s in (0, 1, 8, 15) for r in (1, 15) for L in lens.values()}
    assert _union("C") == want


def test_coverage_L():
    got = set()
    for cid, case in CASES.items():
        if case.family != "L":
            continue
        pl = CM.model(cid, C)[0]
        for b in _target_blobs(case, pl):
            key = ((b[0] - b[1]) & 15, b[1] & 15)
            got |= {key + (_body_quads(b, k),) for k in range(_n_chunks(b))}
        assert case.quads <= got
    counts = (1, 255, 256, 257, 2047, 2048)
    want = {(0, 0, q) for q in counts} | {(7, 5, q) for q in counts[:-1]} | {(9, 0, q) for q in counts}
    assert want <= got
    assert set().union(*(c.quads for c in CASES.values() if c.family == "L")) == want
    # from dst start 5 no chunk holds 2048 whole quads; the chunk boundary cuts the last one into tail and head
    pl = CM.model("L-s7-d5", C)[0]
    big = max(_target_blobs(CASES["L-s7-d5"], pl), key=lambda b: b[2])
    assert [_body_quads(big, k) for k in range(_n_chunks(big))] == [2047, 0]


def _events(case, pl):
    """the named walk events the case's plan shows, by walk()"""
    cs, ev = pl.chunk_start, set()
    for w in range(pl.grid):
        pairs = SD.walk(pl, w)
        lo = SD.wg_range(cs[-1], pl.grid, w)[0]
        b0, k0 = pairs[0]
        n0 = cs[b0 + 1] - cs[b0]
        assert cs[b0] <= lo < cs[b0 + 1] and k0 == lo - cs[b0]
        if n0 >= 3 and 0 < k0 < n0 - 1:
            ev.add("first_chunk_mid_blob")
        if n0 >= 2 and k0 == n0 - 1:
            ev.add("first_chunk_last_of_blob")
        for i in (1, 2, 3):
            if i < len(pairs) and pairs[i][0] != pairs[i - 1][0]:
                ev.add(f"switch_at_step_{i}")
        if sum(1 for b, _ in pairs if cs[b + 1] - cs[b] == 1) >= 4:
            ev.add("four_one_chunk_blobs_in_a_walk")
        if b0 == 0:
            ev.add("search_lands_on_blob_0")
        if b0 == len(pl.blobs) - 1:
            ev.add("search_lands_on_last_blob")
        if w and cs[b0] == lo:
            ev.add("search_lands_on_exact_start")
        if cs[b0] < lo:
            ev.add("search_lands_inside_a_blob")
    return ev


def test_coverage_W():
    seen, totals, sizes = set(), set(), set()
    for cid, case in CASES.items():
        if case.family != "W":
            continue
        pl = CM.model(cid, C)[0]
        ev = _events(case, pl)
        assert set(case.events) <= ev, (cid, sorted(set(case.events) - ev))
        print(f"{cid}: chunks per blob {case.chunk_counts}, grid {pl.grid}: {', '.join(sorted(ev))}")
        seen |= set(case.events)
        totals.add(pl.chunk_start[-1])
        sizes |= {hi - lo for lo, hi in SD.wg_ranges(pl.chunk_start[-1], pl.grid)}
        # every chunk of every blob exactly once over the grid
        pairs = [p for w in range(pl.grid) for p in SD.walk(pl, w)]
        assert pairs == [(b, k) for b, blob in enumerate(pl.blobs) for k in range(_n_chunks(blob))]
    assert seen == set(CM.W_EVENTS)
    assert totals == {1, 2, 3, 4, 5, 7, 8, 9, 13}
    assert sizes == {1, 2, 3, 4}                     # 3- and 4-chunk workgroups mix (7, 13); 1, 2: the small totals
    for total in (7, 13):
        assert {hi - lo for lo, hi in SD.wg_ranges(total, SD.grid_for(total))} == {3, 4}


def test_coverage_Z():
    seen = set()
    for cid, case in CASES.items():
        if case.family != "Z":
            continue
        L = np.array(case.lens)
        pl = CM.model(cid, C)[0]
        have = set()
        for c in range(case.n):
            col = L[:, c]
            nz = np.flatnonzero(col)
            if len(nz) == 0:
                have.add("whole_clerk_empty")
                base = pl.clerk_base[c]
                end = pl.clerk_base[c + 1] if c + 1 < case.n else pl.dst_len
                assert end - base == 16              # its job is the 16 bytes of padding
                continue
            if col[0] == 0:
                have.add("first_blob_of_a_clerk_empty")
            if col[-1] == 0:
                have.add("last_blob_of_a_clerk_empty")
            if any(b - a >= 3 for a, b in zip(nz, nz[1:])):
                have.add("run_of_empties_between")   # at least two empties in a row between non-empty blobs
        if not L.any():
            have.add("every_blob_empty")
            assert pl.record == (0, 0, 0, C, 0) and pl.grid == 0
        if L.shape == (1, 1):
            have.add("P1_n1")
        assert set(case.shapes) <= have, (cid, have)
        assert len(pl.blobs) == int((L > 0).sum())
        seen |= set(case.shapes)
    assert seen == set(CM.Z_SHAPES)
    assert CASES[CM.ALL_EMPTY].shapes and not np.array(CASES[CM.ALL_EMPTY].lens).any()


def test_family_counts():
    fam = {}
    for case in CASES.values():
        fam[case.family] = fam.get(case.family, 0) + 1
    assert fam == {"Q": 16, "L": 3, "C": 48, "W": 10, "Z": 5}
    print(f"{len(CASES)} cases: {fam}")


# ---------------------------------------------------------------- the record
@pytest.mark.parametrize("cid", CM.IDS)
def test_predicted_record_is_self_consistent(cid):
    pl = CM.model(cid, C)[0]
    blobs, chunks, grid, chunk_bytes, shifts = pl.record
    assert chunk_bytes == C and blobs == len(pl.blobs) and chunks == pl.chunk_start[-1]
    assert (bin(shifts).count("1") >= 1) == (blobs > 0) and shifts < 1 << 16
    assert grid == (chunks + 3) // 4 == pl.grid
    assert chunks == sum(_n_chunks(b) for b in pl.blobs) and (chunks > 0) == (blobs > 0)
    ranges = SD.wg_ranges(chunks, grid)
    assert [lo for lo, _ in ranges] + [chunks] == [0] + [hi for _, hi in ranges] if grid else chunks == 0
    assert all(chunks // grid <= hi - lo <= min(4, -(-chunks // grid)) for lo, hi in ranges)


# ---------------------------------------------------------------- fault injection
def _catches(fault, cid):
    case = CASES[cid]
    bad = SD.transpose_model(case.src(), case.part_off(), case.P, case.n, fault=fault, C=C)
    return not np.array_equal(bad, CM.model(cid, C)[1])


def fault_table(first_only=True):
    """fault -> the cases whose full dst buffer (guard bytes included) it changes, the smaller sources first"""
    order = sorted(CM.IDS, key=lambda cid: int(CASES[cid].part_off()[-1]))
    table = {}
    for fault in SD.FAULTS:
        table[fault] = []
        for cid in order:
            if _catches(fault, cid):
                table[fault].append(cid)
                if first_only:
                    break
    return table


def test_every_fault_is_caught_by_some_case():
    assert len(SD.FAULTS) == len(set(SD.FAULTS)) == 9
    table = fault_table()
    for i, fault in enumerate(SD.FAULTS, 1):
        print(f"fault {i} {fault}: caught by {table[fault][0] if table[fault] else 'NO CASE'}")
    holes = [f for f, caught in table.items() if not caught]
    assert not holes, f"no case of the matrix notices: {holes}"


def test_faults_are_caught_where_they_are_aimed():
    """each fault against a case built for the arithmetic it breaks (the table above takes the smallest source)"""
    aimed = {"tail_drops_last_byte": "Q-s0", "body_guard_le": "L-s7-d5", "head_le": "Q-s5",
             "body_shift_mod4": "Q-s12", "later_chunks_minus16": "C-s3-d0-b", "walk_stuck_on_one_chunk": "W-13b",
             "search_first_ge": "W-7", "tail_stale_blob": "Z-mixed", "tail_lanes_16_31": "Q-s9"}
    assert sorted(aimed) == sorted(SD.FAULTS)
    for fault, cid in aimed.items():
        assert _catches(fault, cid), (fault, cid)


# ---------------------------------------------------------------- the grid cap
def test_grid_cap_is_arithmetic_only():
    """launch_snapshot_transpose gives each workgroup more than 4 chunks once total / 4 would reach 2^31 - 1
    workgroups.  The smallest such total is 4 * (2^31 - 1) chunks, 256 TiB of payload at 32 KiB a chunk: this branch
    cannot be run on a device, so it is checked here as arithmetic alone, in the kernel's wrapping 64-bit terms.
    The kernel forms total * (w + 1): on the capped grid alone that product wraps from about 6 * 2^31 chunks on
    (the ranges at 2^40 chunks then neither partition nor stay inside the plan), so the launcher also keeps
    grid * total below 2^64."""
    cap = 4 * (2 ** 31 - 1)
    for total in (cap - 1, cap, cap + 4, 6 * 2 ** 31, 2 ** 40, 2 ** 63 + 5):
        G = SD.grid_for(total)
        assert 0 < G < 2 ** 32 and G <= total
        assert G == (total + 3) // 4 if total < cap else total * G < 2 ** 64
        rng = np.random.default_rng(total % 1000)
        ws = sorted(w for w in {0, 1, 2, G // 2, G - 3, G - 2, G - 1, *map(int, rng.integers(0, G, 2000))}
                    if 0 <= w < G)
        assert SD.wg_range(total, G, 0)[0] == 0 and SD.wg_range(total, G, G - 1)[1] == total
        per = -(-total // G)
        for w in ws:
            lo, hi = SD.wg_range(total, G, w)
            assert (lo, hi) == (total * w // G, total * (w + 1) // G)    # the exact quotients: the ranges partition
            assert 0 < hi - lo <= per
            if w + 1 < G:
                assert SD.wg_range(total, G, w + 1)[0] == hi
    # without the second bound the product does wrap: the capped grid alone at 6 * 2^31 and at 2^40 chunks
    for total in (6 * 2 ** 31, 2 ** 40):
        capped = -(-total // (total // 0x7FFFFFFF + 1))
        assert capped < 2 ** 32 and total * capped >= 2 ** 64 and SD.grid_for(total) < capped
        lo, hi = SD.wg_range(total, capped, capped - 1)
        assert hi != total
    assert cap * SD.grid_for(cap) < 2 ** 64 and SD.grid_for(cap + 4) == -(-(cap + 4) // 5)


if __name__ == "__main__":                           # the full table (every catching case), for the evidence file
    fam = {}
    for case in CASES.values():
        fam[case.family] = fam.get(case.family, 0) + 1
    print(f"{len(CASES)} cases: {fam}")
    for i, (fault, caught) in enumerate(fault_table(first_only=False).items(), 1):
        by = {}
        for cid in caught:
            by.setdefault(CASES[cid].family, []).append(cid)
        print(f"fault {i} {fault}: {len(caught)} cases -- " +
              "; ".join(f"{f}: {len(v)} (first {v[0]})" for f, v in sorted(by.items())))
