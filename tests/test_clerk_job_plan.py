"""CPU: the case tables of the clerk job (tests/clerk_job_cases.py) and its Python-integer model.

The model -- fold tile after tile from the carried state, then zigzag-LEB128 the result -- is held against
oracle.combine over all blobs and oracle.varint_encode for every case and split; the tables are held against the
boundaries their comments name; and the model shows that the inputs can tell a wrong continuation from a right
one: a split that restarted from 0, or that canonicalised the carried state, changes at least one column."""
import numpy as np
import pytest

from tests import clerk_job_cases as CJ
from tests import codec_dispatch as CD

CASES = CJ.cases()


def test_the_matrix_covers_every_value_the_plan_lists():
    assert sorted({m for m, _, _ in CASES}) == sorted(CJ.MODULI) == sorted((433, 2147482801, 2**62, 2**62 + 1, 2**63 - 1))
    assert sorted({d for _, _, d in CASES}) == [1, 1023, 1024, 1025, 2047, 2048, 2049, 3276, 3278, 4097]
    assert sorted({n for _, n, _ in CASES}) == [1, 7, 8, 9, 17]
    for n in CJ.BLOBS:                      # every count with every modulus, and with every dimension
        assert {m for m, k, _ in CASES if k == n} == set(CJ.MODULI)
    for d in CJ.DIMS:
        assert {n for _, n, k in CASES if k == d} == set(CJ.BLOBS)


def test_splits():
    assert CJ.splits(1) == [(1,)]
    for n in (7, 8, 9, 17):
        sp = CJ.splits(n)
        assert sp[:3] == [(n,), (1, n - 1), (n - 1, 1)] and len(sp) == 4 and len(sp[3]) == 3
        assert all(sum(s) == n and min(s) >= 1 for s in sp)
        cuts = [sum(sp[3][:i]) for i in (1, 2)]
        assert any(c % 8 for c in cuts), "the three tiles cut inside a group of 8"
    assert 8 < sum(CJ.splits(17)[3][:2]) < 16       # and once inside the second group


def test_every_dimension_lands_where_its_comment_says():
    assert CJ.SLOT_TILE == 4 * CD.THREADS and CJ.ENC_CHUNK == CD.ENC_CHUNK and CJ.REGION == CD.REGION
    assert 5 * (CJ.REGION_CROSS_FROM - 1) <= CJ.REGION < 5 * CJ.REGION_CROSS_FROM
    for dim, (tiles, chunks, crosses) in CJ.DIMS.items():
        assert -(-dim // CJ.SLOT_TILE) == tiles, dim
        assert -(-dim // CJ.ENC_CHUNK) == chunks, dim
        assert (5 * dim > CJ.REGION) == crosses == (dim >= CJ.REGION_CROSS_FROM), dim
    d = sorted(CJ.DIMS)
    for edge in (CJ.SLOT_TILE, CJ.ENC_CHUNK):
        assert {edge - 1, edge, edge + 1} <= set(d)
    assert CJ.REGION_CROSS_FROM - 1 in d and CJ.REGION_CROSS_FROM + 1 in d and 2 * CJ.ENC_CHUNK + 1 in d


def test_a_five_byte_blob_crosses_the_region_where_the_table_says(oracle):
    for dim in (3276, 3278):
        blob = oracle.varint_encode(np.full(dim, CJ.M31 - 1, np.int64))
        assert len(blob) == 5 * dim
        assert (len(blob) > CJ.REGION) == CJ.DIMS[dim][2]


@pytest.mark.parametrize("m", CJ.MODULI)
def test_steered_columns_reach_the_edges_at_every_boundary(m):
    """At every blob boundary a split cuts at, the carried states of the steered columns hold +-(m - 1), +-1 and 0,
    and the blob behind the boundary brings a sum of exactly +m and of exactly -m."""
    for n in (7, 8, 9, 17):
        x = CJ.rows(m, n, 1025)
        for b in CJ.boundaries(n):
            state = CJ.fold([0] * 1025, x[:b], m)[:CJ.STEER]
            assert state == CJ.steered_states(m, n, 1025, b)
            assert {m - 1, -(m - 1), 0, 1, -1} <= set(state), (n, b, state)
            sums = {s + int(v) for s, v in zip(state, x[b][:CJ.STEER])}
            assert {m, -m} <= sums, (n, b)
    assert abs(int(CJ.rows(m, 17, 1025).min())) <= m - 1 and int(CJ.rows(m, 17, 1025).max()) <= m - 1


def test_field_cases_fit_int32_and_wide_cases_do_not():
    for m, n, dim in CASES:
        x = CJ.rows(m, n, dim)
        fits = bool((x >= -(2**31)).all() and (x < 2**31).all())
        assert fits == CJ.is_field(m), CJ.case_id((m, n, dim))


@pytest.mark.parametrize("case", CASES, ids=CJ.case_id)
def test_model_against_the_oracle_and_wrong_continuations_show(oracle, case):
    m, n, dim = case
    x = CJ.rows(m, n, dim)
    want = oracle.combine(m, x)
    want_payload = oracle.varint_encode(want)
    for split in CJ.splits(n):
        state, payload = CJ.tiled_job(x, split, m)
        assert state == want.tolist(), split
        assert payload == want_payload, split
        if len(split) == 1:
            continue
        head = x[:, :64]                    # the steered columns, the witnesses and some random ones
        assert CJ.tiled_job(head, split, m, CJ.restart)[0] != state[:64], f"a restart from 0 would not show: {split}"
        assert CJ.tiled_job(head, split, m, CJ.canonical(m))[0] != state[:64], \
            f"a canonicalised carry would not show: {split}"


@pytest.mark.parametrize("case", CASES, ids=CJ.case_id)
def test_which_cases_stay_on_the_slot_path(oracle, case):
    """The dispatch each case's one-call job must report (tests/codec_dispatch.py from the bytes): slots for the
    field moduli, so the payload is encoded by the device-length kernels, with the one exception takes_slots() names;
    the i64 matrix for the moduli past 2^31."""
    m, n, dim = case
    buf, off = CJ.layout([oracle.varint_encode(r) for r in CJ.rows(m, n, dim)])
    job = CD.Job(buf, off)
    record = CD.predict(job, m, {})[0]
    assert (record[0] == CD.SLOTS) == CJ.takes_slots(case), record
    if not CJ.is_field(m):
        assert record[0] == CD.MATRIX64
    elif not CJ.takes_slots(case):
        assert record == (CD.MATRIX32, 0, CD.FB_SLOT_WIDE, 1) and job.max_region_count() == CD.SLOT_CAP + 1
    assert int(job.counts[0]) == dim and len(set(job.counts.tolist())) == 1
