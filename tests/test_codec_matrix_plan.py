"""CPU: the plan of tests/test_gpu_codec_matrix.py against the bytes of its payloads and against the codec
instantiations in the built library (scripts/code_objects.py, kernel names only).

Every varint_decode_kernel / slot_combine_kernel / varint_decode_combine_kernel / varint_write_kernel instantiation
that ships must be the kernel tests/codec_dispatch.py predicts for at least one planned case, and no case may predict
a name the library lacks.  The record each case states is recomputed here from its payload bytes, and the edge each
section is there for is asserted on those bytes: a case that stops exercising its edge fails without a GPU.
"""
import importlib.util
import os

import numpy as np
import pytest

from sda_amd import engine as E
from tests import codec_dispatch as CD
from tests import codec_matrix_cases as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

FAMILIES = ("varint_decode_kernel<", "slot_combine_kernel<", "varint_decode_combine_kernel<", "varint_write_kernel<")


def _job(case):
    buf, off, rows = case.job()
    return CD.Job(np.frombuffer(buf, np.uint8), off), rows


@pytest.fixture(scope="module")
def predictions():
    """{case id: (record, kernels)} from the bytes"""
    return {c.id: CD.predict(_job(c)[0], c.m, c.env()) for c in CM.COMBINE_CASES}


@pytest.fixture(scope="module")
def shipped():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    names = {k["pretty"] for k in CO.kernels(E.LIB_PATH) if k["pretty"].startswith(FAMILIES)}
    assert len(names) >= 18, "the fat binary parser found too few codec kernels"
    return names


def _planned(predictions):
    names = {k for _, kernels in predictions.values() for k in kernels}
    return names | {c.kernel for c in CM.DECODE_CASES} | {c.kernel for c in CM.ENCODE_CASES}


def test_case_ids_are_unique_and_knobs_known():
    ids = [c.id for c in CM.COMBINE_CASES + CM.DECODE_CASES + CM.ENCODE_CASES]
    assert len(ids) == len(set(ids))
    for c in CM.COMBINE_CASES + CM.DECODE_CASES + CM.ENCODE_CASES:
        assert set(c.env()) <= set(CM.KNOBS), c.id


def test_every_shipped_instantiation_is_claimed_by_a_case(shipped, predictions):
    unclaimed = sorted(shipped - _planned(predictions))
    assert not unclaimed, f"instantiations no case of the matrix runs: {unclaimed}"


def test_no_case_predicts_a_kernel_the_library_lacks(shipped, predictions):
    invented = sorted(_planned(predictions) - shipped)
    assert not invented, f"predicted kernels missing from the library: {invented}"


def test_stated_records_follow_from_the_bytes(predictions):
    """the record a case states (by its section's rule) is the one the dispatcher's rules give for its payloads"""
    wrong = [(c.id, c.record, predictions[c.id][0]) for c in CM.COMBINE_CASES if predictions[c.id][0] != c.record]
    assert not wrong, wrong[:10]


def test_payloads_decode_to_one_dimension():
    for c in CM.COMBINE_CASES:
        job, rows = _job(c)
        if not job.irregular().any():                      # (an irregular blob's count is the sequential decoder's)
            assert (job.counts == rows.shape[1]).all() and job.n == rows.shape[0], c.id


def test_section_a_covers_the_slot_combine(predictions):
    a = [c for c in CM.COMBINE_CASES if c.section == "a"]
    plain = [c for c in a if c.record[0] == CD.SLOTS and c.knobs]
    assert {(c.record[1], c.m, c.args[1], c.args[2]) for c in plain} == \
        {(cpl, m, n, d) for cpl in (1, 2, 4) for m in CM.SLOT_MODULI for n in CM.SLOT_BLOBS for d in CM.slot_dims(cpl)}
    assert any(not c.knobs and c.record == (CD.SLOTS, 4, 0, 1) for c in a)
    assert {(c.record[1], c.record[3]) for c in a if c.record[0] == CD.SLOTS_GROUPED} == {(1, 17), (1, 6), (2, 17), (2, 6)}
    for c in plain:
        # SMALL_M follows m <= 2^62 on either side of the edge
        small = "true" if c.m <= 2**62 else "false"
        assert predictions[c.id][1][-1] == f"slot_combine_kernel<{c.record[1]}, 8, {small}>", c.id
        # every share fits int32 and, wherever the rows have room for them, the planted values are there
        _, rows = _job(c)
        assert rows.min() >= -(2**31) and rows.max() <= 2**31 - 1, c.id
        if rows.size >= 4:
            assert rows.min() == -(2**31) and rows.max() == 2**31 - 1, c.id
            if c.m - 1 < 2**31:
                assert (rows == c.m - 1).any() and (rows == -(c.m - 1)).any(), c.id


@pytest.mark.parametrize("cpl", [2, 4])
def test_section_a_straddling_lane_takes_every_residue(cpl):
    """over the 9000-wide cases of a CPL, the c0 of the tiles that continue into a next region takes every residue
    mod CPL: the lane that straddles the region gap loads twice and merges at every position"""
    seen, most = set(), 0
    for c in CM.COMBINE_CASES:
        if c.section == "a" and c.record[1] == cpl and c.args[2] == 9000:
            job, _ = _job(c)
            most = max(most, job.max_region_count())
            seen |= {c0 % cpl for _, _, c0, n in job.slot_c0(cpl * CD.THREADS) if c0 < n}
    assert seen == set(range(cpl)) and most <= CD.SLOT_CAP, (seen, most)


def test_section_b_inputs_raise_the_flag_they_name():
    jobs = {c.name: _job(c)[0] for c in CM.COMBINE_CASES if c.section == "b"}
    assert len(jobs) == 7
    six, two31 = jobs["six_bytes"], jobs["two31"]
    assert six.length.max() == 6 and not six.irregular().any() and six.max_region_count() <= CD.SLOT_CAP
    assert two31.length.max() == 5 and two31.fifth_group().max() == 16 and two31.max_region_count() <= CD.SLOT_CAP
    assert jobs["cap_4097"].max_region_count() == 4097 and jobs["cap_4097"].fits_int32()
    blob, _, cnt = jobs["cap_4096"].region_counts()
    assert (cnt == 4096).all() and set(jobs["cap_4096"].length) == {4} and not jobs["cap_4096"].slot_wide()
    assert jobs["irregular"].irregular().tolist() == [False, False, True, False, False]
    assert not jobs["matrix_wide"].fits_int32() and jobs["narrow0"].fits_int32()


def test_section_c_rings_are_shorter_at_and_longer_than_the_job():
    c = [x for x in CM.COMBINE_CASES if x.section == "c"]
    fused = {(x.record[1], x.args[2], x.args[3], x.args[1]) for x in c if x.record[0] == CD.FUSED}
    assert fused == {(d, n, dim, k) for d in CM.FUSED_DEPTHS for n in CM.FUSED_BLOBS for dim in CM.FUSED_DIMS
                     for k in ("field", "onebyte")}
    for d in CM.FUSED_DEPTHS:                              # fewer blobs than the ring, whole rings, a ring and a tail
        ns = {n for dd, n, _, _ in fused if dd == d}
        assert any(n < d for n in ns) and any(n % d == 0 for n in ns) and any(n > d and n % d for n in ns)
    multi = [x for x in c if x.record[0] == CD.FUSED_MULTI]
    assert {(x.env()["SDA_DC_DEPTH"], x.args[2], x.args[3]) for x in multi} == \
        {(str(d), n, dim) for d in CM.FUSED_DEPTHS for n in CM.MULTI_BLOBS for dim in CM.FUSED_DIMS}
    assert all(x.record[1] == 2 for x in multi)
    for x in multi[:3]:
        job, _ = _job(x)
        assert job.long().all() and set(job.length) == {10}


def test_section_d_has_two_grid_slices():
    buf, off, rows = CM.big_job()
    assert len(off) - 1 == 65_538 > CD.GRID_Y and rows.shape == (65_538, 5) and CD.slices(65_538) == 2
    job = CD.Job(np.frombuffer(buf, np.uint8), off)
    assert (job.counts == 5).all() and not job.slot_wide()
    buf, off, picked = CM.big_decode_job()
    job = CD.Job(np.frombuffer(buf, np.uint8), off)
    irr = job.irregular()
    assert irr[65_536] and irr.sum() == 1 and job.counts[65_537] == 6
    assert picked[65_536].size == 3 + 2 and picked[65_537].size == 6 and len(picked) >= 60
    assert {0, 65_534, 65_535, 65_536, 65_537} <= set(picked)


def test_section_e_scans_carry():
    buf, off, rows = CM.carry_job()
    job = CD.Job(np.frombuffer(buf, np.uint8), off)
    assert (job.blob_regions() > CD.THREADS).all() and job.n == 3, job.blob_regions()
    assert not job.slot_wide()
    shapes = {(c.rows, c.length, c.stride) for c in CM.ENCODE_CASES}
    assert len(CM.ENCODE_CASES) == 6 and len(shapes) == 3
    assert any(r > CD.THREADS for r, _, _ in shapes)                                  # varint_rows_kernel's carry
    assert any(-(-n // CD.ENC_CHUNK) > CD.THREADS and n % CD.ENC_CHUNK for _, n, _ in shapes)   # varint_offsets_kernel's
    # two rows whose second starts 8 bytes off a 16-byte boundary (the first, and full chunks, take the paired loads)
    assert any(r == 2 and s > n and (s * 8) % 16 == 8 for r, n, s in shapes)
    for c in CM.ENCODE_CASES:
        v = CM.encode_values(c.seed, c.rows, c.length, c.stride)
        sizes = {len(CM.O.varint_encode(v[0, i:i + 1])) for i in range(min(c.length, 400))}
        assert sizes == set(range(1, 11)) or c.length < 100, (c.id, sizes)
    assert {c.kernel for c in CM.ENCODE_CASES} == {"varint_write_kernel<true>", "varint_write_kernel<false>"}


def _near(pos, period, skip=None):
    """signed distances of the positions to their nearest multiple of `period` (not a multiple of `skip`)"""
    edge = (pos + period // 2) // period * period
    keep = np.ones(pos.size, bool) if skip is None else edge % skip != 0
    return set((pos - edge)[keep].tolist())


def test_section_g_sweep_reaches_every_edge_offset():
    buf, off, rows = CM.sweep_job()
    job = CD.Job(np.frombuffer(buf, np.uint8), off)
    span = set(range(-CM.EDGE_SPAN, CM.EDGE_SPAN + 1))
    assert (job.counts == CM.SWEEP_DIM).all() and rows.shape == (job.n, CM.SWEEP_DIM) and not job.slot_wide()
    begins, ends = job.off[:-1], job.off[1:]
    assert span <= _near(begins, CD.REGION) and span <= _near(ends, CD.REGION)
    assert span <= _near(begins, CD.SUB_REGION, CD.REGION) and span <= _near(ends, CD.SUB_REGION, CD.REGION)
    # elements straddling a region edge: (length, bytes before the edge)
    edge = job.term_pos // CD.REGION * CD.REGION
    cross = job.start_pos < edge
    splits = set(zip(job.length[cross].tolist(), (edge - job.start_pos)[cross].tolist()))
    assert set(CM.SWEEP_SPLITS) <= splits, sorted(set(CM.SWEEP_SPLITS) - splits)


def test_section_g_long_sweep_splits_and_truncated_tail():
    buf, off, rows = CM.long_sweep_job()
    job = CD.Job(np.frombuffer(buf, np.uint8), off)
    assert not job.irregular().any() and job.length.max() == 11 and (job.counts == [r.size for r in rows]).all()
    edge = job.term_pos // CD.REGION * CD.REGION
    cross = job.start_pos < edge
    splits = set(zip(job.length[cross].tolist(), (edge - job.start_pos)[cross].tolist()))
    assert set(CM.LONG_SPLITS) <= splits, sorted(set(CM.LONG_SPLITS) - splits)
    raw = np.frombuffer(buf, np.uint8)
    tails = [b for b in range(job.n) if off[b + 1] > off[b] and raw[off[b + 1] - 1] >= 0x80]
    assert len(tails) == 1 and off[tails[0] + 1] % CD.REGION == 0 and (raw[off[tails[0] + 1] - 3:off[tails[0] + 1]] >= 0x80).all()
    assert (job.counts == 0).sum() == 1
    assert set(np.unique(job.length)) >= set(range(1, 12))


def test_section_f_names_both_store_kinds_of_every_decode():
    names = {c.kernel for c in CM.DECODE_CASES if c.section == "f"}
    for c in CM.COMBINE_CASES:
        if c.section == "f":
            names |= {k for k in CM.combine_kernels(c) if k.startswith("varint_decode_kernel<")}
    assert names == {f"varint_decode_kernel<{t}, {s}, {nt}>" for t, s in (("long", "false"), ("int", "false"), ("int", "true"))
                     for nt in ("true", "false")}
