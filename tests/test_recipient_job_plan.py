"""CPU: the plan of tests/test_gpu_recipient_job.py (tests/recipient_job_cases.py) held against

  * the two references: for every case the blobs are decoded by the oracle, and on those rows the step-wise flow over
    the C oracle equals the big-integer model (tests/pipeline_model.py), wherever the oracle's domain covers the case;
  * the host form's checks (tests/pipeline_dispatch.py): a derived case expects exactly what its row of
    tests/pipeline_matrix_cases.py expects of sda_recipient_reveal, status and output;
  * the seed rule (first 8 values, `as u32`, zero padded) against the oracle's ChaCha mask combine;
  * the new record: every route value is taken by some case;
  * the library: the three symbols exist, and the shapes the case file promises are really there.
No GPU.
"""
import ctypes as C
import os

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import pipeline_dispatch as PD
from tests import pipeline_matrix_cases as PC
from tests import pipeline_model as PM
from tests import recipient_job_cases as RJ
from tests.test_pipeline_matrix_plan import ENGINE_ONLY, RECIPIENT_OUTSIDE_ORACLE, _oracle_recipient

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [c.id for c in RJ.CASES]


def _model(case):
    masks, indexed = RJ.rows(case)
    try:
        return PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, case.mode), None
    except PM.ModelError as e:
        return None, (e.status, e.cls)


@pytest.mark.parametrize("case", RJ.CASES, ids=IDS)
def test_job_case_on_the_decoded_rows(case):
    masks, indexed = RJ.rows(case)
    want = RJ.expected_status(case)
    model, model_status = _model(case)
    if case.base is not None:
        # the payload form of a matrix row: the oracle decodes exactly the host rows, and the call is expected to
        # end as sda_recipient_reveal's
        assert (masks, indexed) == tuple(PC.host_rows(case.base))
        assert want == PC.recipient_expected_status(case.base, "host")
        assert RJ.out_len(case) == case.base.D or want is not None
    if want is not None and want[1] in ENGINE_ONLY:
        return                                     # the C ABI's own checks: neither reference has an opinion
    assert model_status == want
    if want is None:
        assert len(model) == RJ.out_len(case)
    if case.base is not None and case.base.id in RECIPIENT_OUTSIDE_ORACLE:
        return
    try:
        oracle, oracle_status = _oracle_recipient(case, masks, indexed, case.mode), None
    except E.SdaError as e:
        oracle, oracle_status = None, e.status
    assert oracle_status == (want[0] if want else None)
    assert oracle == model


def test_blobs_are_the_oracles_encoding_behind_junk(oracle):
    case = next(c for c in RJ.CASES if c.id.startswith("cross-add2"))
    mask_blobs, indexed = RJ.blobs(case)
    buf, off = RJ.layout([b for _, b in indexed])
    assert off[0] == RJ.LEAD and len(buf) == off[-1] + 32
    for k, (_, b) in enumerate(indexed):
        assert buf[off[k]:off[k + 1]] == b
        assert len(b) == 5 * RJ.CROSS > RJ.REGION                  # five bytes a value: past a decode region
    assert all(len(b) > RJ.REGION for b in mask_blobs)
    cp = next(c for c in RJ.CASES if c.id.startswith("cross-cp"))
    assert all(len(b) == 5 * (RJ.CROSS + 1) for _, b in RJ.blobs(cp)[1])


def test_seed_rule_agrees_with_the_oracles_mask_combine(oracle):
    """first 8 values, `as u32`, zero padded -- on the decoded seeds of every ChaCha case"""
    seen_lens, seen_wide, seen_neg = set(), False, False
    for case in RJ.CASES:
        if not isinstance(case.ms, S.ChaChaMasking) or RJ.expected_status(case) is not None:
            continue
        masks, _ = RJ.rows(case)
        if not masks or case.ms.dimension == 0:
            continue
        D = min(case.ms.dimension, 64)
        key = np.zeros((len(masks), 8), np.int64)
        for i, r in enumerate(masks):
            seen_lens.add(len(r))
            seen_wide |= any(v >= 2**32 for v in r)
            seen_neg |= any(v < 0 for v in r)
            for j, v in enumerate(r[:8]):
                key[i, j] = v & 0xFFFFFFFF
        want = [int(v) for v in oracle.chacha_mask_combine(case.ms.modulus, D, key)]
        assert PM.chacha_mask_combine(case.ms.modulus, D, [list(r)[:8] for r in masks]) == want, case.id
    assert set(RJ.SEED_LENS) <= seen_lens and seen_wide and seen_neg


def test_malformed_seed_blobs_decode_by_the_codecs_rules(oracle):
    case = next(c for c in RJ.CASES if c.id == "seeds-malformed-D257")
    long_run, cut, cut_long, only_runs = RJ.rows(case)[0]
    assert len(long_run) == 3 and long_run[1:] == [-3, 135]         # the 11-byte run is one element
    assert cut == [2, 3, -3]                                          # 0x85 alone: the partial value 5 -> -3
    assert len(cut_long) == 2 and cut_long[0] == 1
    assert len(only_runs) == 3                                        # 11 + 11 + 1 continuation bytes


def test_every_route_of_the_new_record_is_taken():
    job = set()
    for case in RJ.CASES:
        if RJ.expected_status(case) is None and RJ.out_len(case):
            for form in ("host", "dev"):
                job.add(RJ.expected_records(case, form)[0][:2])
            job.add(RJ.expected_records(case, "host", multi=True)[0][:2])
    assert {r[0] for r in job} == {RJ.MASK_NONE, RJ.MASK_FULL_COMBINED, RJ.MASK_FULL_STREAMED, RJ.MASK_CHACHA,
                                   RJ.MASK_CHACHA_SPLIT}
    assert {r[1] for r in job} == {RJ.SHARE_ADDITIVE, RJ.SHARE_PACKED}
    assert (E.RECIPIENT_JOB_MASK_NONE, E.RECIPIENT_JOB_MASK_FULL_COMBINED, E.RECIPIENT_JOB_MASK_FULL_STREAMED,
            E.RECIPIENT_JOB_MASK_CHACHA, E.RECIPIENT_JOB_MASK_CHACHA_SPLIT) == (0, 1, 2, 3, 4)
    assert (E.RECIPIENT_JOB_SHARE_ADDITIVE, E.RECIPIENT_JOB_SHARE_PACKED) == (1, 2)


def test_the_promised_shapes_are_there():
    by_group = {}
    for c in RJ.CASES:
        by_group.setdefault(c.group, []).append(c)
    counts = {len(RJ.rows(c)[1]) for c in by_group["counts"]}
    assert counts == set(RJ.CLERK_COUNTS)
    assert {RJ.out_len(c) for c in by_group["counts"]} == set(PC.ELEMENTWISE_D)
    assert {len(RJ.rows(c)[0]) for c in by_group["seeds"]} >= set(RJ.SEED_COUNTS)
    for ss in (PC.FL, PC.CP):
        for L in PC.packed_dims(ss):
            B = PD.batches(ss, L)
            mine = [c for c in by_group["packed"] if c.ss is ss and c.dimension == L]
            lens = [sorted(len(r) for _, r in RJ.rows(c)[1]) for c in mine]
            assert any(l[0] == l[-1] == B for l in lens)
            assert any(l[0] >= B and l[-1] > B and len(set(l)) > 1 for l in lens)
            short = [c for c, l in zip(mine, lens) if l[0] == B - 1]
            assert short and all(RJ.expected_status(c) == (PD.PRECONDITION, "index out of bounds") for c in short)
    late = by_group["late"][0]
    assert RJ.expected_records(late, "dev")[1][4] == 2
    # the masking moduli of the matrix, negative ones included, reach the job through the derived cases
    q = {c.ms.modulus for c in RJ.DERIVED if isinstance(c.ms, S.FullMasking)}
    assert set(PC.MODULI) | set(PC.NEGATIVE_MODULI) <= q
    derived_status = [c for c in RJ.DERIVED if c.base.group == "status"]
    assert any(RJ.expected_status(c) == (PD.INVALID_ARGUMENT, "output buffer too small") for c in derived_status)
    assert {f[4] for f in RJ.FAULTS} == {RJ.ALIGN, RJ.OFFSETS, RJ.NULL}


def test_the_library_exports_the_job():
    lib = E.load_library()
    for name in ("sda_recipient_job", "sda_recipient_job_dev", "sda_recipient_job_last_launch"):
        assert hasattr(lib, name), name
    header = open(os.path.join(os.path.dirname(HERE), "include", "sda_engine.h")).read()
    assert header.count("sda_status sda_recipient_job") == 3
    v = [C.c_uint32() for _ in range(3)]
    assert lib.sda_recipient_job_last_launch(None, *[C.byref(x) for x in v]) == E.ERR_INVALID_ARGUMENT
    assert all(hasattr(E.Engine, n) for n in ("recipient_job", "recipient_job_dev", "recipient_job_last_launch"))


def test_no_case_is_left_out_skipped_or_expected_to_fail():
    src = open(os.path.join(HERE, "test_gpu_recipient_job.py")).read()
    assert "skip" not in src.replace("importorskip", "") and "xfail" not in src
    assert "RJ.CASES" in src and "RJ.FAULTS" in src
    assert len(set(IDS)) == len(IDS)
