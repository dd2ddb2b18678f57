"""CPU: the plan of tests/test_gpu_pipeline_matrix.py (tests/pipeline_matrix_cases.py) held against

  * the two references: for every case the big-integer model (tests/pipeline_model.py) equals the step-wise flow over
    the C oracle (tests/oracle_backend.py), wherever the oracle's domain covers the case;
  * the pipelines' decisions (tests/pipeline_dispatch.py): every value of every decision is taken by some case, and
    every early return of both status matrices is some row's;
  * what the cases' tags promise: "representative" cases really depend on the reveal's representative, residue_only
    cases really do not, "wrap" cases really leave i64;
  * the GPU file: no case is left out, skipped or expected to fail, and its buffer check sees every word.
No GPU.
"""
import os
import re

import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import pipeline_dispatch as PD
from tests import pipeline_matrix_cases as PC
from tests import pipeline_model as PM
from tests.oracle_backend import OracleBackend

I64_MIN, I64_MAX = PD.I64_MIN, PD.I64_MAX
HERE = os.path.dirname(os.path.abspath(__file__))
GPU_FILE = os.path.join(HERE, "test_gpu_pipeline_matrix.py")


def _ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------- the oracle's domain
# The C oracle divides by the modulus it is given and restates tss for distinct points in one mode.  Outside that:
RECIPIENT_OUTSIDE_ORACLE = {
    "status-chacha-m0-masks": "gen_range(0, 0): the oracle would divide by zero",
    "status-chacha-negative-masks": "gen_range(0, m < 0): the oracle's rejection zone is computed from (u64)m",
    "status-chacha-m0-no-masks": "`% 0` in the unmask: the oracle would divide by zero",
    "status-full-m0": "`% 0` in the mask combine: the oracle would divide by zero",
    "status-full-i64min": "modulus i64::MIN is outside the engine's domain; C's `%` overflows at i64::MIN % -1",
    "status-chacha-i64min-no-masks": "modulus i64::MIN, as above",
    "status-add-m0": "`% 0` in the Additive combine: the oracle would divide by zero",
    "status-add-i64min": "modulus i64::MIN, as above",
    "status-add-mismatching-after-m0": "`% 0` in the Additive combine: the oracle would divide by zero",
    "status-full-ragged-masks": "the oracle's combine_rows checks every length first; the model follows full.rs:43-46",
}
PARTICIPANT_OUTSIDE_ORACLE = {
    "status-dev-share-count-0": "share_count - 1 underflows: the oracle takes n >= 1",
    "status-keyed-share-count-0": "share_count - 1 underflows: the oracle takes n >= 1",
    "status-dev-additive-m0": "gen_range(0, 0) / `% 0`: the oracle would divide by zero",
    "status-keyed-additive-negative": "gen_range(0, m < 0) panics in the reference; the oracle takes its draws as given",
}
for _e in PD.ENTRIES:
    PARTICIPANT_OUTSIDE_ORACLE[f"status-{_e}-full-m0"] = "`% 0` in the mask: the oracle would divide by zero"
    PARTICIPANT_OUTSIDE_ORACLE[f"status-{_e}-chacha-negative"] = "gen_range(0, m < 0): outside the oracle's draws"
    PARTICIPANT_OUTSIDE_ORACLE[f"status-{_e}-seed-words"] = "the seed length is the caller's: the oracle takes any"

# early returns that belong to the engine's C ABI, not to the reference: neither reference has an opinion
ENGINE_ONLY = {"1..8 words", "clerk shares per batch", "output buffer too small", "bad mode", "NULL argument",
               "Full masking needs the drawn masks", "need the randomness draws", "payload_cap",
               "int32 shares need a PackedShamir scheme", "modulus <= 2^31"}


def _oracle_recipient(case, masks, indexed, mode):
    """The step-wise flow of tests/test_gpu_pipelines.py over the oracle; CANONICAL: the residues of its reveal."""
    be = OracleBackend()
    ms, ss = case.ms, case.ss
    mask = be.mask_combine(ms, masks)
    masked = np.asarray(be.secret_reconstruct(ss, case.dimension, indexed), np.int64)
    if mode == PD.CANONICAL and PD.is_packed(ss):
        masked = np.mod(masked, ss.prime_modulus)
    return [int(v) for v in be.positive(case.m_out, be.secret_unmask(ms, (mask, masked)))]


RECIPIENT_ALL = PC.RECIPIENT_CASES + PC.RECIPIENT_ZERO + PC.RECIPIENT_STATUS


@pytest.mark.parametrize("case", RECIPIENT_ALL, ids=_ids(RECIPIENT_ALL))
def test_recipient_model_equals_the_stepwise_oracle(case):
    for form in case.forms:
        masks, indexed = PC.host_rows(case) if form == "host" else PC.recipient_inputs(case)
        want_status = PC.recipient_expected_status(case, form)
        if case.group == "status":
            assert want_status is not None, "a status row must fail"
            if case.null or want_status[1] in ENGINE_ONLY:
                continue                           # the C ABI's own checks: neither reference has an opinion
        try:
            model = PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, case.mode)
            model_status = None
        except PM.ModelError as e:
            model, model_status = None, (e.status, e.cls)
        if case.group == "status":
            assert model_status == want_status
        else:
            assert want_status is None and model_status is None
            assert len(model) == case.D
        if case.id in RECIPIENT_OUTSIDE_ORACLE:
            continue
        try:
            oracle = _oracle_recipient(case, masks, indexed, case.mode)
            oracle_status = None
        except E.SdaError as e:
            oracle, oracle_status = None, e.status
        assert oracle_status == (model_status[0] if model_status else None)
        assert oracle == model


def test_the_oracle_domain_lists_name_real_cases():
    assert set(RECIPIENT_OUTSIDE_ORACLE) <= set(_ids(PC.RECIPIENT_STATUS))
    assert set(PARTICIPANT_OUTSIDE_ORACLE) <= set(_ids(PC.PARTICIPANT_STATUS))
    # every successful case is inside the oracle's domain
    assert not [c for c in RECIPIENT_OUTSIDE_ORACLE if not c.startswith("status-")]


PARTICIPANT_ALL = PC.PARTICIPANT_CASES + PC.PARTICIPANT_ZERO + PC.PARTICIPANT_STATUS


def _oracle_participant(case, secrets, seed, full, draws):
    be = OracleBackend()
    sec = np.asarray(secrets, np.int64)
    if isinstance(case.ms, S.FullMasking):
        _, masked = be.secret_mask(case.ms, sec, full_masks=np.asarray(full, np.int64))
    elif isinstance(case.ms, S.ChaChaMasking):
        _, masked = be.secret_mask(case.ms, sec, seed=np.asarray(seed[:8] if len(seed) else [0], np.uint32))
    else:
        masked = sec
    if len(sec) == 0:
        return [], [[] for _ in range(case.ss.output_size())]
    sh = np.asarray(be.share_generate(case.ss, masked, np.asarray(draws, np.int64)), np.int64)
    if case.mode == PD.CANONICAL and PD.is_packed(case.ss):
        sh = np.mod(sh, case.ss.prime_modulus)
    return [int(v) for v in masked], [[int(v) for v in row] for row in sh]


@pytest.mark.parametrize("case", PARTICIPANT_ALL, ids=_ids(PARTICIPANT_ALL))
def test_participant_model_equals_the_stepwise_oracle(case):
    secrets, seed, full, draws = PC.participant_inputs(case)
    want_status = PC.participant_expected_status(case)
    try:
        model = PM.participant(case.ms, case.ss, secrets, draws, seed=seed, full_masks=full,
                               mode=case.mode if case.mode in (0, 1) else 0)
        model_status = None
    except PM.ModelError as e:
        model, model_status = None, (e.status, e.cls)
    if case.group == "status":
        assert want_status is not None, "a status row must fail"
        if want_status[1] in ENGINE_ONLY:
            assert model_status is None
        elif case.null != "seed":
            assert model_status == want_status
    else:
        assert want_status is None and model_status is None
        assert len(model[1]) == case.ss.output_size() and all(len(r) == case.B for r in model[1])
    if model is None or case.id in PARTICIPANT_OUTSIDE_ORACLE or case.mode not in (0, 1):
        return
    masked, shares = _oracle_participant(case, secrets, seed, full, draws)
    assert (masked, shares) == (model[0], model[1])


def test_keyed_draws_follow_the_documented_rule():
    """A keyed case's draws are elements 0.. of (KEY, STREAM): column d's n - 1 draws at bound m, batch b's t draws
    at bound p - 1 -- tests/draws_model.py, laid out as the caller-supplied draws are."""
    from tests import draws_model as DM
    for case in PC.PARTICIPANT_CASES:
        if case.keyed and case.D:
            _, _, _, draws = PC.participant_inputs(case)
            per, bound = ((case.ss.privacy_threshold(), case.ss.prime_modulus - 1) if PD.is_packed(case.ss)
                          else (case.ss.share_count - 1, case.ss.modulus))
            assert len(draws) == case.B * per
            if per:
                last = case.B * per - 1
                assert draws[last] == DM.draw(PC.KEY, PC.STREAM, last, bound)[0]


# ---------------------------------------------------------------- every decision value is taken
def _recipient_decisions(case, env_exact=None):
    _, indexed = PC.recipient_inputs(case)
    idx = [i for i, _ in indexed]
    ms, ss = case.ms, case.ss
    d = {"mask_kind": PD.mask_kind(ms), "pending": PD.chacha_pending(ms, case.n_masks),
         "multi_mask": PD.multi_mask(ms, case.n_masks)}
    if case.packed:
        d.update(residue_only=PD.residue_only(ms, ss, case.m_out, env_exact),
                 run_mode=(case.mode, PD.run_mode(ms, ss, case.m_out, case.mode, env_exact)),
                 fell_back=PD.fell_back(ms, ss, case.m_out, case.mode, idx, env_exact),
                 compact=PD.compact(ss, case.dimension, case.share_len))
    return d


def test_every_recipient_decision_value_is_taken():
    seen = {}
    why_false = set()
    true_kinds = set()
    for case in PC.RECIPIENT_CASES:
        for k, v in _recipient_decisions(case).items():
            seen.setdefault(k, set()).add(v)
        if not case.packed or case.mode != PD.EXACT:
            continue
        p = case.ss.prime_modulus
        if PD.residue_only(case.ms, case.ss, case.m_out):
            true_kinds.add(PD.mask_kind(case.ms))
            assert "residue_only" in case.tags, case.id
            assert not PD.residue_only(case.ms, case.ss, case.m_out, "1")
            why_false.add("env")
        else:
            assert "residue_only" not in case.tags, case.id
            if case.m_out != p:
                why_false.add("output_modulus")
            if not isinstance(case.ms, S.NoMasking) and abs(case.ms.modulus) != p and case.m_out == p:
                why_false.add("mask_modulus")
    assert true_kinds == {PD.MASK_NONE, PD.MASK_FULL, PD.MASK_CHACHA}
    assert why_false == {"env", "output_modulus", "mask_modulus"}
    assert seen["mask_kind"] == {PD.MASK_NONE, PD.MASK_FULL, PD.MASK_CHACHA}
    assert seen["residue_only"] == {True, False}
    assert seen["run_mode"] == {(0, 0), (0, 1), (1, 1)}
    assert seen["fell_back"] == {True, False}
    assert seen["compact"] == {True, False}
    assert seen["pending"] == {True, False}
    assert seen["multi_mask"] == {True, False}
    records = {PD.recipient_record(c.ms, c.ss, c.dimension, c.subset, c.share_len, c.m_out, c.mode,
                                   late_resolve="late" in c.tags) for c in PC.RECIPIENT_CASES}
    for field, values in enumerate(({1, 2, 3}, {0, 1, 2}, {0, 1}, {0, 1}, {1, 2})):
        assert {r[field] for r in records} == values, field
    # the tables' spread: every modulus class on both sides, every shape, every subset kind
    add = [c for c in PC.RECIPIENT_CASES if not c.packed]
    assert {abs(c.ss.modulus) for c in add} >= set(PC.MODULI)
    assert {c.ss.modulus for c in add} >= set(PC.NEGATIVE_MODULI)
    assert {c.ms.modulus for c in add if isinstance(c.ms, S.FullMasking)} >= set(PC.MODULI + PC.NEGATIVE_MODULI)
    assert {c.length for c in add} >= set(PC.ELEMENTWISE_D)
    assert {c.ss.share_count for c in add} >= {1, 2, 3}
    for ss in (PC.FL, PC.CP):
        mine = [c for c in PC.RECIPIENT_CASES if c.ss == ss]
        assert {c.length for c in mine} >= set(PC.packed_dims(ss))
        assert {c.m_out for c in mine} >= {ss.modulus, ss.modulus + 2, 2**40, 0, -ss.modulus, I64_MAX}
        assert {c.share_extra for c in mine} == {0, 3} and any(c.host_share_extra for c in mine)
    assert {c.n_masks for c in PC.RECIPIENT_CASES} >= {0, 1, 5}
    assert {c.seed_words for c in PC.RECIPIENT_CASES if isinstance(c.ms, S.ChaChaMasking)} >= {1, 4, 8}
    assert any(c.host_mask_lens and max(c.host_mask_lens) > 8 for c in PC.RECIPIENT_CASES)
    assert {c.out_slack for c in PC.RECIPIENT_CASES} == {0, 8} and any(c.out_slack == -1 for c in PC.RECIPIENT_STATUS)
    cm = {c.ms.modulus for c in PC.RECIPIENT_CASES if isinstance(c.ms, S.ChaChaMasking) and c.n_masks}
    assert cm >= {PC.CHACHA_FAST, PC.CHACHA_HIGH_REJECTION, PC.CHACHA_ABOVE_2_62}
    assert sum(c.ss == PC.wide_scheme() for c in PC.RECIPIENT_CASES) == 1


def test_chacha_moduli_are_named_from_the_chacha_matrix():
    from tests import test_gpu_chacha_matrix as CM
    assert PC.CHACHA_FAST in CM.FAST and PC.CHACHA_FAST in CM.REJECTS
    assert PD.chacha_fast_path(PC.CHACHA_FAST) and all(PD.chacha_fast_path(m) for m in CM.FAST)
    assert not PD.chacha_fast_path(PC.CHACHA_HIGH_REJECTION) and PC.CHACHA_HIGH_REJECTION <= 2**62
    assert PD.U64_MAX % PC.CHACHA_HIGH_REJECTION + 1 > 2**36          # its rejection rate alone takes it off
    assert not PD.chacha_fast_path(PC.CHACHA_ABOVE_2_62) and PC.CHACHA_ABOVE_2_62 > 2**62
    assert not PD.chacha_fast_path(433, "stream")
    assert PC.LATE_D > PC.LATE_PAIR


def test_every_participant_decision_value_is_taken():
    records = {}
    for c in PC.PARTICIPANT_CASES:
        records.setdefault(c.entry, set()).add(PD.participant_record(c.ms, c.ss, c.entry, late_resolve="late" in c.tags))
    for entry in ("dev", "keyed"):
        assert {r[0] for r in records[entry]} == {1, 2, 3, 4}, entry
    for entry in ("dev32", "keyed32"):
        assert {r[0] for r in records[entry]} >= {1, 2, 3}, entry      # route 4's moduli pass no int32 row
    assert {r[1] for rs in records.values() for r in rs} == {1, 2, 3, 4}
    assert {r[1] for r in records["dev"]} == {1, 3} and {r[1] for r in records["keyed32"]} == {2, 4}
    assert {r[2] for rs in records.values() for r in rs} == {1, 2}
    C = PC.PARTICIPANT_CASES
    assert {c.secrets for c in C} == {"inside", "i64"} and {c.payload for c in C} == {True, False}
    assert {c.mode for c in C if PD.is_packed(c.ss)} == {0, 1}
    assert {c.ms.seed_words() for c in C if isinstance(c.ms, S.ChaChaMasking)} >= {0, 1, 8, 9}
    assert {c.ss.share_count for c in C if not PD.is_packed(c.ss)} >= {1, 2, 3}
    assert {c.D for c in C if not PD.is_packed(c.ss)} >= set(PC.ELEMENTWISE_D)
    for ss in (PC.FL, PC.CP):
        assert {c.D for c in C if c.ss == ss} >= set(PC.packed_dims(ss))
    assert {c.entry for c in C if c.ss == PC.wide_scheme()} == set(PD.ENTRIES)
    assert {c.ms.modulus for c in C if isinstance(c.ms, S.ChaChaMasking)} >= {PC.CHACHA_FAST, PC.CHACHA_HIGH_REJECTION,
                                                                              PC.CHACHA_ABOVE_2_62, 1, 2}


RECIPIENT_STATUS_CLASSES = {
    (PD.PRECONDITION, "masks.iter().all"), (PD.UNSUPPORTED, "1..8 words"), (PD.PRECONDITION, "gen_range"),
    (PD.PRECONDITION, "divisor of zero"), (PD.UNSUPPORTED, "i64::MIN"),
    (PD.MISMATCHING_DIMENSION, "Mismatching dimension"), (PD.PRECONDITION, "mask.len() == dimension"),
    (PD.PRECONDITION, "index out of bounds"), (PD.NOT_ENOUGH_SHARES, "Not enough shares"),
    (PD.UNSUPPORTED, "clerk shares per batch"), (PD.INVALID_ARGUMENT, "bad mode"),
    (PD.PRECONDITION, "mask.len() == masked_secrets.len()"), (PD.INVALID_ARGUMENT, "output buffer too small"),
    (PD.INVALID_ARGUMENT, "NULL argument"),
}
PARTICIPANT_STATUS_CLASSES = {
    (PD.INVALID_ARGUMENT, "NULL argument"), (PD.UNSUPPORTED, "int32 shares need a PackedShamir scheme"),
    (PD.INVALID_ARGUMENT, "bad mode"), (PD.PRECONDITION, "share_count - 1 underflows"), (PD.PRECONDITION, "gen_range"),
    (PD.UNSUPPORTED, "modulus <= 2^31"), (PD.INVALID_ARGUMENT, "Full masking needs the drawn masks"),
    (PD.PRECONDITION, "dimension == secrets.len()"), (PD.PRECONDITION, "seed words"),
    (PD.INVALID_ARGUMENT, "need the randomness draws"), (PD.INVALID_ARGUMENT, "payload_cap"),
}


def test_status_matrices_hold_every_early_return():
    got = {PC.recipient_expected_status(c, f) for c in PC.RECIPIENT_STATUS for f in c.forms}
    assert got == RECIPIENT_STATUS_CLASSES
    # the rows the issue names, by what makes them fail
    by_id = {c.id: c for c in PC.RECIPIENT_STATUS}
    assert PC.recipient_expected_status(by_id["status-packed-short-enough"], "dev")[1] == "index out of bounds"
    assert PC.recipient_expected_status(by_id["status-packed-empty-rows-few"], "dev")[1] == "index out of bounds"
    assert PC.recipient_expected_status(by_id["status-add-mismatching-after-none-mask"], "host")[1] == "masks.iter().all"
    assert PC.recipient_expected_status(by_id["status-add-mismatching-after-m0"], "host")[1] == "divisor of zero"
    assert PC.recipient_expected_status(by_id["status-chacha-m0-no-masks"], "dev")[1] == "divisor of zero"
    got = {PC.participant_expected_status(c) for c in PC.PARTICIPANT_STATUS}
    assert got == PARTICIPANT_STATUS_CLASSES
    for entry in PD.ENTRIES:
        mine = {PC.participant_expected_status(c) for c in PC.PARTICIPANT_STATUS if c.entry == entry}
        assert mine >= {(PD.PRECONDITION, "gen_range"), (PD.PRECONDITION, "seed words"),
                        (PD.PRECONDITION, "dimension == secrets.len()"), (PD.INVALID_ARGUMENT, "payload_cap")}, entry
    # zero-length successes
    assert all(PC.recipient_expected_status(c, f) is None and c.D == 0 for c in PC.RECIPIENT_ZERO for f in c.forms)
    assert any(not c.packed and not c.subset for c in PC.RECIPIENT_ZERO)
    assert all(PC.participant_expected_status(c) is None for c in PC.PARTICIPANT_ZERO)
    # the status codes are the header's, as the binding has them
    for name in ("MISMATCHING_DIMENSION", "NOT_ENOUGH_SHARES", "PRECONDITION", "INVALID_ARGUMENT", "UNSUPPORTED"):
        assert getattr(PD, name) == getattr(E, "ERR_" + name)
    assert (PD.MASK_NONE, PD.MASK_FULL, PD.MASK_CHACHA, PD.MASK_COMBINED_ROW) == (
        E.RECIPIENT_MASK_NONE, E.RECIPIENT_MASK_FULL, E.RECIPIENT_MASK_CHACHA, E.RECIPIENT_MASK_COMBINED_ROW)
    assert (PD.REVEAL_ADDITIVE, PD.REVEAL_EXACT, PD.REVEAL_CANONICAL) == (
        E.RECIPIENT_REVEAL_ADDITIVE, E.RECIPIENT_REVEAL_EXACT, E.RECIPIENT_REVEAL_CANONICAL)
    assert (1, 2, 3, 4) == (E.PARTICIPANT_MASK_NONE, E.PARTICIPANT_MASK_FULL_ADD, E.PARTICIPANT_MASK_CHACHA_FUSED,
                            E.PARTICIPANT_MASK_CHACHA_COMBINE_ADD)
    assert (1, 2, 3, 4) == (E.PARTICIPANT_SHARE_ADDITIVE, E.PARTICIPANT_SHARE_ADDITIVE_KEYED,
                            E.PARTICIPANT_SHARE_PACKED, E.PARTICIPANT_SHARE_PACKED_KEYED)


# ---------------------------------------------------------------- the steering steers
def _flows(case):
    masks, indexed = PC.recipient_inputs(case) if "dev" in case.forms else PC.host_rows(case)
    exact = PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, PD.EXACT)
    # (a canonical reveal of repeated points does not exist)
    canon = PM.recipient(case.ms, masks, case.ss, case.dimension, indexed, case.m_out,
                         PD.CANONICAL) if not PD.has_duplicates([i for i, _ in indexed]) else None
    return exact, canon


def test_representative_cases_depend_on_the_representative():
    cases = [c for c in PC.RECIPIENT_CASES if "representative" in c.tags]
    assert len(cases) >= 10
    for case in cases:
        exact, canon = _flows(case)
        assert canon is not None and exact != canon, case.id
        assert not PD.residue_only(case.ms, case.ss, case.m_out), case.id


def test_residue_only_cases_do_not():
    cases = [c for c in PC.RECIPIENT_CASES if "residue_only" in c.tags]
    assert len(cases) >= 10
    for case in cases:
        assert case.mode == PD.EXACT and PD.residue_only(case.ms, case.ss, case.m_out), case.id
        exact, canon = _flows(case)
        masks, indexed = PC.recipient_inputs(case) if "dev" in case.forms else PC.host_rows(case)
        masked = PM.recipient_steps(case.ms, masks, case.ss, case.dimension, indexed, case.m_out, PD.EXACT)[1]
        if case.length >= 8:                       # (a few elements may all be non-negative)
            assert any(v < 0 for v in masked), f"{case.id}: the exact reveal has no negative representative to hide"
        if canon is None:                          # repeated points: the fall-back case, there is no canonical flow
            assert PD.fell_back(case.ms, case.ss, case.m_out, case.mode, case.subset), case.id
        else:
            assert exact == canon, case.id


def test_wrap_cases_leave_i64():
    r = [c for c in PC.RECIPIENT_CASES if "wrap" in c.tags]
    assert len(r) >= 3
    for case in r:
        masks, indexed = PC.recipient_inputs(case)
        mask, masked, _ = PM.recipient_steps(case.ms, masks, case.ss, case.dimension, indexed, case.m_out)
        assert any(not I64_MIN <= v - k <= I64_MAX for v, k in zip(masked, mask)), case.id
    p = [c for c in PC.PARTICIPANT_CASES if "wrap" in c.tags]
    assert len(p) >= 3 and {c.entry for c in p} >= {"dev", "keyed"}
    for case in p:
        secrets, _, full, _ = PC.participant_inputs(case)
        assert any(not I64_MIN <= s + k <= I64_MAX for s, k in zip(secrets, full)), case.id


def test_raw_rows_carry_the_specials():
    for case in PC.RECIPIENT_CASES:
        if case.raw and not case.packed and case.length >= 14 and "wrap" not in case.tags:
            _, indexed = PC.recipient_inputs(case)
            for c, row in indexed:
                assert set(PC.specials(case.ss.modulus)) <= set(row), case.id
    seen = set()
    for case in PC.RECIPIENT_CASES:
        if case.raw and not case.packed and case.length == 1:
            seen |= {row[0] for _, row in PC.recipient_inputs(case)[1]}
    assert len(seen) >= 3                                   # dimension 1: the rotation spreads them over the cases


def test_late_cases_use_a_golden_rejecting_seed(oracle):
    for case in [c for c in PC.RECIPIENT_CASES + PC.PARTICIPANT_CASES if "late" in c.tags]:
        assert PD.chacha_fast_path(case.ms.modulus)
        hit = oracle.chacha_first_reject(case.ms.modulus, np.asarray(PC.LATE_SEED, np.uint32), case.ms.dimension)
        assert hit == PC.LATE_PAIR < case.ms.dimension, case.id


def test_zero_row_chacha_combine_is_zeros_in_both_references(oracle):
    """chacha.rs:57-76 with no seed row: `dimension` zeros for any modulus, and no division by it."""
    from tests.cpu_engine import CpuEngine
    cases = [c for c in PC.RECIPIENT_CASES if "zero_rows" in c.tags]
    assert {c.ms.modulus > 0 for c in cases} == {True, False}
    for m in (433, -PC.P, -(2**62 + 1), 0, I64_MIN):
        ms = S.ChaChaMasking(m, 5, 128)
        assert PM.mask_combine(ms, []) == [0] * 5
        assert OracleBackend().mask_combine(ms, []).tolist() == [0] * 5
        out = np.full(5, -7, np.int64)
        CpuEngine().chacha_mask_combine_dev(m, 5, 0, 4, 0, out.ctypes.data)
        assert out.tolist() == [0] * 5
    with pytest.raises(PM.ModelError):
        PM.mask_combine(S.ChaChaMasking(-433, 5, 128), [[1, 2, 3, 4]])
    with pytest.raises(E.SdaError) as ei:
        OracleBackend().mask_combine(S.ChaChaMasking(-433, 5, 128), [[1, 2, 3, 4]])
    assert ei.value.status == E.ERR_PRECONDITION
    with pytest.raises(E.SdaError):
        OracleBackend().mask_combine(S.ChaChaMasking(0, 5, 128), [[1, 2, 3, 4]])


# ---------------------------------------------------------------- conditions on the GPU file
def test_no_case_is_left_out_skipped_or_expected_to_fail():
    from tests import test_gpu_pipeline_matrix as G
    ran = [c.id for cases in G.GROUPS.values() for c in cases]
    assert sorted(ran) == sorted(c.id for c in PC.ALL_CASES)
    text = open(GPU_FILE).read()
    assert not re.search(r"\b(skip|skipif|xfail)\b", text.replace("importorskip", ""))
    for name in G.GROUPS:
        assert re.search(rf"^def {name}\(", text, re.M), name
    assert len(set(c.id for c in PC.ALL_CASES)) == len(PC.ALL_CASES)


def test_the_buffer_check_sees_every_word():
    """Guarded.check compares every output element, every word of the slack and every guard word: one changed word
    anywhere in the buffer fails it."""
    from tests import test_gpu_pipeline_matrix as G
    want = np.arange(5, dtype=np.int64)
    for dtype, poison in ((np.int64, PC.POISON), (np.int32, PC.POISON32), (np.uint8, PC.POISON8)):
        host = G.guarded_host(5, 8, dtype)
        assert host.size == 2 * PC.GUARD + 5 + 8 and (host == poison).all()
        host[PC.GUARD:PC.GUARD + 5] = want
        G.check_guarded(host, want.astype(dtype), 8, "ok")
        for pos in range(host.size):
            bad = host.copy()
            bad[pos] ^= 1
            with pytest.raises(AssertionError):
                G.check_guarded(bad, want.astype(dtype), 8, f"word {pos}")
