"""CPU: the whole-aggregation driver (tests/job_aggregation.py) over its oracle backend, before any GPU is involved.

  - over every case id of tests/test_gpu_job_aggregation.py the oracle backend's output is (sum_p s_p) mod m in Python
    integers: the expected values, the driver and the chosen inputs (the no-wrap precondition) are right;
  - the case list is the covering matrix it claims to be;
  - the comparison has teeth: the driver over deliberately faulty oracle backends (no engine code) must fail it.

FINDINGS of the faulty backends, each moved to the check that does see it:
  - a recipient handed clerk c's result under index c + 1 is invisible to the final sum under an Additive scheme: its
    reconstruction is the index-free sum of the results (additive.rs:56-70).  It is visible under PackedShamir.
  - a snapshot that swaps two clerks' columns is invisible to the final sum under an Additive scheme for the same
    reason (every clerk folds a full column, and the sum of the clerk results does not care which); it is caught by
    check (c) of the GPU file, restated here: clerk c's payload must decode to the combine of the participants'
    payloads for clerk c.
  - under the decoded reveal a single stale clerk within the radius is corrected, by design: the output stays the
    sum and the fault shows in `blame` (FAULT_CASES).
"""
import numpy as np
import pytest

from oracle import oracle as O
from sda_amd import schemes as S
from tests import job_aggregation as JA

CASES = JA.CASES
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def traces():
    return {}


def _trace(traces, case):
    if case.id not in traces:
        traces[case.id] = JA.run_case(JA.OracleBackend(O), case)
    return traces[case.id]


# ---------------------------------------------------------------------------------------------------- the matrix
def test_case_ids_are_unique_and_every_axis_value_occurs():
    assert len(set(IDS)) == len(IDS)
    for axis in JA.AXES:
        assert {getattr(c, axis) for c in CASES} == set(JA.VALUES[axis]), axis
    assert all(JA.valid(c) for c in CASES + JA.FAULT_CASES)


def test_every_feasible_pair_of_neighbouring_axes_is_covered():
    import itertools
    everything = [JA.Case(*v) for v in itertools.product(*[JA.VALUES[a] for a in JA.AXES])]
    feasible = [c for c in everything if JA.valid(c)]
    skipped = set()
    for a, b in JA.PAIRS:
        have = {(getattr(c, a), getattr(c, b)) for c in CASES}
        can = {(getattr(c, a), getattr(c, b)) for c in feasible}
        assert have == can, (a, b, sorted(can - have))
        skipped |= {(a, va, b, vb) for va in JA.VALUES[a] for vb in JA.VALUES[b]} - {(a, x, b, y) for x, y in can}
    # what no case can hold (JA.valid): the size limit; k - 1 = 0; the decoded job outside its schemes, and
    # FULL_LOOP_PACKED (8 clerks, k + t = 7) from a subset
    decoded = ("dec-all", "dec-r1", "dec-r2")
    want = {("P", 33, "dkind", "big")}
    want |= {("scheme", s, "dkind", "k-1") for s in ("add32", "add36", "add61")}
    want |= {("scheme", s, "recipient", r) for s in ("add32", "add36", "add61", "b16", "wide") for r in decoded}
    want |= {("scheme", "fl", "recipient", r) for r in decoded[1:]}
    assert skipped == want


def test_the_dimensions_are_the_ones_named():
    for c in CASES:
        k = c.k
        assert c.D in (1, k - 1, k + 1, 2049, 2048 * k + 5) and c.D >= 1
        assert c.ss.modulus <= JA.M_MAX


def test_column_zero_holds_the_edge_secrets():
    seen = set()
    for c in CASES:
        secrets, keys, seeds = JA.inputs(c)
        m = c.ss.modulus
        assert (np.abs(secrets) < m).all()
        seen |= {("0", "1", "-1", "m-1", "-(m-1)")[[0, 1, -1, m - 1, -(m - 1)].index(int(v))] for v in secrets[:, 0]}
        assert len({k for k, _, _ in keys}) == c.P
    assert seen == {"0", "1", "-1", "m-1", "-(m-1)"}


# ---------------------------------------------------------------------------------------------------- the sum
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_chain_gives_the_plain_sum(traces, case):
    tr = _trace(traces, case)
    secrets, _, _ = JA.inputs(case)
    assert np.array_equal(tr.output, JA.expected(secrets, case.ss.modulus))
    if tr.decode is not None:
        assert (tr.decode.bad_batches, tr.decode.undecoded, sum(tr.decode.blame)) == (0, 0, 0)
        assert not tr.verdict.any() and not tr.wrong.any()


@pytest.mark.parametrize("case", JA.FAULT_CASES, ids=[c.id for c in JA.FAULT_CASES])
def test_oracle_chain_with_misbehaving_clerks(case):
    check_faulty_clerks(case, JA.run_case(JA.OracleBackend(O), case))


def check_faulty_clerks(case, tr):
    """(f) on a trace: within the radius the sum stands and exactly the misbehaving clerks are blamed; one clerk
    past it, no batch that differs from the sum is reported clean.  The plain job over the same payloads differs."""
    ss = case.ss
    secrets, _, _ = JA.inputs(case)
    want = JA.expected(secrets, ss.modulus)
    n, k = ss.output_size(), ss.secret_count
    r = n - JA.kt_of(ss)
    bad = sorted(c for c, _ in case.faulty)
    assert tr.decode.redundancy == r and tr.decode.radius == r // 2
    assert not np.array_equal(tr.job_output, want), "the fault is real: the plain job reveals something else"
    if case.faults <= r // 2:
        assert np.array_equal(tr.output, want)
        assert tr.decode.undecoded == 0
        assert [c for c in range(n) if tr.decode.blame[c]] == bad
    else:
        differs = [b for b in range(len(tr.verdict)) if not np.array_equal(tr.output[b * k:(b + 1) * k],
                                                                          want[b * k:(b + 1) * k])]
        assert all(tr.verdict[b] == 0xFFFF for b in differs)
        assert tr.decode.undecoded == int(np.count_nonzero(tr.verdict == 0xFFFF)) >= len(differs)
        assert tr.decode.undecoded, "a clerk past the radius goes unnoticed"


# ---------------------------------------------------------------------------------------------------- teeth
class SwappedColumns(JA.OracleBackend):
    """the snapshot hands clerk 0 clerk 1's column and the reverse"""
    def snapshot(self):
        super().snapshot()
        t = self.tr.transposed
        t[0], t[1] = t[1], t[0]


class DropsLast(JA.OracleBackend):
    """clerk 1 drops its last participation"""
    def clerk(self, c, blobs):
        return super().clerk(c, blobs[:-1] if c == 1 else blobs)


class FoldsTwice(JA.OracleBackend):
    """clerk 1 folds participation 0 twice"""
    def clerk(self, c, blobs):
        return super().clerk(c, list(blobs) + [blobs[0]] if c == 1 else blobs)


class ShiftedIndex(JA.OracleBackend):
    """the recipient is handed clerk c's result under index c + 1 (the last one wraps to 0)"""
    def indexed(self, sel):
        got = super().indexed(sel)
        n = self.n
        return [((c + 1) % n, b) for c, b in got]


class MissesAMask(JA.OracleBackend):
    """the mask fold misses participant 0"""
    def fold_masks(self, payloads):
        return super().fold_masks(payloads[1:])


def _pick(scheme_kind, masking=None, min_p=2, job=False):
    for c in CASES:
        if JA.is_packed(c.ss) != (scheme_kind == "packed") or c.P < min_p or c.scheme == "wide":
            continue
        if masking is not None and c.masking != masking:
            continue
        if job and c.recipient.startswith("dec"):
            continue
        return c
    raise AssertionError("the matrix has no such case")


def _final_comparison_fails(backend, case):
    secrets, _, _ = JA.inputs(case)
    tr = JA.run_case(backend, case)
    return tr, not np.array_equal(tr.output, JA.expected(secrets, case.ss.modulus))


def _column_check_fails(tr, case):
    """check (c): clerk c's payload is the combine of the participants' payloads for clerk c"""
    m = case.ss.modulus
    for c in range(case.ss.output_size()):
        rows = np.stack([O.varint_decode(tr.participant_payloads[p][c]) for p in range(case.P)])
        if not np.array_equal(O.varint_decode(tr.clerk_payloads[c]), O.combine(m, rows)):
            return True
    return False


@pytest.mark.parametrize("kind", ["packed", "additive"])
@pytest.mark.parametrize("fault", [DropsLast, FoldsTwice])
def test_a_clerk_that_folds_the_wrong_rows_fails_the_sum(fault, kind):
    case = _pick(kind, job=True)
    tr, fails = _final_comparison_fails(fault(O), case)
    assert fails and _column_check_fails(tr, case)


@pytest.mark.parametrize("kind", ["packed", "additive"])
def test_a_mask_fold_that_misses_a_participant_fails_the_sum(kind):
    case = _pick(kind, masking="full", job=True)
    assert _final_comparison_fails(MissesAMask(O), case)[1]


def test_swapped_columns():
    case = _pick("packed", job=True)
    tr, fails = _final_comparison_fails(SwappedColumns(O), case)
    assert fails and _column_check_fails(tr, case)
    # FINDING: invisible to the sum under an Additive scheme; check (c) sees it
    case = _pick("additive", job=True)
    tr, fails = _final_comparison_fails(SwappedColumns(O), case)
    assert not fails and _column_check_fails(tr, case)


def test_a_result_under_the_next_index():
    case = _pick("packed", job=True)
    assert _final_comparison_fails(ShiftedIndex(O), case)[1]
    # FINDING: an Additive reconstruction has no indices; nothing in the chain can see this
    case = _pick("additive", job=True)
    assert not _final_comparison_fails(ShiftedIndex(O), case)[1]


def test_the_honest_backend_passes_the_checks_the_faulty_ones_fail(traces):
    for kind in ("packed", "additive"):
        case = _pick(kind, job=True)
        tr = _trace(traces, case)
        secrets, _, _ = JA.inputs(case)
        assert np.array_equal(tr.output, JA.expected(secrets, case.ss.modulus)) and not _column_check_fails(tr, case)


def test_the_driver_refuses_what_the_identity_does_not_cover():
    be = JA.OracleBackend(O)
    key = tuple(range(8))
    with pytest.raises(AssertionError, match="2\\^62"):
        JA.run_job_aggregation(be, S.NoMasking(), S.Additive(2, (1 << 62) + 1), [[1]], [(key, 1, 2)], [None], JA.Plan())
    with pytest.raises(AssertionError, match="secrets"):
        JA.run_job_aggregation(be, S.NoMasking(), S.Additive(2, 433), [[433]], [(key, 1, 2)], [None], JA.Plan())
    with pytest.raises(AssertionError, match="never serve two"):
        JA.run_job_aggregation(be, S.NoMasking(), S.Additive(2, 433), [[1], [2]], [(key, 1, 2), (key, 2, 3)],
                               [None, None], JA.Plan())
    tr = JA.run_job_aggregation(be, S.NoMasking(), S.Additive(2, 1 << 62), [[(1 << 62) - 1], [(1 << 62) - 1]],
                                [(key, 1, 2), (key, 3, 4)], [None, None], JA.Plan())
    assert tr.output.tolist() == [(1 << 62) - 2]
