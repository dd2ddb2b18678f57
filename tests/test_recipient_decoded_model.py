"""CPU: tests/recipient_decoded_model.py (the robust recipient job's definition) held against the oracle.

On small schemes the model equals the oracle's own composition -- reconstruct from the shares without the wrong
clerks, unmask, positive() -- with whole wrong rows inside the radius, and equals tests/recipient_job_cases'
expected output (the recipient job's model) on clean payloads wherever the robust call is defined.  Mask values at
the edges of (-p, p) and of i64 give the big-integer residue; inside (-p, p) that is the reference's wrapping
unmask + positive(), outside it need not be, which is why the contract is stated as the residue."""
import numpy as np
import pytest

from sda_amd import schemes as S
from tests import checked_reveal_model as R
from tests import pipeline_dispatch as PD
from tests import pipeline_model as PM
from tests import recipient_decoded_model as RD
from tests import recipient_job_cases as RC
from tests.test_checked_reveal_model import SCHEMES, clean_rows, kt_of

I64_MIN, I64_MAX = -2**63, 2**63 - 1
SMALL = (("b8", 8), ("b8", 6), ("b16", 13), ("config", 19))


def _masks(ms, rng, D, p):
    if isinstance(ms, S.FullMasking):
        return [[int(v) for v in rng.integers(0, p, D)] for _ in range(3)]
    if isinstance(ms, S.ChaChaMasking):
        return [[int(v) for v in rng.integers(0, 2**32, 4)] for _ in range(2)]
    return []


@pytest.mark.parametrize("kind", ("none", "full", "chacha"))
@pytest.mark.parametrize("name,n_idx", SMALL)
def test_model_equals_the_oracles_composition_without_the_wrong_clerks(oracle, name, n_idx, kind):
    sch = SCHEMES[name]
    p, kt = sch.prime_modulus, kt_of(sch)
    rng = np.random.default_rng(n_idx)
    rows, D, secrets = clean_rows(oracle, sch, rng)
    other, _, _ = clean_rows(oracle, sch, rng)
    ms = {"none": S.NoMasking(), "full": S.FullMasking(p), "chacha": S.ChaChaMasking(p, D, 128)}[kind]
    masks = _masks(ms, rng, D, p)
    idx = rng.permutation(sch.share_count)[:n_idx].tolist()
    e_max = (n_idx - kt) // 2
    wrong_pos = sorted({0, n_idx - 1, kt - 1})[:e_max]
    sh = rows[idx].copy()
    for j in wrong_pos:
        sh[j] = other[idx[j]]
        same = (sh[j] - rows[idx[j]]) % p == 0
        sh[j][same] += 1
    exp = RD.run(oracle, ms, masks, sch, D, list(zip(idx, sh)))
    assert exp.undecoded == 0 and exp.bad_batches == (sh.shape[1] if wrong_pos else 0)
    assert exp.blame == [sh.shape[1] if j in wrong_pos else 0 for j in range(n_idx)]
    # the oracle's composition on the clerks that were right
    keep = [j for j in range(n_idx) if j not in wrong_pos]
    rc, masked = oracle.packed_reconstruct(R._params(oracle, sch), D, [idx[j] for j in keep], sh[keep])
    assert rc == 0
    mask = PM.mask_combine(ms, masks)
    out = masked if kind == "none" else oracle.unmask(p, np.asarray(mask, np.int64), masked)
    out = oracle.positive(p, out)
    assert np.array_equal(exp.out, out)
    assert np.array_equal(exp.secrets, secrets % p)
    assert np.array_equal(exp.out, (secrets - np.asarray(mask if mask else [0] * D, np.int64)) % p)


def _defined(case):
    ss, ms = case.ss, case.ms
    if not case.packed or RC.expected_status(case) is not None or case.dimension == 0:
        return False
    _, indexed = RC.rows(case)
    idx = [i for i, _ in indexed]
    # the cases' clerk rows are random values, not sharings: they are consistent exactly where nothing is redundant
    return (case.m_out == ss.prime_modulus and ss.secret_count <= 8 and len(idx) == kt_of(ss) and len(set(idx)) == len(idx)
            and (isinstance(ms, S.NoMasking) or abs(ms.modulus) == ss.prime_modulus))


CLEAN = [c for c in RC.CASES if _defined(c)]


def test_the_job_cases_reach_every_masking_kind():
    kinds = {type(c.ms) for c in CLEAN}
    assert kinds == {S.NoMasking, S.FullMasking, S.ChaChaMasking}, kinds


@pytest.mark.parametrize("case", CLEAN, ids=[c.id for c in CLEAN])
def test_model_equals_the_recipient_jobs_model_on_clean_payloads(oracle, case):
    masks, indexed = RC.rows(case)
    exp = RD.run(oracle, case.ms, masks, case.ss, case.dimension, indexed)
    assert exp.bad_batches == 0 and exp.undecoded == 0 and not exp.verdict.any()
    assert [int(v) for v in exp.out] == [int(v) for v in RC.expected_output(case)]


def test_edge_mask_values_give_the_big_integer_residue(oracle):
    sch = SCHEMES["b16"]
    p = sch.prime_modulus
    rng = np.random.default_rng(5)
    rows, D, secrets = clean_rows(oracle, sch, rng)
    idx = list(range(12))
    edge = [0, 1, -1, p - 1, -(p - 1), p, -p, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
    mask = [edge[i % len(edge)] for i in range(D)]
    assert D >= len(edge)
    exp = RD.run(oracle, S.FullMasking(p), None, sch, D, list(zip(idx, rows[idx])), mask=mask)
    for s, m, o in zip(secrets, mask, exp.out):
        q, r = divmod(int(s) - m, p)
        assert int(o) == r and 0 <= r < p and q * p + r == int(s) - m
    # inside (-p, p) this is the reference's wrapping unmask followed by positive()
    inside = [i for i, m in enumerate(mask) if abs(m) < p]
    ref = oracle.positive(p, oracle.unmask(p, np.asarray(mask, np.int64), secrets))
    assert np.array_equal(exp.out[inside], ref[inside])
    # at the ends of i64 the wrapping `-` leaves the residue class
    assert any(int(exp.out[i]) != int(ref[i]) for i, m in enumerate(mask) if abs(m) > 2**62)


def test_record_expectations():
    p = 433
    assert RD.record(S.NoMasking(), 4, 4) == (0, 1, 0)
    assert RD.record(S.FullMasking(p), 5, 4) == (1, 1, 1)
    assert RD.record(S.FullMasking(p), 4, 4, fused=False, redo=True) == (2, 1, 0)
    assert RD.record(S.ChaChaMasking(p, 8, 128), 4, 4, redo=True) == (1, 2, 0)
