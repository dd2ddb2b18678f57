"""GPU: a whole aggregation in which every role makes its job call and hands the output to the next role's job call
(tests/job_aggregation.py): sda_participant_job[_dev] -> sda_snapshot_transpose_dev -> sda_clerk_job[_dev] ->
sda_recipient_job[_dev] or sda_recipient_job_decoded[_dev], against (sum_p s_p) mod m in Python integers.

The matrix (job_aggregation.CASES) is a covering one: every value of each axis -- scheme, masking, participants,
dimension, clerk tiling, recipient -- meets every value of its neighbouring axes, and the scheme also meets every
dimension and every recipient; tests/test_job_aggregation_model.py holds it to that and runs every case id over the
oracle backend on the CPU.  Each case, on the device backend (all three clerk tilings) and on the host backend:
  (a) the output, read out of its guarded buffer, equals the plain sum;
  (b) both backends produce the same participant payloads, mask payloads, clerk payloads and output, byte for byte;
  (c) each clerk's payload decodes to oracle.combine of the oracle-decoded participant payloads of its column, and the
      transposed bytes are oracle.snapshot_transpose's: a failure of (a) is localised to a role;
  (d) the three clerk tilings leave identical states, payloads and folded masks;
  (e) the decoded job on consistent results: the output of (a), every count zero, verdict and wrong all zero;
  (g) the launch records name the routes the per-role files compute for the case's schemes.
(f) FAULT_CASES: clerks that misbehave by running the real clerk job on wrong inputs, up to, at and one past the
decoded reveal's radius.

Measured on an MI355X: see profiles/job_aggregation/cases.txt.
"""
import numpy as np
import pytest

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import codec_dispatch as CD
from tests import job_aggregation as JA
from tests import recipient_decoded_model as RD
from tests import recipient_job_cases as RJ
from tests import snapshot_dispatch as SD
from tests.test_job_aggregation_model import check_faulty_clerks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = JA.CASES
TILE_ENV = "SDA_PARTICIPANT_TILE_BATCHES"


@pytest.fixture
def no_knobs(monkeypatch):
    from tests import codec_matrix_cases as CM
    for k in tuple(CM.KNOBS) + (TILE_ENV, "SDA_RECIPIENT_EXACT", "SDA_CHACHA_PATH", "SDA_RECIPIENT_FUSE_UNMASK",
                                "SDA_RECIPIENT_REDO", "SDA_HOST_STAGE_MB"):
        monkeypatch.delenv(k, raising=False)


def _localise(oracle, case, tr, what):
    """(c): the snapshot and every clerk against the oracle on the bytes the role before produced"""
    m, n, P = case.ss.modulus, case.ss.output_size(), case.P
    assert tr.transposed == oracle.snapshot_transpose(tr.participant_payloads), f"{what}: snapshot"
    faulty = dict(case.faulty)
    for c in range(n):
        rows = np.stack([oracle.varint_decode(b) for b in tr.transposed[c]])
        assert rows.shape == (P, JA.width(case.ss, case.D)), (what, c)
        if c in faulty:
            continue
        want = oracle.combine(m, rows)
        assert np.array_equal(tr.clerk_states[c], want), f"{what}: clerk {c} state"
        assert tr.clerk_payloads[c] == oracle.varint_encode(want), f"{what}: clerk {c} payload"
    if isinstance(case.ms, S.FullMasking) and tr.combined_mask is not None:
        masks = np.stack([oracle.varint_decode(b) for b in tr.mask_payloads])
        assert masks.shape == (P, case.D) and 0 <= masks.min() and masks.max() < m
        assert np.array_equal(tr.combined_mask, oracle.combine(m, masks)), f"{what}: mask fold"
    if isinstance(case.ms, S.ChaChaMasking):
        _, _, seeds = JA.inputs(case)
        assert [oracle.varint_decode(b).tolist() for b in tr.mask_payloads] == seeds, f"{what}: seeds"
    if isinstance(case.ms, S.NoMasking):
        assert tr.mask_payloads == [b""] * P


def _same_bytes(dev, host, what):
    """(b)"""
    assert dev.participant_payloads == host.participant_payloads, f"{what}: participant payloads"
    assert dev.mask_payloads == host.mask_payloads, f"{what}: mask payloads"
    assert dev.clerk_payloads == host.clerk_payloads, f"{what}: clerk payloads"
    assert all(np.array_equal(a, b) for a, b in zip(dev.clerk_states, host.clerk_states)), f"{what}: clerk states"
    assert np.array_equal(dev.output, host.output), f"{what}: output"


def _same_tilings(dev, what):
    """(d)"""
    assert set(dev.tilings) == set(JA.TILINGS)
    s0, p0, m0 = dev.tilings["one"]
    for tiling in JA.TILINGS[1:]:
        s, p, m = dev.tilings[tiling]
        assert all(np.array_equal(a, b) for a, b in zip(s0, s)), f"{what}: states under {tiling}"
        assert p0 == p, f"{what}: payloads under {tiling}"
        assert (m0 is None and m is None) or np.array_equal(m0, m), f"{what}: folded mask under {tiling}"


def _routes(case, dev, host):
    """(g): the records of the last call of every role, from the per-role files' helpers"""
    from tests.test_gpu_clerk_job import FINISH_CODEC_RECORD, finish_record, job_record
    from tests.test_gpu_decoded_reveal import _record as decode_record
    from tests.test_gpu_participant_job import _route as participant_route
    ms, ss, P, D, n, W = case.ms, case.ss, case.P, case.D, case.ss.output_size(), JA.width(case.ss, case.D)
    sel, order = JA.clerk_order(ss, case.plan())
    out = {}
    # participant
    want = E.ParticipantJobLaunch(*participant_route(ms, ss), 1)
    assert dev.records["participant_job"] == want and host.records["participant_job"] == want
    out["participant"] = tuple(want)
    # snapshot
    plan = SD.plan(dev.part_off, P, n)
    assert dev.records["snapshot"] == plan.record
    assert dev.clerk_base.tolist() == plan.clerk_base and dev.clerk_off.tolist() == plan.clerk_off
    out["snapshot"] = plan.record
    # clerk: every call of the first and the last clerk job, from the bytes where the snapshot put them
    out["clerk"] = set()
    for c in (order[0], order[-1]):
        lo = int(dev.clerk_base[c])
        job_bytes = dev.transposed_bytes[lo:lo + int(dev.clerk_off[c][-1])]
        calls = [x for x in dev.clerk_calls if x[1] == c]
        assert {x[0] for x in calls} == set(JA.TILINGS)
        for tiling, _, b0, b1, first, pay, job_rec, codec_rec in calls:
            if b0 == b1:
                assert (job_rec, codec_rec) == (finish_record(W), FINISH_CODEC_RECORD), (tiling, c)
                continue
            record = CD.predict(CD.Job(job_bytes, dev.clerk_off[c][b0:b1 + 1]), ss.modulus, {})[0]
            assert codec_rec == record, (tiling, c, b0, b1)
            assert job_rec == job_record(record, first, pay, W, W if first else len(dev.transposed[c][0])), (tiling, c)
            out["clerk"].add((CD.PATH_NAMES[record[0]],) + tuple(job_rec))
    assert host.records["clerk_job"] == (0, 2, -(-W // CD.ENC_CHUNK))
    out["clerk"] = sorted(out["clerk"])
    # recipient
    lens = [W] * len(sel)
    for tr, form in ((dev, "dev"), (host, "host")):
        job, rec = RJ.records(ms, P if ms.has_mask() else 0, ss, D, sel, lens, ss.modulus, case.plan().mode, form)
        assert tr.records["recipient_job"] == job, form
        if case.plan().recipient == "job":
            assert tr.records["recipient"] == rec, form
        else:
            assert tr.records["recipient_decoded"] == RD.record(ms, W, W), form
            assert tr.records["packed_decode"] == decode_record(ss, len(sel), tr.verdict, tr.wrong,
                                                               tr.decode.bad_batches), form
        out[f"recipient-{form}"] = (job, rec if case.plan().recipient == "job" else tr.records["recipient_decoded"])
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_chain_gives_the_plain_sum(engine, oracle, no_knobs, case):
    secrets, _, _ = JA.inputs(case)
    want = JA.expected(secrets, case.ss.modulus)
    dev = JA.run_case(JA.DeviceBackend(engine), case, every_tiling=True)
    host = JA.run_case(JA.HostBackend(engine), case)
    print(f"CASE {case.id} device_equals_sum={np.array_equal(dev.output, want)} "
          f"host_equals_sum={np.array_equal(host.output, want)}")
    # (c) first: it names the role
    _localise(oracle, case, dev, "device")
    _localise(oracle, case, host, "host")
    _same_tilings(dev, case.id)                                  # (d)
    _same_bytes(dev, host, case.id)                              # (b)
    assert np.array_equal(dev.output, want), "device: (a)"       # (a)
    assert np.array_equal(host.output, want), "host: (a)"
    if case.plan().recipient == "decoded":                       # (e)
        r = len(case.clerks or range(case.ss.output_size())) - JA.kt_of(case.ss)
        for tr in (dev, host):
            assert tr.decode == E.ShareDecode(r, r // 2, 0, 2**64 - 1, 0, [0] * (r + JA.kt_of(case.ss)))
            assert not tr.verdict.any() and not tr.wrong.any()
    print(f"ROUTES {case.id} {_routes(case, dev, host)}")        # (g)


@pytest.mark.parametrize("case", JA.FAULT_CASES, ids=[c.id for c in JA.FAULT_CASES])
def test_misbehaving_clerks(engine, oracle, no_knobs, case):
    """(f)"""
    dev = JA.run_case(JA.DeviceBackend(engine), case)
    host = JA.run_case(JA.HostBackend(engine), case)
    model = JA.run_case(JA.OracleBackend(oracle), case)
    _localise(oracle, case, dev, "device")
    _localise(oracle, case, host, "host")
    _same_bytes(dev, host, case.id)
    assert dev.clerk_payloads == model.clerk_payloads            # the misbehaving clerks' results included
    for tr in (dev, host):
        check_faulty_clerks(case, tr)
        assert tr.decode == model.decode
        assert np.array_equal(tr.verdict, model.verdict) and np.array_equal(tr.wrong, model.wrong)
        assert np.array_equal(tr.output, model.output) and np.array_equal(tr.job_output, model.job_output)
