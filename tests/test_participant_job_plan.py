"""CPU: the participant job's payload bound and tile plan (sda_amd/csrc/participant_job_plan.h).

sda_participant_job_payload_bound needs no device: it is called through the library here and held to the oracle's
encoding of the extreme shares +-(m - 1) and of the extreme mask value m - 1.  tests/host_c/participant_job_plan.cc is
a stand-alone program (its own main) that includes the header -- the bound against a scalar encoder and the tile
plan's ranges -- compiled here with ROCm's clang++ under AddressSanitizer and UBSan and run as a child process; the
sanitizer runtimes are linked into the program itself.
"""
import os
import shutil
import subprocess

import pytest

from sda_amd import SdaError, schemes as S
from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "participant_job_plan.cc")
MODULI = (433, 2147482801, 2**31, 2**31 + 1, 6148914691236517205)
CP = S.CONFIG_PACKED


@pytest.mark.parametrize("m", MODULI, ids=[f"m{m}" for m in MODULI])
def test_bound_is_the_oracle_encoding_of_the_extreme_values(oracle, m):
    per = max(len(oracle.varint_encode([m - 1])), len(oracle.varint_encode([-(m - 1)])))
    assert per == (2 if m == 433 else 5 if m <= 2**31 + 1 else 10)
    for n in (2, 3):
        for d in (0, 1, 7, 2049):
            # Additive: d shares a clerk; a Full mask of d values in [0, m)
            assert E.participant_job_payload_bound(S.FullMasking(m), S.Additive(n, m), d) == (d * per, d * per)
            assert E.participant_job_payload_bound(S.NoMasking(), S.Additive(n, m), d) == (d * per, 0)
            # a ChaCha seed word `as i64` is below 2^32: 5 bytes, whatever the dimension
            for bits, words in ((0, 0), (32, 1), (256, 8), (288, 9)):
                assert len(oracle.varint_encode([2**32 - 1])) == 5
                assert E.participant_job_payload_bound(S.ChaChaMasking(m, d, bits), S.Additive(n, m), d) == \
                    (d * per, 5 * words)
    # the worst row is met: d extreme shares encode to exactly the bound
    assert len(oracle.varint_encode([m - 1, -(m - 1)] * 4)) <= 8 * per
    assert len(oracle.varint_encode([m - 1] * 8)) == 8 * per or len(oracle.varint_encode([-(m - 1)] * 8)) == 8 * per


def test_packed_bound_counts_batches():
    p, k = CP.prime_modulus, CP.secret_count
    for d in (0, 1, k - 1, k, k + 1, 2049):
        B = (d + k - 1) // k
        assert E.participant_job_payload_bound(S.FullMasking(p), CP, d) == (5 * B, 5 * d)
    fl = S.FULL_LOOP_PACKED
    assert E.participant_job_payload_bound(S.NoMasking(), fl, 10) == (2 * 4, 0)


def test_one_additive_clerk_is_bounded_by_the_mask():
    """share_count 1 hands the masked secret out as it stands: the masking modulus bounds it, no masking nothing."""
    assert E.participant_job_payload_bound(S.NoMasking(), S.Additive(1, 433), 3) == (30, 0)
    assert E.participant_job_payload_bound(S.FullMasking(2147482801), S.Additive(1, 433), 3) == (15, 15)


def test_bound_statuses():
    bad = S.FullMasking(433)
    ms = bad.c()
    ms.kind = 7
    import ctypes as C
    row, mask = C.c_uint64(), C.c_uint64()
    lib = E.load_library()
    ss = S.Additive(2, 433).c()
    assert lib.sda_participant_job_payload_bound(C.byref(ms), C.byref(ss), 1, C.byref(row), C.byref(mask)) == \
        E.ERR_INVALID_ARGUMENT
    assert lib.sda_participant_job_payload_bound(None, C.byref(ss), 1, C.byref(row), C.byref(mask)) == \
        E.ERR_INVALID_ARGUMENT
    with pytest.raises(SdaError) as ei:
        E.participant_job_payload_bound(S.NoMasking(), S.Additive(70000, 433), 1)
    assert ei.value.status == E.ERR_UNSUPPORTED
    with pytest.raises(SdaError) as ei:
        E.participant_job_payload_bound(S.NoMasking(), S.Additive(1, 433), 2**62)      # 10 bytes a value
    assert ei.value.status == E.ERR_INVALID_ARGUMENT


def _clangxx():
    for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or ""):
        if p and os.path.exists(p):
            return p
    return None


def test_plan_header_under_sanitizers(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not available")
    exe = tmp_path / "participant_job_plan"
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-O1", "-g", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    tail = (run.stdout + run.stderr)[-4000:]
    assert run.returncode == 0, tail
    assert run.stdout.strip().endswith("participant_job_plan OK"), tail
