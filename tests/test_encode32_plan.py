"""CPU: the plan of tests/test_gpu_encode32.py (tests/encode32_cases.py) against the source and the oracle."""
import os
import re

import numpy as np
import pytest

from sda_amd import engine as E
from tests import encode32_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_constant_mirrors_the_source():
    src = open(os.path.join(ROOT, "sda_amd", "csrc", "codec_encode.hip")).read()
    m = re.search(r"^#define SDA_ENC32_CHUNK (\d+)", src, flags=re.M)
    assert m and int(m[1]) == EC.ENC32_CHUNK
    assert "constexpr uint32_t kEnc32Chunk = SDA_ENC32_CHUNK;" in src


def test_bindings_declare_the_int32_entry_points():
    names = {s[0] for s in E.SIGNATURES}
    assert {"sda_varint_encode32_dev", "sda_participant_share32_dev"} <= names
    assert callable(E.Engine.varint_encode32_dev) and callable(E.Engine.participant_share32_dev)


def test_planted_values_have_their_sizes(oracle):
    for v, size in EC.planted():
        assert len(oracle.varint_encode(np.array([v], np.int64))) == size, v
    for s in range(1, 6):
        lo, hi = EC.class_bounds(s)
        for z in (lo, hi):
            assert len(oracle.varint_encode(EC.unzigzag([z]).astype(np.int64))) == s


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.id)
def test_case_holds_what_it_is_meant_to(oracle, case):
    C = EC.C
    v = EC.case_values(case)
    payload, row_bytes = EC.case_expected(case)
    EC.check_classes(case, payload)
    assert int(row_bytes.sum()) == len(payload)
    assert case.stride >= case.length and (v[:, case.length:] == EC.PAD).all()
    if case.kind == "mixed":
        sizes = EC.element_sizes(payload)
        assert sizes.size == case.rows * case.length
        per_row = sizes.reshape(case.rows, case.length)
        for c in range(1, 4):                      # 5 bytes | chunk boundary | 1 byte
            if c * C < case.length:
                assert (per_row[:, c * C - 1] == 5).all() and (per_row[:, c * C] == 1).all()
    else:
        assert int(row_bytes[0]) == 5 * case.length and int(row_bytes[1]) == case.length


def test_participant_schemes_take_the_routes_they_name():
    """tests/test_gpu_participant32.py: at D = 4099, at both shares_out offsets it uses and in BOTH modes, the
    n + 1 = 81 scheme stays on the register kernels (so sda_participant_share32_dev writes i64 shares into scratch
    and narrows them), CONFIG_PACKED on the direct int32 kernels (n + 1 <= 27), the n + 1 = 243 scheme on the
    workspace kernels -- by tests/packed_dispatch.py, the restatement of launch_packed_generate's choice."""
    from tests import packed_dispatch as PD
    sch = EC.participant_schemes()
    assert list(sch) == ["packed", "n80-scratch", "n242-workspace"]
    for name, s in sch.items():
        B = -(-EC.PARTICIPANT_D // s.secret_count)
        assert EC.PARTICIPANT_D % s.secret_count, "the last batch is ragged"
        assert s.privacy_threshold() > 0
        for mode in (PD.EXACT, PD.CANONICAL):
            for off in (0, 4):
                kernel = PD.gen_kernel(s, B, off, mode)
                if name == "n242-workspace":
                    assert kernel == "wide", (name, mode, off, kernel)
                else:
                    n3 = s.share_count + 1
                    assert kernel.startswith(f"packed_gen_kernel<{s.secret_count + s.privacy_threshold() + 1}, {n3},"), \
                        (name, mode, off, kernel)
                    assert n3 == (81 if name == "n80-scratch" else 27)


def test_shapes_reach_the_paths_they_name():
    C = EC.C
    by = {c.name: c for c in EC.CASES}
    assert by["1-row-scan-carry"].rows > 256 and by["1-row-scan-carry"].length < C
    assert -(-EC.CASE2.length // C) > 256 and EC.CASE2.length % C
    assert EC.CASE3.stride % 4 == 1 and EC.CASE3.length > 3 * C and EC.CASE3.length % C
    assert sorted((r * EC.CASE3.stride * 4) % 16 for r in range(4)) == [0, 4, 8, 12]
    assert by["4-extremes"].length % C == 0
