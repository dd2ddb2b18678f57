"""CPU: the draws kernel's register, scratch and LDS budget (no GPU needed), read from the library the GPU tests
load (scripts/code_objects.py, as tests/test_kernel_resources_encode32.py does)."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

WANT = "draws_kernel"


@pytest.fixture(scope="module")
def kernel():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    rows = [k for k in CO.kernels(E.LIB_PATH) if k["pretty"] == WANT or k["pretty"].startswith(WANT + "(")]
    assert len(rows) == 1, [k["pretty"] for k in rows]
    return rows[0]


def test_draws_kernel_exists_and_uses_no_agprs_scratch_or_spills(kernel):
    assert not kernel["agpr"] and not kernel["scratch"] and not kernel["vgpr_spill"], kernel


def test_draws_kernel_keeps_eight_waves_per_simd(kernel):
    """64 VGPRs is the most at which 8 waves share a SIMD; the write-back tile (256 lanes x 9 u64) is the only LDS,
    so eight workgroups fit a CU's 160 KiB."""
    assert kernel["vgpr"] <= 64, kernel["vgpr"]
    assert 0 < kernel["lds"] <= 160 * 1024 // 8, kernel["lds"]
