"""CPU: the fused Full-mask kernel's register, scratch and LDS budget (no GPU needed), read from the library the GPU
tests load (scripts/code_objects.py, as tests/test_kernel_resources_draws.py does).  The figures are those DESIGN.md
§4.6 states."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

WANT = "full_mask_keyed_kernel"
INSTANCES = ("long", "int")                 # MaskOut = int64_t, int32_t
LDS_BYTES = 256 * 9 * 8                     # the write-back tile: 256 lanes x 9 u64


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    rows = [k for k in CO.kernels(E.LIB_PATH) if k["pretty"].startswith(WANT + "<")]
    return {k["pretty"][len(WANT) + 1:].split(">")[0]: k for k in rows}, rows


def test_both_instantiations_exist_exactly_once(kernels):
    by_type, rows = kernels
    assert len(rows) == 2 and sorted(by_type) == sorted(INSTANCES), [k["pretty"] for k in rows]


@pytest.mark.parametrize("out", INSTANCES)
def test_no_agprs_scratch_or_spills(kernels, out):
    k = kernels[0][out]
    assert not k["agpr"] and not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k


@pytest.mark.parametrize("out", INSTANCES)
def test_eight_waves_per_simd(kernels, out):
    """64 VGPRs is the most at which 8 waves share a SIMD -- the draws kernel's occupancy, with a lane's eight
    secrets held across the ChaCha rounds; the write-back tile is the only LDS, so eight workgroups fit a CU's
    160 KiB."""
    k = kernels[0][out]
    assert k["vgpr"] <= 64, k["vgpr"]
    assert k["lds"] == LDS_BYTES and 8 * k["lds"] <= 160 * 1024, k["lds"]
