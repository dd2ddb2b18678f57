"""CPU: register budgets of the clerk job's device-length encode kernels (codec_encode.hip, job_encode_*), read from
the library the GPU tests load (scripts/code_objects.py, as tests/test_kernel_resources_combine32.py does).

They are the host-length encoder's bodies behind a gate that reads the row's length from a device word, so they must
cost what their siblings cost: no scratch, no spills, no AGPRs, the same static LDS, and a VGPR count in the
sibling's occupancy bucket (gfx950 allocates VGPRs in blocks of 8 out of 512 per SIMD lane: waves per SIMD =
min(8, 512 // roundup(vgpr, 8)))."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

SIBLING = {
    "job_encode_size_kernel": "varint_size_kernel",
    "job_encode_offsets_kernel": "varint_offsets_kernel",
    "job_encode_rows_kernel": "varint_rows_kernel",
    "job_encode_write_kernel<true>": "varint_write_kernel<true>",
    "job_encode_write_kernel<false>": "varint_write_kernel<false>",
}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return {k["pretty"]: k for k in CO.kernels(E.LIB_PATH)}


def _waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def test_the_device_length_encode_kernels_exist_once(kernels):
    all_names = [k["pretty"] for k in CO.kernels(E.LIB_PATH)]
    for name in SIBLING:
        assert all_names.count(name) == 1, name


@pytest.mark.parametrize("name", sorted(SIBLING))
def test_device_length_kernel_costs_what_its_sibling_costs(kernels, name):
    k, s = kernels[name], kernels[SIBLING[name]]
    assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"] and not k["agpr"], k
    assert k["lds"] == s["lds"], (k["lds"], s["lds"])
    assert _waves(k["vgpr"]) >= _waves(s["vgpr"]), (k["vgpr"], s["vgpr"])
