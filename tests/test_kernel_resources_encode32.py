"""CPU: register, scratch and LDS budgets of the int32 varint encode kernels (no GPU needed), read from the library
the GPU tests load (scripts/code_objects.py, as tests/test_kernel_resources_packed32.py does)."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

WANT = ("varint_size32_kernel", "varint_write32_kernel<true>", "varint_write32_kernel<false>")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _one(kernels, name):
    rows = [k for k in kernels if k["pretty"] == name or k["pretty"].startswith(name + "(")]
    assert len(rows) == 1, (name, [k["pretty"] for k in rows])
    return rows[0]


def test_int32_encode_kernels_exist_and_use_no_agprs_scratch_or_spills(kernels):
    for name in WANT:
        k = _one(kernels, name)
        assert not k["agpr"] and not k["scratch"] and not k["vgpr_spill"], (name, k)


def test_write32_static_lds_is_at_most_the_i64_write_kernels(kernels):
    cap = _one(kernels, "varint_write_kernel<true>")["lds"]
    assert cap > 0
    for name in WANT[1:]:
        lds = _one(kernels, name)["lds"]
        assert 0 < lds <= cap, (name, lds, cap)
