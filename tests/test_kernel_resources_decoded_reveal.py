"""CPU: the decoded reveal's kernels in the built library (scripts/code_objects.py, as tests/test_kernel_resources.py
reads it): every packed_decode instantiation exists once, none has AGPRs, scratch, VGPR or SGPR spills or LDS (the
decoder's syndromes, locator and evaluator are registers at compile-time indices), and each stays inside 256 VGPRs.
The VGPR count of each RMAX is recorded (DESIGN.md §4.2 states them)."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

RMAX = (4, 8, 12, 16, 32)
EXPECTED = [f"packed_decode_kernel<{m}>" for m in RMAX] + [f"packed_decode32_kernel<{m}>" for m in RMAX]


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _rows(kernels):
    return [k for k in kernels if k["pretty"].startswith("packed_decode")]


def test_every_decode_instantiation_exists_once(kernels):
    names = [k["pretty"] for k in _rows(kernels)]
    assert sorted(names) == sorted(EXPECTED), names


def test_decode_kernels_match_no_other_familys_prefix(kernels):
    for k in _rows(kernels):
        assert not k["pretty"].startswith(("packed_check", "packed_repair", "packed_reveal"))


def test_decode_kernels_use_no_agprs_scratch_spills_or_lds(kernels):
    bad = [(k["pretty"], k["vgpr"], k["agpr"], k["scratch"], k["vgpr_spill"], k["sgpr_spill"], k["lds"])
           for k in _rows(kernels)
           if k["agpr"] or k["scratch"] or k["vgpr_spill"] or k["sgpr_spill"] or k["lds"] or k["vgpr"] > 256]
    assert not bad, bad


@pytest.mark.parametrize("rmax", RMAX)
@pytest.mark.parametrize("width", ("", "32"))
def test_register_count_of_each_rmax_is_recorded(kernels, rmax, width, record_property):
    by = {k["pretty"]: k for k in kernels}
    k = by[f"packed_decode{width}_kernel<{rmax}>"]
    record_property("decode_vgpr", k["vgpr"])
    print(f"{k['pretty']}: {k['vgpr']} VGPRs")
    assert k["vgpr"] <= 256
