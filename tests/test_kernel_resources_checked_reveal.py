"""CPU: the checked reveal's kernels in the built library (scripts/code_objects.py, as tests/test_kernel_resources.py
reads it): every packed_repair instantiation exists once, none has AGPRs, scratch or spills, none has static LDS (the
staged flush is dynamic LDS, as the canonical reveal's), and each register bucket stays inside 256 VGPRs.  The VGPR
count of each bucket is recorded next to the canonical reveal's of the same bucket (DESIGN.md §4.2 states them)."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

BUCKETS = (8, 16, 32)
EXPECTED = ([f"packed_repair_kernel<{b}>" for b in BUCKETS] + [f"packed_repair32_kernel<{b}>" for b in BUCKETS] +
            ["packed_repair_fix_kernel", "packed_repair32_fix_kernel"])


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _rows(kernels):
    return [k for k in kernels if k["pretty"].startswith("packed_repair")]


def test_every_repair_instantiation_exists_once(kernels):
    names = [k["pretty"] for k in _rows(kernels)]
    assert sorted(names) == sorted(EXPECTED), names


def test_repair_kernels_match_no_other_familys_prefix(kernels):
    for k in _rows(kernels):
        assert not k["pretty"].startswith(("packed_check", "packed_reveal"))


def test_repair_kernels_use_no_agprs_scratch_spills_or_static_lds(kernels):
    bad = [(k["pretty"], k["vgpr"], k["agpr"], k["scratch"], k["vgpr_spill"], k["sgpr_spill"], k["lds"])
           for k in _rows(kernels)
           if k["agpr"] or k["scratch"] or k["vgpr_spill"] or k["sgpr_spill"] or k["lds"] or k["vgpr"] > 256]
    assert not bad, bad


@pytest.mark.parametrize("bucket", BUCKETS)
@pytest.mark.parametrize("width", ("", "32"))
def test_register_bucket_is_recorded_next_to_the_canonical_reveal(kernels, bucket, width, record_property):
    by = {k["pretty"]: k for k in kernels}
    repair = by[f"packed_repair{width}_kernel<{bucket}>"]
    reveal = by[f"packed_reveal{width}_canon_kernel<{bucket}, true>"]
    record_property("repair_vgpr", repair["vgpr"])
    record_property("reveal_canon_vgpr", reveal["vgpr"])
    print(f"{repair['pretty']}: {repair['vgpr']} VGPRs; {reveal['pretty']}: {reveal['vgpr']} VGPRs")
    assert repair["vgpr"] <= 256
