"""CPU: the share consistency check's kernels in the built library (scripts/code_objects.py, as
tests/test_kernel_resources.py reads it): every instantiation exists once, none has AGPRs, scratch or spills, none
has static LDS, and each register bucket fits the VGPRs of the canonical reveal kernel of the same bucket -- it
holds the same shares and stages no output."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

BUCKETS = (8, 16, 32)
EXPECTED = ([f"packed_check_kernel<{b}>" for b in BUCKETS] + [f"packed_check32_kernel<{b}>" for b in BUCKETS] +
            ["packed_check_loop_kernel", "packed_check32_loop_kernel", "packed_check_locate_kernel",
             "packed_check32_locate_kernel"])


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _check_rows(kernels):
    return [k for k in kernels if k["pretty"].startswith("packed_check")]


def test_every_check_instantiation_exists_once(kernels):
    names = [k["pretty"] for k in _check_rows(kernels)]
    assert sorted(names) == sorted(EXPECTED), names


def test_check_kernels_use_no_agprs_scratch_spills_or_static_lds(kernels):
    bad = [(k["pretty"], k["vgpr"], k["agpr"], k["scratch"], k["vgpr_spill"], k["sgpr_spill"], k["lds"])
           for k in _check_rows(kernels)
           if k["agpr"] or k["scratch"] or k["vgpr_spill"] or k["sgpr_spill"] or k["lds"] or k["vgpr"] > 256]
    assert not bad, bad


@pytest.mark.parametrize("bucket", BUCKETS)
@pytest.mark.parametrize("width", ("", "32"))
def test_register_bucket_fits_the_canonical_reveal_of_the_same_bucket(kernels, bucket, width):
    by = {k["pretty"]: k for k in kernels}
    check = by[f"packed_check{width}_kernel<{bucket}>"]
    reveal = by[f"packed_reveal{width}_canon_kernel<{bucket}, true>"]
    assert check["vgpr"] <= reveal["vgpr"], (check["pretty"], check["vgpr"], reveal["pretty"], reveal["vgpr"])
