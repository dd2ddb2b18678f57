"""CPU: register budgets of the int32 combine and narrowing kernels (no GPU needed), read from the library the
GPU tests load (scripts/code_objects.py, as tests/test_kernel_resources.py does).

The 4-columns-per-lane int32 combine keeps the i64 default's occupancy (8 waves per SIMD) only within 64 VGPRs;
its four accumulators and the m > 2^62 slow path cost more registers than the i64 sibling's two, so the rows per
batch are chosen to stay under the cap (combine.hip, kWide32Rows)."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _clean(k):
    return not k["scratch"] and not k["vgpr_spill"] and not k["agpr"]


def test_wide_int32_combine_kernels_fit_64_vgprs(kernels):
    rows = [k for k in kernels if k["pretty"].startswith("combine_exact_kernel<int, 4,")]
    assert rows, "no combine_exact_kernel<int, 4, ...> in the library"
    bad = [(k["pretty"], k["vgpr"], k["scratch"], k["vgpr_spill"]) for k in rows if k["vgpr"] > 64 or not _clean(k)]
    assert not bad, bad
    # the software-pipelined instantiations of the public entry points, plain and accumulating, both modulus ranges
    # <int, 4, ROWS, SMALL_M, ACC, FLAG = false, PIPE = true>
    piped = {tuple(k["pretty"].split("<", 1)[1].rstrip(">").split(", ")[3:]) for k in rows
             if k["pretty"].rstrip(">").endswith("true")}
    assert piped == {(s, a, "false", "true") for s in ("true", "false") for a in ("true", "false")}, piped


def test_int32_accumulating_kernels_exist(kernels):
    """ACC = true for every lane width the int32 dispatch can take."""
    for vec in (1, 2, 4):
        rows = [k for k in kernels if k["pretty"].startswith(f"combine_exact_kernel<int, {vec}, ")
                and k["pretty"].split(", ")[4] == "true"]
        assert rows, vec
        assert all(_clean(k) for k in rows), [(k["pretty"], k["scratch"], k["vgpr_spill"]) for k in rows]


def test_narrow32_kernels_have_no_scratch(kernels):
    rows = [k for k in kernels if k["pretty"].startswith("narrow32_kernel")]
    assert len(rows) >= 2, [k["pretty"] for k in rows]           # 16-byte and scalar
    assert all(_clean(k) for k in rows), [(k["pretty"], k["scratch"], k["vgpr_spill"]) for k in rows]
