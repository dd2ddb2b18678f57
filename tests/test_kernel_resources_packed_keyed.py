"""CPU: register and LDS budgets of the keyed packed-Shamir share-gen kernels (no GPU needed), read from the library
the GPU tests load (scripts/code_objects.py, as tests/test_kernel_resources.py does).

packed_gen_keyed_kernel / packed_gen32_keyed_kernel share packed_gen_body with their unkeyed siblings: the draws are
made into the same LDS tile image the siblings load them into, and the ChaCha registers are dead before the transform
starts, so each keyed kernel keeps its sibling's LDS and its sibling's waves per EU.
"""
import importlib.util
import os
import re

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

VGPRS_PER_SIMD = 512          # per lane; allocated in blocks of 8


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _args(pretty, family):
    """(L, N3, WIDE / STORE, CANON, LAZY, SIGNBIT) of one instantiation of `family`, else None"""
    m = re.match(re.escape(family) + r"<(\d+), (\d+), (\w+), (\w+), (\w+), (\w+)>$", pretty)
    if not m:
        return None
    third = int(m[3]) if m[3].isdigit() else m[3] == "true"
    return (int(m[1]), int(m[2]), third) + tuple(x == "true" for x in m.groups()[3:])


def _family(kernels, family):
    return {_args(k["pretty"], family): k for k in kernels if _args(k["pretty"], family) is not None}


def gen_waves(L, N3, canon, lazy):
    """packed_gen.hip: gen_waves (amdgpu_waves_per_eu of the share-gen kernels, keyed ones included)."""
    return 2 if N3 >= 81 else (5 if L <= 16 and (canon or lazy) else 4)


def vgpr_cap(waves):
    return VGPRS_PER_SIMD // waves // 8 * 8


@pytest.mark.parametrize("keyed,unkeyed", [("packed_gen_keyed_kernel", "packed_gen_kernel"),
                                           ("packed_gen32_keyed_kernel", "packed_gen32_kernel")])
def test_keyed_set_is_the_unkeyed_set_up_to_27_points(kernels, keyed, unkeyed):
    got, twins = _family(kernels, keyed), _family(kernels, unkeyed)
    want = {a for a in twins if a[1] <= 27}
    assert len(want) >= 48 and set(got) == want, (sorted(set(got) - want), sorted(want - set(got)))
    for a, k in got.items():
        assert k["lds"] == twins[a]["lds"], (k["pretty"], k["lds"], twins[a]["lds"])


def test_keyed_kernels_use_no_agprs_scratch_or_spills(kernels):
    rows = [k for k in kernels if "packed_gen" in k["pretty"] and "keyed" in k["pretty"]]
    names = {k["pretty"] for k in rows}
    assert {"packed_gen_keyed_fixup_kernel", "packed_gen32_keyed_fixup_kernel"} <= names and len(rows) == 98
    bad = [(k["pretty"], k["vgpr"], k["agpr"], k["scratch"], k["vgpr_spill"]) for k in rows
           if k["agpr"] or k["scratch"] or k["vgpr_spill"]]
    assert not bad, bad


def test_keyed_kernels_fit_the_waves_they_ask_for(kernels):
    """amdgpu_waves_per_eu is gen_waves of the unkeyed sibling: 5 waves (102 VGPRs, rounded down to the allocation
    block: 96) for the canonical and lazy kernels, 4 (128) for the non-lazy exact ones."""
    assert (vgpr_cap(5), vgpr_cap(4)) == (96, 128)
    seen = 0
    for family in ("packed_gen_keyed_kernel", "packed_gen32_keyed_kernel"):
        for a, k in _family(kernels, family).items():
            L, N3, _, canon, lazy, _ = a
            assert k["vgpr"] <= vgpr_cap(gen_waves(L, N3, canon, lazy)), (k["pretty"], k["vgpr"])
            seen += 1
    assert seen == 96
    want = {  # the benchmarked pair (configs[2]) and its int32 forms: as the siblings in tests/test_kernel_resources.py
        "packed_gen_keyed_kernel<16, 27, true, true, false, false>": 102,
        "packed_gen_keyed_kernel<16, 27, true, false, true, true>": 102,
        "packed_gen32_keyed_kernel<16, 27, 1, true, false, false>": 102,
        "packed_gen32_keyed_kernel<16, 27, 1, false, true, true>": 102,
    }
    for name, cap in want.items():
        rows = [k for k in kernels if k["pretty"] == name]
        assert len(rows) == 1 and rows[0]["vgpr"] <= cap, (name, rows)
