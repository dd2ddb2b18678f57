"""CPU: register and LDS budgets of the int32 packed-Shamir kernels (no GPU needed), read from the library the GPU
tests load (scripts/code_objects.py, as tests/test_kernel_resources.py does).

The int32 kernels (packed_gen32_*, packed_reveal32_*, packed_reveal_fixup_kernel<.., int>) share their bodies
with the i64 kernels and differ only in the share loads / stores, so they keep the twins' budgets: no AGPRs, no
scratch, no spills -- except the reveal fix-up's generic path, whose private i64 array is scratch by design and
which keeps the allow-listed prefix `packed_reveal_fixup_kernel<`."""
import importlib.util
import os
import re

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

FIXUP = "packed_reveal_fixup_kernel<"
LDS_PER_CU = 160 << 10
SIMDS_PER_CU = 4


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _is32(pretty):
    return pretty.startswith(("packed_gen32_", "packed_reveal32_")) or (pretty.startswith(FIXUP) and pretty.endswith(", int>"))


def _gen32_args(pretty):
    m = re.match(r"packed_gen32_kernel<(\d+), (\d+), (\d+), (\w+), (\w+), (\w+)>", pretty)
    return None if not m else (int(m[1]), int(m[2]), int(m[3])) + tuple(x == "true" for x in m.groups()[3:])


def test_int32_packed_kernels_exist_and_use_no_agprs_scratch_or_spills(kernels):
    rows = [k for k in kernels if _is32(k["pretty"])]
    names = {k["pretty"] for k in rows}
    for want in ("packed_gen32_kernel<16, 27, 1, true, false, false>", "packed_gen32_fixup_kernel",
                 "packed_gen32_wide_kernel", "packed_reveal32_wide_kernel",
                 "packed_reveal32_exact_kernel<16, true, 8, true, true>", "packed_reveal32_canon_kernel<16, true>",
                 "packed_reveal32_fixup_wave_kernel<16>", "packed_reveal_fixup_kernel<96, 0, int>"):
        assert want in names, want
    bad = [(k["pretty"], k["vgpr"], k["agpr"], k["scratch"], k["vgpr_spill"]) for k in rows
           if (k["agpr"] or k["scratch"] or k["vgpr_spill"] or k["vgpr"] > 256) and not k["pretty"].startswith(FIXUP)]
    assert not bad, bad
    fix = [(k["pretty"], k["agpr"]) for k in rows if k["pretty"].startswith(FIXUP) and k["agpr"]]
    assert not fix, fix


def test_share_gen32_instantiations_mirror_the_i64_set_up_to_27_points(kernels):
    """<L, N3, STORE, CANON, LAZY, SIGNBIT> for every Makefile GEN_PART with n + 1 <= 27: the lazy kernels with
    the pair store (1), the others with the pair store and the one-batch-per-lane store (0); nothing at
    n + 1 = 81 (scratch + narrowing), and no other STORE value (a 16-byte quad store, 2, measured slower and was
    removed: DESIGN.md §4.2)."""
    seen = {_gen32_args(k["pretty"]) for k in kernels}
    seen.discard(None)
    expect = set()
    for n3, ls in ((3, (2,)), (9, (2, 4, 8)), (27, (2, 4, 8, 16))):
        for L in ls:
            expect |= {(L, n3, 1, False, True, True), (L, n3, 1, False, True, False)}
            for store in (0, 1):
                expect |= {(L, n3, store, True, False, False), (L, n3, store, False, False, False)}
    assert seen == expect, (sorted(seen - expect), sorted(expect - seen))


def test_configs2_int32_kernels_keep_their_twins_caps(kernels):
    want = {  # kernel prefix -> max VGPRs (tests/test_kernel_resources.py, the i64 twins)
        "packed_gen32_kernel<16, 27, 1, true, false, false>": 102,    # canonical, 5 waves
        "packed_gen32_kernel<16, 27, 1, false, true, true>": 102,     # exact sign-bit, 5 waves
        "packed_reveal32_exact_kernel<16, true, 8, true, true>": 64,  # exact reveal, 8 waves
        "packed_reveal32_canon_kernel<16, true>": 128,
    }
    for prefix, cap in want.items():
        rows = [k for k in kernels if k["pretty"].startswith(prefix)]
        assert rows, prefix
        for k in rows:
            assert k["vgpr"] <= cap and not k["scratch"] and not k["vgpr_spill"] and not k["agpr"], (k["pretty"], k["vgpr"])


def test_reveal32_kernels_have_no_static_lds(kernels):
    """reveal_flush reads the results back from the dynamic LDS base as 16-byte words: that base is 16-byte
    aligned only while no static LDS precedes it."""
    rows = [k for k in kernels if k["pretty"].startswith(("packed_reveal32_exact_kernel<", "packed_reveal32_canon_kernel<"))]
    assert len(rows) >= 15
    assert all(k["lds"] == 0 for k in rows), [(k["pretty"], k["lds"]) for k in rows if k["lds"]]


def test_share_gen32_lds_allows_its_waves_per_eu(kernels):
    """The int32 stores take no LDS of their own (the LDS-staged 16-byte flush was not built), so the
    static LDS is the i64 twin's input stage: at L <= 16 the canonical and lazy kernels ask for 5 waves per
    EU = 5 workgroups of 4 waves per CU, which must fit 160 KiB."""
    for k in kernels:
        a = _gen32_args(k["pretty"])
        if a is None:
            continue
        L, _, _, canon, lazy, _ = a
        if L <= 16 and (canon or lazy):
            wgs = 5 * SIMDS_PER_CU // (256 // 64)
            assert wgs * k["lds"] <= LDS_PER_CU, (k["pretty"], k["lds"])
        twin = "packed_gen_kernel<%d, %d, %s, %s, %s, %s>" % (
            a[0], a[1], "true" if a[2] else "false", *("true" if x else "false" for x in a[3:]))
        t = [x for x in kernels if x["pretty"] == twin]
        assert t and t[0]["lds"] == k["lds"], (k["pretty"], k["lds"], twin)
