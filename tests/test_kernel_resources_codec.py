"""CPU: the share payload codec's kernels after the split into codec_decode.hip and codec_encode.hip (no GPU needed),
read from the library the GPU tests load (scripts/code_objects.py, as tests/test_kernel_resources_encode32.py does):
the two objects hold the codec's 32 kernels, each once, and the encode kernels, which share one size body and one
write body, keep the budgets of the separate kernels they replaced."""
import importlib.util
import os

import pytest

from sda_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

ENCODE = ("varint_size_kernel", "varint_size32_kernel", "varint_write_kernel<true>", "varint_write_kernel<false>",
          "varint_write32_kernel<true>", "varint_write32_kernel<false>")
WANT = ENCODE + (
    "varint_offsets_kernel", "varint_rows_kernel", "varint_count_kernel", "varint_scan_kernel", "varint_cap_kernel",
    "varint_sequential_kernel", "varint_tile_plan_kernel", "slot_dims_kernel", "slot_plan_kernel",
    "slot_commit_kernel",
) + tuple(f"slot_combine_kernel<{c}, 8, {sm}>" for c in (1, 2, 4) for sm in ("true", "false")) + (
    "varint_decode_kernel<int, false, false>", "varint_decode_kernel<int, false, true>",
    "varint_decode_kernel<int, true, false>", "varint_decode_kernel<int, true, true>",
    "varint_decode_kernel<long, false, false>", "varint_decode_kernel<long, false, true>",
    "varint_decode_combine_kernel<2, true>", "varint_decode_combine_kernel<2, false>",
    "varint_decode_combine_kernel<4, false>", "varint_decode_combine_kernel<8, false>",
)
# static LDS in bytes: the write kernels' chunk image ((chunk * 10 + 32) / 16 and (chunk * 5 + 30) / 16 quads) plus
# the four wave sums of the block scan; the size kernels' four wave sums (u64 and u32)
LDS = {"varint_write_kernel<true>": 20528, "varint_write_kernel<false>": 20528,
       "varint_write32_kernel<true>": 10272, "varint_write32_kernel<false>": 10272,
       "varint_size_kernel": 32, "varint_size32_kernel": 16}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    return CO.kernels(E.LIB_PATH)


def _is_codec(pretty):
    return pretty.startswith(("varint_", "slot_"))


def test_the_two_codec_objects_hold_the_32_codec_kernels_each_once(kernels):
    assert len(WANT) == len(set(WANT)) == 32
    got = sorted(k["pretty"] for k in kernels if _is_codec(k["pretty"]))
    assert got == sorted(WANT), (sorted(set(got) - set(WANT)), sorted(set(WANT) - set(got)),
                                 sorted(n for n in set(got) if got.count(n) > 1))


def test_encode_kernels_keep_their_budgets(kernels):
    by_name = {k["pretty"]: k for k in kernels if k["pretty"] in ENCODE}
    assert sorted(by_name) == sorted(ENCODE)
    for name in ENCODE:
        k = by_name[name]
        assert k["lds"] == LDS[name], (name, k["lds"])
        assert not k["agpr"] and not k["scratch"] and not k["vgpr_spill"], (name, k)
        # 8 waves per SIMD; LDS bounds the occupancy of these kernels, not registers
        assert k["vgpr"] <= 64, (name, k["vgpr"])
