"""CPU: the draw rule's model (tests/draws_model.py) against the committed RFC 7539 vectors and its own recorded
values, the input condition the GPU retry cases rely on, and the four draws symbols of the library."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from sda_amd import engine as E
from tests import draws_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("sda_draws_dev", "sda_draws", "sda_share_generate_keyed", "sda_secret_mask_keyed")


def test_model_reproduces_rfc7539_blocks():
    coords = DM.rfc_coordinates()
    assert len(coords) == 2
    assert any(first == 0x4800000000000008 for _, _, _, first, _ in coords)
    for name, key, stream_id, first, want in coords:
        assert DM.draws(key, stream_id, first, 8, 1 << 32).tolist() == want, name


@pytest.mark.parametrize("bound", [DM.BOUND_THIRD, DM.BOUND_QUARTER], ids=["third", "quarter"])
def test_large_bounds_force_the_retry_path(bound):
    """A condition on the inputs: with these bounds the GPU cases cannot pass without running retries."""
    _, rounds = DM.draws_with_rounds(DM.TEST_KEY, DM.TEST_STREAM, 0, 4096, bound)
    assert (rounds > 0).mean() >= 0.20
    assert rounds.max() >= 4


def test_model_matches_its_recorded_values():
    recs = json.load(open(os.path.join(GOLDEN, "draws_kat.json")))
    assert len(recs) >= 4
    for r in recs:
        got = DM.draws(tuple(r["key"]), r["stream_id"], r["first"], 16, r["bound"])
        assert got.tolist() == r["draws"], r


def test_library_exports_the_draws_entry_points():
    lib = E.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    key = (C.c_uint32 * 8)()
    out = (C.c_int64 * 4)()
    mlen = C.c_uint64()
    assert lib.sda_draws_dev(None, key, 0, 0, 4, 433, None, None) == E.ERR_INVALID_ARGUMENT
    assert lib.sda_draws(None, key, 0, 0, 4, 433, out, 4) == E.ERR_INVALID_ARGUMENT
    assert lib.sda_share_generate_keyed(None, None, out, 4, key, 0, out, 4) == E.ERR_INVALID_ARGUMENT
    assert lib.sda_secret_mask_keyed(None, None, out, 4, key, 0, out, 4, C.byref(mlen), out) == E.ERR_INVALID_ARGUMENT


def test_python_tile_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "sda_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t kDrawsTile = (\d+);", src).group(1)) == E.DRAWS_TILE
