"""Writes tests/golden/draws_kat.json: a few (key, stream_id, first, bound) -> 16-value records of the draws model
(tests/draws_model.py), so that drift in the model is caught (tests/test_draws_model.py).  CPU only.
    python scripts/gen_draws_kat.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import draws_model as DM  # noqa: E402

CASES = [  # (key, stream_id, first, bound)
    (DM.TEST_KEY, 0, 0, 433),
    (DM.TEST_KEY, 7, 3, 2147482800),
    ((0,) * 8, 0, 0, 1),
    (DM.TEST_KEY, DM.TEST_STREAM, 2045, DM.BOUND_THIRD),
    (DM.TEST_KEY, DM.TEST_STREAM, 4096 - 8, DM.BOUND_QUARTER),
    (tuple(range(1, 9)), 0xFFFFFFFF, (1 << 35) - 5, (1 << 63) - 1),
]
recs = [{"key": list(k), "stream_id": s, "first": f, "bound": b, "draws": DM.draws(k, s, f, 16, b).tolist()}
        for k, s, f, b in CASES]
with open(os.path.join(ROOT, "tests", "golden", "draws_kat.json"), "w") as fh:
    json.dump(recs, fh, indent=1)
    fh.write("\n")
