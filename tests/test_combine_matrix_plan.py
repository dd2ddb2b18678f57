"""CPU: the plan of tests/test_gpu_combine_matrix.py against the share-combine instantiations in the built library
(scripts/code_objects.py, as tests/test_kernel_resources.py reads them), against the oracle and against itself.

Every combine_exact_kernel / combine_replay_kernel instantiation that ships must be the kernel
tests/combine_dispatch.py predicts for at least one planned case, and no case may predict a name the library lacks.
The steering model (tests/combine_matrix_cases.py, Python integers) must agree with oracle.combine on every case's
inputs, and every case must hit each event its element type, modulus and row count can reach.
"""
import importlib.util
import os

import numpy as np
import pytest

from sda_amd import engine as E
from tests import combine_dispatch as CB
from tests import combine_matrix_cases as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

FAMILIES = ("combine_exact_kernel<", "combine_replay_kernel<")


@pytest.fixture(scope="module")
def shipped():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    names = {k["pretty"] for k in CO.kernels(E.LIB_PATH) if k["pretty"].startswith(FAMILIES)}
    assert len(names) >= 38, "the fat binary parser found too few combine kernels"
    return names


def _planned():
    return {c.kernel for c in CM.EXACT_CASES + CM.REPLAY_CASES}


def test_every_shipped_instantiation_is_claimed_by_a_case(shipped):
    unclaimed = sorted(shipped - _planned())
    assert not unclaimed, f"instantiations no case of the matrix runs: {unclaimed}"
    print(f"{len(shipped)} instantiations, all claimed")


def test_no_case_predicts_a_kernel_the_library_lacks(shipped):
    invented = sorted(_planned() - shipped)
    assert not invented, f"predicted kernels missing from the library: {invented}"


def test_every_case_reaches_the_kernel_it_names():
    """The dispatcher's rules, applied to the case's shape, alignment and knobs at every row count it runs, give
    the instantiation the case names (device buffers are at least 256-byte aligned: base address 0 here)."""
    for c in CM.EXACT_CASES:
        for n in c.ns:
            p = c.predicted(n)
            assert p.kernel == c.kernel, (c.id, n, p.kernel)
            assert (p.kind, p.elem_bytes, p.vec, p.rows) == (CB.EXACT, c.inst.elem_bytes, c.inst.vec, c.inst.rows)
            assert p.variant == ((CB.SMALL_M if c.small else 0) | (CB.ACC if c.acc else 0) |
                                 (CB.FLAG if c.flag else 0) | (CB.PIPE if c.inst.pipe else 0))
    for c in CM.REPLAY_CASES:
        for n in c.ns:
            p = c.predicted(n)
            assert p.kernel == c.kernel and (p.kind, p.vec, p.rows) == (CB.REPLAY, c.vec, 8), (c.id, n, p)


def test_plan_shapes():
    """Two workgroups with a 3-lane tail; every instantiation runs its whole row-count set at its main modulus and
    the first and last modulus of its class; every modulus of the issue runs; each alignment fall-back runs."""
    by_kernel = {}
    for c in CM.EXACT_CASES:
        assert c.shape.dim in (c.inst.vec * CM.LANES, 2 * c.inst.vec * CM.LANES)
        by_kernel.setdefault(c.kernel, []).append(c)
    assert len(by_kernel) == 34
    for kernel, cases in by_kernel.items():
        u = cases[0].inst.rows
        small = cases[0].small
        assert any(set(c.ns) >= {0} | set(CM.row_counts(u)) for c in cases), kernel
        moduli = {c.m for c in cases}
        cls = CM.SMALL_MODULI if small else CM.BIG_MODULI
        assert {cls[0], cls[-1]} <= moduli and (CM.P in moduli or 2**63 - 25 in moduli), (kernel, moduli)
    assert {c.m for c in CM.EXACT_CASES} == set(CM.SMALL_MODULI + CM.BIG_MODULI)
    assert CM.row_counts(4) == (1, 3, 4, 5, 8, 9, 12, 15, 17) and CM.row_counts(2) == (1, 2, 3, 4, 5, 6, 7, 9)
    tags = {(c.inst.tag, c.shape.tag) for c in CM.EXACT_CASES}
    for want in (("int_2_8", "out_16mod32"), ("int_2_8", "in_8mod16"), ("int_2_8", "stride_2mod4"),
                 ("int_2_8", "dim_2mod4"), ("int_2_8", "vec2_knob"), ("int_1_8", "in_4mod8"), ("int_1_8", "out_8mod16"),
                 ("long_1_8", "odd_dim"), ("long_1_8", "odd_stride"), ("long_1_8", "in_8mod16"),
                 ("long_1_8", "out_8mod16"), ("int_4_8", "pipe0"), ("long_2_8", "pipe0")):
        assert want in tags, want
    assert len({c.m for c in CM.EXACT_CASES if c.inst.tag == "int_4_8"}) > 1         # SDA_COMBINE_PIPE=0, int32
    modes = {(c.kernel, c.flag_mode) for c in CM.EXACT_CASES if c.flag_mode}
    assert len(modes) == 6 * 5                   # every FLAG instantiation: the four outcomes and a word already 1
    assert {c.shape.tag for c in CM.REPLAY_CASES if c.vec == 1} >= {"odd_dim", "code_4mod8", "in_8mod16"}
    replay = {}
    for c in CM.REPLAY_CASES:
        replay.setdefault(c.kernel, set()).add(c.m)
    assert len(replay) == 4
    for kernel, moduli in replay.items():
        cls = CM.SMALL_MODULI if CM.P in moduli else CM.BIG_MODULI
        assert {cls[0], cls[-1]} <= moduli and (CM.P in moduli or 2**63 - 25 in moduli), (kernel, moduli)


# The events a case cannot reach, written out per element type, modulus class and ACC (cases of n >= 2 rows; a plain
# case of one row starts from r == 0 and also misses X+-, and with i64 rows the two wraps):
W4 = {"W+max", "W+wrap", "W-min", "W-wrap"}
SV = {"S+m", "S-m", "S+m1", "S-m1"}
VM = {"V+m", "V-m", "V+m1", "V-m1"}
X2 = {"X+", "X-"}


def _unreachable(elem_bytes, m, acc):
    if elem_bytes == 8:
        if m == 1:
            return {"W+wrap", "W-wrap"}          # r is always 0: r + v cannot leave i64
        return {"X+"} if m == 2**63 - 1 else set()               # m + 1 is no i64 value
    if m < 2**31:                                # int32 rows, m < 2^31: the +-m family, never the i64 wraps
        return W4 | ({"X+"} if m == 2**31 - 1 else set())
    if not acc:                                  # larger m, from 0: only v == 0 and the int32 limits (and r + v == 0)
        return W4 | SV | VM | X2
    if m <= 2**63 - 2**31:                       # an accumulator near +-m puts the sums in reach, not the wraps
        return W4 | VM | X2
    return VM | X2                               # m within 2^31 of 2^63: an accumulator near +-m reaches the wraps


def test_reachable_events_are_as_written_out():
    for eb in (8, 4):
        for m in CM.SMALL_MODULI + CM.BIG_MODULI:
            for acc in (False, True):
                assert set(CM.EVENT_NAMES) - CM.reachable(eb, m, acc, 9) == _unreachable(eb, m, acc), (eb, m, acc)
            one_row = set(CM.EVENT_NAMES) - CM.reachable(eb, m, False, 1)
            extra = (set() if m == 1 else X2) | ({"W+wrap", "W-wrap"} if eb == 8 else set())
            assert one_row == _unreachable(eb, m, False) | extra, (eb, m)
            assert CM.reachable(eb, m, True, 1) == CM.reachable(eb, m, True, 9)


def test_every_case_hits_each_reachable_event_and_the_model_agrees_with_the_oracle(oracle):
    """Per case and row count: the emitted events are exactly the reachable ones; each is real (the Python-integer
    model's running value in front of the event row and the row's value satisfy it); every value fits the element
    type; and the model's result is oracle.combine's (the initial accumulator as a row in front: (0 + r) % m == r)."""
    checked = 0
    for c in CM.EXACT_CASES:
        tmin, tmax = CM.limits(c.inst.elem_bytes)
        for n in c.ns:
            inp = c.inputs(n)
            assert inp.rows.shape == (n, c.shape.dim)
            if n:
                assert tmin <= inp.rows.min() and inp.rows.max() <= tmax
            if inp.acc0 is not None:
                assert np.abs(inp.acc0.astype(object)).max() < c.m
            if not c.flag_mode and n:
                assert {h[2] for h in inp.hits} == CM.reachable(c.inst.elem_bytes, c.m, c.acc, n), (c.id, n)
            evs = {e[0]: e for e in CM.events(c.m, c.inst.elem_bytes)}
            model = []
            hit_at = {col: (row, name) for col, row, name in inp.hits}
            for col in range(c.shape.dim):
                traj = CM.model_column(c.m, inp.rows[:, col], 0 if inp.acc0 is None else int(inp.acc0[col]))
                model.append(traj[-1])
                if col in hit_at:
                    row, name = hit_at[col]
                    assert CM.holds(*evs[name], traj[row], int(inp.rows[row, col]), c.m), (c.id, n, col, name)
            full = inp.rows if inp.acc0 is None else np.vstack([inp.acc0[None, :], inp.rows])
            exp = oracle.combine(c.m, full) if full.shape[0] else np.zeros(c.shape.dim, np.int64)
            assert model == exp.tolist(), (c.id, n)
            checked += 1
    assert checked >= 34 * 9


def test_flag_modes_give_their_flags():
    for c in CM.EXACT_CASES:
        if c.flag_mode:
            inp = c.inputs(c.ns[0])
            assert CM.expected_flags(c.m, inp.rows) == [int(c.flag_mode[0]), int(c.flag_mode[1])], c.id
    m = CM.P
    lim = 2**63 - m
    edge = np.array([[lim, -lim]], np.int64)
    assert CM.expected_flags(m, edge) == [1, 0] and CM.expected_flags(m, edge + np.array([[1, 0]])) == [1, 1]


def test_replay_model_agrees_with_the_oracle(oracle):
    """The replay model against the reference recurrence: started from the canonical state (a row in front), the
    oracle's result is the final state up to its sign, and it is negative exactly when the last sign event was a
    set (the initial codes, 0..6, are below the reset code 7 used here)."""
    for c in CM.REPLAY_CASES:
        for n in c.ns:
            rows, state0, code0 = CM.replay_inputs(c.m, n, c.shape.dim, n)
            lim = 2**63 - c.m
            assert n == 0 or (rows.min() >= -lim and rows.max() <= lim)
            st, cd = CM.model_replay(c.m, rows, state0, code0, 7)
            ref = oracle.combine(c.m, np.vstack([state0[None, :], rows])).tolist()
            assert [r % c.m for r in ref] == st, (c.id, n)
            assert [r < 0 for r in ref] == [k == 8 for k in cd], (c.id, n)
            assert all(k in (7, 8) or k == int(k0) for k, k0 in zip(cd, code0))


def test_grid_invariants():
    rng = np.random.default_rng(7)
    for per_cu in range(1, 9):
        for cus in (1, 8, 60, 104, 228, 256, 304):
            slots = cus * per_cu
            fill = max(64 * slots, per_cu * 256 * 64)
            edges = [fill - 1, fill, fill + 1, 248 * slots, 256 * slots - 9, 256 * slots, 256 * slots + 1,
                     3 * 256 * slots, 3 * 256 * slots + 1]
            for n_lanes in edges + rng.integers(1, 5 * 256 * slots, size=200).tolist():
                g = CB.grid(per_cu, cus, n_lanes)
                if n_lanes < fill:
                    assert g is None, (per_cu, cus, n_lanes)
                    continue
                assert g is not None, (per_cu, cus, n_lanes)
                G, wlo, nwide = g
                assert wlo % 8 == 0 and 8 <= wlo <= 248
                assert nwide <= G and G % slots == 0
                assert n_lanes <= CB.lanes_covered(G, wlo, nwide) < n_lanes + 8
                assert CB.lane_start(G - 1, wlo, nwide) < n_lanes       # the last workgroup holds a live lane
    slots = 256 * 8
    lanes = CM.balanced_lanes(slots, 8)
    small_part = CM.balanced_lanes(104 * 8, 8)   # fewer than 256 CUs: combine_grid's early exit is the threshold
    assert CB.grid(8, 104, small_part["below"]) is None
    assert all(CB.grid(8, 104, small_part[g]) is not None for g in CM.GEOMETRIES if g != "below")
    assert CB.grid(8, 256, lanes["below"]) is None
    assert CB.grid(8, 256, lanes["fill"]) == (slots, 64, 0)
    assert CB.grid(8, 256, lanes["one_wide"]) == (slots, 64, 1)
    assert CB.grid(8, 256, lanes["all_248"]) == (slots, 248, 0)
    assert CB.grid(8, 256, lanes["mixed"]) == (slots, 248, slots - 1)
    assert CB.grid(8, 256, lanes["all_256"]) == (slots, 248, slots)
    assert CB.grid(8, 256, lanes["second_round"]) == (2 * slots, 128, 1)


def test_balanced_plan_coverage():
    plan = CM.balanced_plan()
    per_inst, per_family, big_moduli, padded = {}, {}, set(), {}
    for (inst, small, acc, flag), geo, m, pad in plan:
        per_inst.setdefault((inst.tag, small, acc, flag), set()).add(geo)
        fam = CM.family(inst, flag)
        per_family.setdefault(fam, set()).add(geo)
        assert CB.small_m(m) == small
        if not small and fam != "int32":
            big_moduli.add(m)
        if pad:
            assert geo != "below"                # row stride > dim on the balanced grid, not on the plain one
            padded.setdefault(fam, set()).add(small)
    assert len(per_inst) == 10 and all("mixed" in g and len(g) >= 2 for g in per_inst.values())
    assert all(g == set(CM.GEOMETRIES) for g in per_family.values()) and len(per_family) == 3
    assert big_moduli == set(CM.BIG_MODULI)
    assert set(padded) == set(per_family) and all(v == {True, False} for v in padded.values())
