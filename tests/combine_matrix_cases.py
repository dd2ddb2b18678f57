"""The plan of tests/test_gpu_combine_matrix.py as data: every combine_exact_kernel / combine_replay_kernel
instantiation of sda_amd/csrc/combine.hip with the entry point, shape, alignment and knobs that reach it through the
public ABI, and the inputs each case runs on.  No GPU, no product import.

tests/test_combine_matrix_plan.py holds the plan against the instantiations in the built library, the steering
model against the oracle and every case against the events it must hit; tests/test_gpu_combine_matrix.py runs it.

Inputs are steered: a model of the recurrence in Python integers (wrapping i64 add, truncated `%`) knows the running
value r of every column, and column c carries event EVENTS[c mod E] at row (c div E) mod n -- the value v that puts
r + v or v itself on an edge of add_trem (modarith.h): its compare-and-adjust (`x >= m`, `x <= -m`), its selector
(v in (-m, m) takes the fast path) and the i64 wrap of r + v.  Random inputs meet these with probability about 1/m.
"""
import functools
from dataclasses import dataclass

import numpy as np

from tests import combine_dispatch as CB

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
I32_MIN, I32_MAX = -(2**31), 2**31 - 1
P = 2147482801
SMALL_MODULI = (1, 2, 433, P, 2**31 - 1, 2**40 + 7, 2**62)       # SMALL_M = true; 2^62 is the last such modulus
BIG_MODULI = (2**62 + 1, 2**63 - 25, 2**63 - 1)                  # SMALL_M = false
LANES = 259                                   # two workgroups, the second with 3 lanes: D = vec * LANES
GUARD = 64                                    # guard words before and after `out` (keeps its 32-byte alignment)
POISON = 0x5A5A5A5A5A5A5A5A
POISON32 = 0x5A5A5A5A


def limits(elem_bytes):
    return (I64_MIN, I64_MAX) if elem_bytes == 8 else (I32_MIN, I32_MAX)


# ---------------------------------------------------------------- the reference model, in Python integers
def wrap64(x):
    return (x + 2**63) % 2**64 - 2**63


def trem(x, m):
    """Rust's i64 `%`: the remainder has the dividend's sign."""
    return -((-x) % m) if x < 0 else x % m


def step(r, v, m):
    """combiner.rs:22-25: result[ix] += value (wrapping); result[ix] %= m."""
    return trem(wrap64(r + v), m)


def model_column(m, values, r0=0):
    """The running value before every row, and the result: [r_0, ..., r_n]."""
    out = [int(r0)]
    for v in values:
        out.append(step(out[-1], int(v), m))
    return out


def model_combine(m, rows, acc0=None):
    n, dim = rows.shape
    return [model_column(m, rows[:, c], 0 if acc0 is None else acc0[c])[-1] for c in range(dim)]


def _np_step(r, v, m):
    x = (r.astype(np.uint64) + v.astype(np.uint64)).astype(np.int64)
    return np.fmod(x, np.int64(m))


# ---------------------------------------------------------------- events
# name -> (kind, target): "sum" r + v == target, "val" v == target, "far" v == +-(m + 1) from r == +-(m - 1)
def events(m, elem_bytes):
    tmin, tmax = limits(elem_bytes)
    return (
        ("S+m", "sum", m), ("S-m", "sum", -m), ("S+m1", "sum", m - 1), ("S-m1", "sum", -(m - 1)), ("S0", "sum", 0),
        ("V+m", "val", m), ("V-m", "val", -m), ("V+m1", "val", m - 1), ("V-m1", "val", -(m - 1)), ("V0", "val", 0),
        # the last sum that fits i64 and the first that wraps, on each side
        ("W+max", "sum", I64_MAX), ("W+wrap", "sum", I64_MAX + 1), ("W-min", "sum", I64_MIN),
        ("W-wrap", "sum", I64_MIN - 1),
        ("Tmin", "val", tmin), ("Tmax", "val", tmax),
        # add_trem's selector is one value tighter than its adjust needs (v == +-m would still come out right on the
        # fast path): the first value that must stay outside is +-(m + 1), wrong there exactly when r == +-(m - 1)
        ("X+", "far", m + 1), ("X-", "far", -(m + 1)),
    )


EVENT_NAMES = tuple(e[0] for e in events(P, 8))
E = len(EVENT_NAMES)


def holds(name, kind, target, r, v, m):
    """Did the step from r with input v realise the event?  (Python integers)"""
    if kind == "sum":
        return r + v == target
    if kind == "val":
        return v == target
    return v == target and r == (m - 1 if target > 0 else -(m - 1))


def settable_r(elem_bytes, m, acc, n):
    """[lo, hi]: the running values a case can put in front of an event row.  An accumulate case chooses the
    column's initial accumulator (any |r| < m); a plain case with a row before the event reaches in one step, from
    0, any |r| < m that fits the element type; a single plain row always starts from 0."""
    tmin, tmax = limits(elem_bytes)
    if acc:
        return -(m - 1), m - 1
    if n >= 2:
        return max(-(m - 1), tmin), min(m - 1, tmax)
    return 0, 0


def reachable(elem_bytes, m, acc, n):
    """The events a case of n rows can hit, by interval arithmetic: a sum event needs an r in settable_r with
    target - r inside the element type; a value event needs the value inside it."""
    tmin, tmax = limits(elem_bytes)
    lo, hi = settable_r(elem_bytes, m, acc, n)
    out = set()
    for name, kind, t in events(m, elem_bytes):
        if kind == "val":
            ok = tmin <= t <= tmax
        elif kind == "sum":
            ok = max(lo, t - tmax) <= min(hi, t - tmin)
        else:
            r = m - 1 if t > 0 else -(m - 1)
            ok = tmin <= t <= tmax and lo <= r <= hi
        if ok:
            out.add(name)
    return frozenset(out)


def _want(kind, t, r, m):
    if kind == "sum":
        return t - r
    if kind == "val":
        return t
    return t if r == (m - 1 if t > 0 else -(m - 1)) else None


def _rstar(kind, t, m, lo, hi, tmin, tmax):
    if kind == "far":
        r = m - 1 if t > 0 else -(m - 1)
        return r if lo <= r <= hi else None
    r = t - tmax if t >= 0 else t - tmin          # the end of [t - tmax, t - tmin] nearer 0 ...
    return min(max(r, lo), hi)                    # ... moved into the settable range


@dataclass
class Inputs:
    rows: np.ndarray            # int64 [n][dim], every value inside the element type
    acc0: np.ndarray            # int64 [dim] initial accumulator, or None
    hits: tuple                 # (column, row, event name) of every event emitted


@functools.lru_cache(maxsize=64)
def steered(elem_bytes, m, n, dim, acc, seed):
    """The steered rows of a case (module docstring).  Other rows are random in (-m, m), clipped to the element
    type; initial accumulators are random in (-m, m) with m - 1, -(m - 1) and 0 planted.  Where the running value
    does not let an event's v fit the element type, the column's accumulator is chosen (and its earlier rows are 0),
    or the row before sets r in one step (from 0 when the running value is out of reach); an event that still does
    not fit is skipped for that column."""
    tmin, tmax = limits(elem_bytes)
    rng = np.random.default_rng(seed)
    rows = rng.integers(max(-(m - 1), tmin), min(m - 1, tmax), size=(n, dim), dtype=np.int64, endpoint=True)
    acc0 = None
    if acc:
        acc0 = rng.integers(-(m - 1), m - 1, size=dim, dtype=np.int64, endpoint=True)
        acc0[0::7], acc0[1::7], acc0[2::7] = m - 1, -(m - 1), 0
    hits = []
    if n == 0:
        return Inputs(rows, acc0, ())
    before = np.empty((n, dim), np.int64)         # the running value in front of each row, on the random rows
    r = np.zeros(dim, np.int64) if acc0 is None else acc0.copy()
    for i in range(n):
        before[i] = r
        r = _np_step(r, rows[i], m)
    lo, hi = settable_r(elem_bytes, m, acc, n)
    evs = events(m, elem_bytes)
    fits = lambda x: x is not None and tmin <= x <= tmax
    for c in range(dim):
        name, kind, t = evs[c % E]
        i = (c // E) % n
        v = _want(kind, t, int(before[i, c]), m)
        if not fits(v):
            rs = _rstar(kind, t, m, lo, hi, tmin, tmax)
            v = None if rs is None else _want(kind, t, rs, m)
            if not fits(v):
                continue
            if acc:
                acc0[c] = rs
                rows[:i, c] = 0
            elif i >= 1:
                vp = rs - int(before[i - 1, c])
                if not fits(vp):                  # out of reach in one step from here: from 0
                    rows[:i - 1, c] = 0
                    vp = rs
                rows[i - 1, c] = vp
            else:
                continue
        rows[i, c] = v
        hits.append((c, i, name))
    return Inputs(rows, acc0, tuple(hits))


FLAG_MODES = ("00", "10", "01", "11")            # (negative seen, out of range seen)


@functools.lru_cache(maxsize=16)
def flag_rows(m, n, dim, mode, seed):
    """Split inputs that raise exactly the flags of `mode`: non-negative values inside the no-wrap range
    [-(2^63 - m), 2^63 - m], plus one -1 (negative, in range), one 2^63 - m + 1 (out of range, not negative: m >= 2)
    or one -2^63 (both)."""
    lim = 2**63 - m
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, min(m - 1, lim), size=(n, dim), dtype=np.int64, endpoint=True)
    at = (n // 2, dim // 3)
    if mode == "10":
        rows[at] = -1
    elif mode == "01":
        assert m >= 2
        rows[at] = lim + 1
    elif mode == "11":
        rows[at] = I64_MIN
    acc0 = rng.integers(-(m - 1), m - 1, size=dim, dtype=np.int64, endpoint=True)
    return Inputs(rows, acc0, ())


def expected_flags(m, rows):
    """[an input < 0, an input outside [-(2^63 - m), 2^63 - m]] from the inputs, in Python integers."""
    lim = 2**63 - m
    assert 1 <= lim <= I64_MAX                    # so +-lim are i64 values
    return [int((rows < 0).any()), int(((rows > lim) | (rows < -lim)).any())]


# ---------------------------------------------------------------- the replay kernel's model and inputs
def model_replay(m, rows, state0, code0, reset_code):
    """combine_replay_kernel's step (combine.hip), per column: c' = (c + v) mod m canonical; the code becomes
    reset_code when c' == 0 or c + v >= m, reset_code + 1 when c + v < 0, else stays."""
    n, dim = rows.shape
    st, cd = [], []
    for c in range(dim):
        s, k = int(state0[c]), int(code0[c])
        for i in range(n):
            t = s + int(rows[i, c])
            s2 = t % m
            if s2 == 0 or t >= m:
                k = reset_code
            elif t < 0:
                k = reset_code + 1
            s = s2
        st.append(s)
        cd.append(k)
    return st, cd


@functools.lru_cache(maxsize=16)
def replay_inputs(m, n, dim, seed):
    """Rows inside the no-wrap range [-(2^63 - m), 2^63 - m] (pass 1 refuses others), a canonical state in [0, m)
    and earlier codes; column c steers c + v onto m, m - 1, 0, -1, -m, 2m - 1 or v onto +-m, +-(m - 1), 0, +-lim
    at row (c div 13) mod n where that v is in range."""
    lim = 2**63 - m
    rng = np.random.default_rng(seed)
    b = min(m - 1, lim)
    rows = rng.integers(-b, b, size=(n, dim), dtype=np.int64, endpoint=True)
    state0 = rng.integers(0, m - 1, size=dim, dtype=np.int64, endpoint=True)
    state0[0::5], state0[1::5] = 0, m - 1
    code0 = rng.integers(0, 6, size=dim, dtype=np.int64, endpoint=True).astype(np.int32)
    for c in range(dim if n else 0):
        k, i = c % 13, (c // 13) % n
        s = model_column_canon(m, rows[:i, c], int(state0[c]))
        v = (m - s, m - 1 - s, -s, -1 - s, -m - s, 2 * m - 1 - s, m, -m, m - 1, -(m - 1), 0, lim, -lim)[k]
        if abs(v) <= lim:
            rows[i, c] = v
    return rows, state0, code0


def model_column_canon(m, values, s):
    for v in values:
        s = (s + int(v)) % m
    return s


# ---------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Shape:
    tag: str
    dim: int
    pad: int = 0                # row stride = dim + pad, the padding poisoned
    in_off: int = 0             # elements between the (256-byte aligned) buffer and the rows
    out_off: int = 0            # i64 words between the (32-byte aligned) guard and `out`
    code_off: int = 0           # replay: int32 elements in front of `code`
    env: tuple = ()

    @property
    def stride(self):
        return self.dim + self.pad


@dataclass(frozen=True)
class Inst:
    """One combine_exact_kernel instantiation family: <T, vec, rows, *, *, *, pipe>."""
    elem_bytes: int
    vec: int
    rows: int
    pipe: bool
    shapes: tuple               # the first one runs every row count

    @property
    def tag(self):
        return f"{'long' if self.elem_bytes == 8 else 'int'}_{self.vec}_{self.rows}{'_pipe' if self.pipe else ''}"


PIPE0 = (("SDA_COMBINE_PIPE", "0"),)
INSTS = (
    Inst(8, 2, 4, True, (Shape("aligned", 2 * LANES), Shape("padded", 2 * LANES, pad=2))),
    Inst(8, 2, 8, False, (Shape("pipe0", 2 * LANES, env=PIPE0), Shape("pipe0_padded", 2 * LANES, pad=4, env=PIPE0))),
    Inst(8, 1, 8, False, (Shape("odd_dim", LANES), Shape("odd_stride", 2 * LANES, pad=1),
                          Shape("in_8mod16", 2 * LANES, in_off=1), Shape("out_8mod16", 2 * LANES, out_off=1))),
    Inst(4, 4, CB.WIDE32_ROWS, True, (Shape("aligned", 4 * LANES), Shape("padded", 4 * LANES, pad=4))),
    Inst(4, 4, 8, False, (Shape("pipe0", 4 * LANES, env=PIPE0), Shape("pipe0_padded", 4 * LANES, pad=8, env=PIPE0))),
    Inst(4, 2, 8, False, (Shape("dim_2mod4", 2 * LANES), Shape("stride_2mod4", 4 * LANES, pad=2),
                          Shape("in_8mod16", 4 * LANES, in_off=2), Shape("out_16mod32", 4 * LANES, out_off=2),
                          Shape("vec2_knob", 4 * LANES, env=(("SDA_COMBINE32_VEC", "2"),)))),
    Inst(4, 1, 8, False, (Shape("odd_dim", LANES), Shape("in_4mod8", 2 * LANES, in_off=1),
                          Shape("out_8mod16", 2 * LANES, out_off=1))),
)
REPLAY_SHAPES = {
    2: (Shape("aligned", 2 * LANES), Shape("padded", 2 * LANES, pad=2)),
    1: (Shape("odd_dim", LANES), Shape("code_4mod8", 2 * LANES, code_off=1), Shape("in_8mod16", 2 * LANES, in_off=1),
        Shape("odd_stride", 2 * LANES, pad=1)),
}


def row_counts(u):
    """No whole batch; one, two, three and four batches (the pipeline's peeled last batch on both buffers); tails
    of 0, 1 and U - 1 rows."""
    return tuple(sorted({1, u - 1, u, u + 1, 2 * u, 2 * u + 1, 3 * u, 4 * u - 1, 4 * u + 1}))


@dataclass(frozen=True)
class Case:
    """One instantiation at one shape and modulus, over its row counts (0: the plain call gives zeros, the
    accumulating ones leave `inout` and the record)."""
    inst: Inst
    shape: Shape
    m: int
    acc: bool
    flag: bool
    ns: tuple
    flag_mode: str = ""         # "": steered inputs; else flag_rows' mode, "+1" appended: the flag words start at 1

    @property
    def small(self):
        return CB.small_m(self.m)

    @property
    def entry(self):
        if self.inst.elem_bytes == 4:
            return "combine32_accumulate_dev" if self.acc else "combine32_dev"
        return "combine_split_dev" if self.flag else ("combine_accumulate_dev" if self.acc else "combine_dev")

    @property
    def kernel(self):
        i = self.inst
        return CB.exact_name(i.elem_bytes, i.vec, i.rows, self.small, self.acc, self.flag, i.pipe)

    @property
    def id(self):
        v = "split" if self.flag else ("acc" if self.acc else "plain")
        mode = f"-flags{self.flag_mode}" if self.flag_mode else ""
        return f"{self.inst.tag}-{v}-{self.shape.tag}-m{self.m}{mode}"

    def env(self):
        return dict(self.shape.env)

    def seed(self, n):
        return (self.m * 31 + self.shape.dim * 7 + n) % (2**32) + (1 if self.acc else 0)

    def inputs(self, n):
        if self.flag_mode:
            return flag_rows(self.m, n, self.shape.dim, self.flag_mode[:2], self.seed(n))
        return steered(self.inst.elem_bytes, self.m, n, self.shape.dim, self.acc, self.seed(n))

    def in_addr(self, base=0):
        return base + self.shape.in_off * self.inst.elem_bytes

    def out_addr(self, base=0):
        return base + (GUARD + self.shape.out_off) * 8

    def predicted(self, n, in_base=0, out_base=0):
        s = self.shape
        return CB.predict(self.inst.elem_bytes, s.dim, CB.launched_stride(n, s.dim, s.stride), self.in_addr(in_base),
                          self.out_addr(out_base), self.m, self.acc, self.flag, self.env())


def _moduli(small, k):
    """first and last modulus of the class and its main one, plus (SMALL_M) one of the four others by turns"""
    if not small:
        return (BIG_MODULI[1], BIG_MODULI[0], BIG_MODULI[2])
    others = (2, 433, 2**31 - 1, 2**40 + 7)
    return (P, 1, 2**62, others[k % 4])


def _exact_cases():
    out, k = [], 0
    for inst in INSTS:
        variants = [(False, False), (True, False)] + ([(True, True)] if inst.elem_bytes == 8 else [])
        for acc, flag in variants:
            for small in (True, False):
                main, *rest = _moduli(small, k)
                k += small
                u = inst.rows
                out.append(Case(inst, inst.shapes[0], main, acc, flag, (0,) + row_counts(u)))
                for m in rest:
                    out.append(Case(inst, inst.shapes[0], m, acc, flag, (u + 1, 4 * u + 1)))
                for shape in inst.shapes[1:]:
                    out.append(Case(inst, shape, main, acc, flag, (2 * u + 1,)))
                if flag:
                    for mode in FLAG_MODES:
                        out.append(Case(inst, inst.shapes[0], main, acc, flag, (2 * u + 1,), mode))
                    out.append(Case(inst, inst.shapes[0], main, acc, flag, (2 * u + 1,), "00+1"))
    return tuple(out)


EXACT_CASES = _exact_cases()


@dataclass(frozen=True)
class ReplayCase:
    vec: int
    shape: Shape
    m: int
    ns: tuple

    @property
    def kernel(self):
        return CB.replay_name(self.vec, CB.small_m(self.m))

    @property
    def id(self):
        return f"replay_{self.vec}-{self.shape.tag}-m{self.m}"

    def env(self):
        return {}

    def predicted(self, n, in_base=0, state_base=0, code_base=0):
        s = self.shape
        return CB.predict_replay(s.dim, CB.launched_stride(n, s.dim, s.stride), in_base + s.in_off * 8,
                                 state_base + GUARD * 8, code_base + (GUARD + s.code_off) * 4, self.m)


def _replay_cases():
    out = []
    for vec, shapes in REPLAY_SHAPES.items():
        for small in (True, False):
            # the main modulus, then the first and last of the class (m = 1: the state is 0 and every step a reset)
            main, *rest = (P, 1, 2**62, 2) if small else (2**63 - 25, 2**62 + 1, 2**63 - 1)
            out.append(ReplayCase(vec, shapes[0], main, (0,) + row_counts(8)))
            for m in rest:
                out.append(ReplayCase(vec, shapes[0], m, (9, 33)))
            for shape in shapes[1:]:
                out.append(ReplayCase(vec, shape, main, (17,)))
    return tuple(out)


REPLAY_CASES = _replay_cases()


# ---------------------------------------------------------------- the balanced grid
BALANCED_ROWS = {8: 9, 4: 5}                   # two whole batches and a tail of the pipelined kernels (4 and 2 rows)
PIPELINED = tuple((inst, small, acc, flag)
                  for inst in INSTS if inst.pipe
                  for acc, flag in ([(False, False), (True, False)] + ([(True, True)] if inst.elem_bytes == 8 else []))
                  for small in (True, False))
GEOMETRIES = ("below", "fill", "one_wide", "all_248", "mixed", "all_256", "second_round")


def balanced_lanes(slots, per_cu):
    """geometry -> lane count, from slots = CUs * per_cu (tests/test_gpu_combine_matrix.py reads per_cu from the
    record and the CU count from the device).  The balanced grid starts at 64 lanes per slot -- of a part of at least
    256 CUs: combine_grid leaves earlier, before it asks for the CU count, below 64 * 256 * per_cu lanes, so on a
    smaller part the fill threshold is that (and "fill" is then wider than 64 lanes per workgroup)."""
    fill = max(64 * slots, 64 * 256 * per_cu)
    return {"below": fill - 1,                 # plain grid
            "fill": fill,                      # balanced, wlo = 64 (256 CUs and more), no wide workgroup
            "one_wide": fill + 1,              # one wide workgroup holding one live lane
            "all_248": 248 * slots,            # every workgroup 248 wide
            "mixed": 256 * slots - 9,          # widths 248 / 256, the last wide workgroup partly filled
            "all_256": 256 * slots,            # every workgroup 256 wide
            "second_round": 256 * slots + 1}


def family(inst, flag):
    return "int32" if inst.elem_bytes == 4 else ("i64_flag" if flag else "i64")


def balanced_plan():
    """(instantiation, geometry, modulus, padded) of every balanced-grid run: every instantiation runs "mixed" and
    its share of the other geometries dealt round its family, so each geometry runs in each family; the
    SMALL_M = false instantiations between them run every such modulus; two runs per family have row stride > dim,
    both on the balanced grid: "mixed" at a SMALL_M modulus and "fill" at a larger one."""
    plan = []
    fams = {}
    for p in PIPELINED:
        fams.setdefault(family(p[0], p[3]), []).append(p)
    for fam, members in fams.items():
        others = [g for g in GEOMETRIES if g != "mixed"]
        big = 0
        for j, p in enumerate(members):
            geos = ["mixed"] + [g for i, g in enumerate(others) if i % len(members) == j]
            for gi, geo in enumerate(geos):
                if p[1]:
                    m = P
                else:
                    m = BIG_MODULI[big % 3]
                    big += 1
                plan.append((p, geo, m, (geo == "mixed" and j == 0) or geo == "fill"))
    return tuple(plan)


def boundary_lanes(n_lanes, geom):
    """Lanes on both sides of every kind of workgroup boundary: wide|wide, wide|narrow at g = nwide,
    narrow|narrow, and the last workgroup's first and last lanes (plain grid: the 256-lane boundaries)."""
    lanes = set()
    if geom is None:
        G = CB.plain_grid(n_lanes)
        starts = [256 * g for g in (1, G // 2, G - 1) if 0 < g < G]
    else:
        G, wlo, nwide = geom
        gs = {1, nwide - 1, nwide, nwide + 1, G - 1}
        starts = [CB.lane_start(g, wlo, nwide) for g in gs if 0 < g < G]
    for s in starts:
        lanes.update((s - 2, s - 1, s, s + 1))
    lanes.update((0, 1, n_lanes - 2, n_lanes - 1))
    return sorted(x for x in lanes if 0 <= x < n_lanes)
