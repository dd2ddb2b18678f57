"""The share-combine dispatch, restated once for the tests (CPU only; no product import).

`predict` / `predict_replay` return the sda_combine_last_launch record that `launch_combine_exact`,
`launch_combine_wide32`, `launch_combine_exact32`, `launch_combine_split` and `launch_combine_replay`
(sda_amd/csrc/combine.hip) must leave for a call -- without its grid fields -- and the pretty name of the kernel
instantiation, spelled as scripts/code_objects.py demangles it, so tests/test_combine_matrix_plan.py can hold the
plan of tests/test_gpu_combine_matrix.py against the instantiations in the built library.  `grid` restates
`combine_grid`, the balanced grid of the pipelined kernels.

Restated here, each next to the line of the product it mirrors:
  the widest-vector rules (columns, row stride and both base addresses line up), SDA_COMBINE_PIPE,
  SDA_COMBINE32_VEC (its two readings: sda_combine32_dev takes 4 columns unless it says 2, the codec's combine takes
  2 unless it says 4), SMALL_M = m <= 2^62, the replay kernel's extra alignment of `code`, and combine_grid.
"""
from collections import namedtuple

NONE, EXACT, REPLAY = 0, 1, 2              # sda_combine_last_launch: kind
SMALL_M, ACC, FLAG, PIPE = 1, 2, 4, 8      # ... variant bits
KNOBS = ("SDA_COMBINE_PIPE", "SDA_COMBINE_BALANCE", "SDA_COMBINE32_VEC")   # every knob the combine reads

WIDE32_ROWS = 2                            # combine.hip: kWide32Rows
WG = 256                                   # lanes per workgroup of the plain grid

# (kind, elem_bytes, vec, rows, variant) as sda_combine_last_launch reports them, and the kernel's pretty name
Launch = namedtuple("Launch", "kind elem_bytes vec rows variant kernel")


def _b(x):
    return "true" if x else "false"


def small_m(m):
    """combine.hip: small_m = modulus <= 2^62 (the kernels without add_trem's wrapping slow path)."""
    return m <= 1 << 62


def launched_stride(n, dim, row_stride):
    """engine_dev.cpp: every entry point hands the launcher `n > 1 ? row_stride : dim`."""
    return row_stride if n > 1 else dim


def _first_char_not_0(env, name):
    """combine_pipe() / combine_balance(): on unless the variable's first character is '0'."""
    v = env.get(name)
    return not (v and v[0] == "0")


def pipe_enabled(env):
    return _first_char_not_0(env, "SDA_COMBINE_PIPE")


def balance_enabled(env):
    return _first_char_not_0(env, "SDA_COMBINE_BALANCE")


def _atoi(s):
    s = (s or "").strip()
    digits = ""
    for i, ch in enumerate(s):
        if ch.isdigit() or (i == 0 and ch in "+-"):
            digits += ch
        else:
            break
    return int(digits) if digits.strip("+-") else 0


def exact_name(elem_bytes, vec, rows, small, acc, flag, pipe):
    return (f"combine_exact_kernel<{'long' if elem_bytes == 8 else 'int'}, {vec}, {rows}, {_b(small)}, {_b(acc)}, "
            f"{_b(flag)}, {_b(pipe)}>")


def replay_name(vec, small):
    return f"combine_replay_kernel<{vec}, 8, {_b(small)}>"


def _exact(elem_bytes, vec, rows, m, acc, flag, pipe):
    s = small_m(m)
    variant = (SMALL_M if s else 0) | (ACC if acc else 0) | (FLAG if flag else 0) | (PIPE if pipe else 0)
    return Launch(EXACT, elem_bytes, vec, rows, variant, exact_name(elem_bytes, vec, rows, s, acc, flag, pipe))


def predict(elem_bytes, dim, stride, in_addr, out_addr, m, acc, flag, env, codec=False):
    """The launch of one combine over `dim` columns (dim > 0) with the launcher's row stride (launched_stride)
    and the device addresses of the rows and of the output.  elem_bytes 8: launch_combine_exact /
    launch_combine_split (flag); 4: launch_combine_wide32 (sda_combine32_dev, the half-width host stream) or, with
    codec=True, launch_combine_exact32 (the decode -> combine's int32 matrix)."""
    assert dim > 0 and (not flag or acc)
    if elem_bytes == 8:
        # launch_combine_exact / launch_combine_split: v2 = dim % 2 == 0 && stride % 2 == 0 && (in | out) % 16 == 0
        v2 = dim % 2 == 0 and stride % 2 == 0 and (in_addr | out_addr) % 16 == 0
        if v2 and pipe_enabled(env):
            return _exact(8, 2, 4, m, acc, flag, True)
        return _exact(8, 2 if v2 else 1, 8, m, acc, flag, False)
    assert elem_bytes == 4 and not flag
    knob = _atoi(env.get("SDA_COMBINE32_VEC"))
    # combine32_wide_lanes: want4 unless the knob says 2; launch_combine_exact32: want4 only when it says 4
    want4 = knob == 4 if codec else knob != 2
    lines4 = dim % 4 == 0 and stride % 4 == 0 and in_addr % 16 == 0 and out_addr % 32 == 0
    if not codec and want4 and pipe_enabled(env) and lines4:
        return _exact(4, 4, WIDE32_ROWS, m, acc, False, True)
    # combine32_narrow_lanes
    if want4 and lines4:
        return _exact(4, 4, 8, m, acc, False, False)
    v2 = dim % 2 == 0 and stride % 2 == 0 and in_addr % 8 == 0 and out_addr % 16 == 0
    return _exact(4, 2 if v2 else 1, 8, m, acc, False, False)


def predict_replay(dim, stride, in_addr, state_addr, code_addr, m):
    """launch_combine_replay: 2 columns per lane also need `code` (int32) on an 8-byte boundary."""
    assert dim > 0
    v2 = dim % 2 == 0 and stride % 2 == 0 and (in_addr | state_addr) % 16 == 0 and code_addr % 8 == 0
    s = small_m(m)
    return Launch(REPLAY, 8, 2 if v2 else 1, 8, SMALL_M if s else 0, replay_name(2 if v2 else 1, s))


def plain_grid(n_lanes):
    return -(-n_lanes // WG)


def grid(per_cu, cus, n_lanes):
    """combine_grid: (G, wlo, nwide) of the balanced grid -- G whole rounds of cus * per_cu resident workgroups,
    every workgroup wlo lanes (a multiple of 8, at most 248) and the first nwide of them 8 more -- or None where
    the launcher keeps the plain grid: a job below 64 lanes per slot."""
    if per_cu <= 0 or n_lanes < per_cu * 256 * 64:          # below 64 lanes per slot of a 256-CU part: no query
        return None
    if cus <= 0:
        return None
    slots = cus * per_cu
    if n_lanes < slots * 64:
        return None
    rounds = -(-n_lanes // (slots * 256))
    g = slots * rounds
    lo = min(n_lanes // g // 8 * 8, 248)
    wide = (n_lanes - g * lo + 7) // 8
    if lo == 0 or wide > g or g > 0x7FFFFFFF:
        return None
    return g, lo, wide


def lane_start(g, wlo, nwide):
    """First lane of workgroup g on the balanced grid (combine_exact_kernel: g wlo + 8 min(g, nwide))."""
    return g * wlo + 8 * min(g, nwide)


def lanes_covered(G, wlo, nwide):
    return G * wlo + 8 * nwide
