"""The snapshot transposition's host plan and copy kernel restated in Python integers and numpy, from the engine's
own code: sda_snapshot_transpose_dev (sda_amd/csrc/engine_codec.cpp) and sda_amd/csrc/snapshot.hip as shipped
(SDA_SNAP_UNALIGNED=1, SDA_SNAP_NT_LOAD=0, 8 quads per lane, 4 chunks per workgroup).  A later kernel variant
updates this file; the cases (tests/snapshot_matrix_cases.py) take the chunk size as an argument.

  plan              clerk_base, clerk_off, dst_len, the clerk-major list of non-empty (src, dst, len), chunk_start,
                    the grid and the sda_snapshot_last_launch record the call must report
  grid_for          launch_snapshot_transpose's grid, the cap branch included (arithmetic only)
  wg_range(s)       the chunk range of workgroup w, in the kernel's wrapping 64-bit arithmetic
  walk              the (blob, chunk in blob) pairs workgroup w copies: binary search, then the forward walk
  copy_chunk_model  copy_chunk: head lanes 0-15, tail lanes 64-79, body quads, every lane an explicit loop index
  transpose_model   the whole dst buffer after the kernel, bytes it must not write included

`fault` names one deliberate mistake in the index arithmetic (FAULTS); tests/test_snapshot_matrix_plan.py shows that
every one of them changes the dst buffer of some case of the matrix.  Unsigned 64-bit values wrap as in the kernel.
With a fault, an access outside the buffers is dropped (a read gives 0); without one it is an AssertionError: the
kernel as written reads only source bytes of its blobs and writes only destination bytes of its blobs.
"""
from collections import namedtuple

import numpy as np

THREADS = 256                      # kThreads
QUADS = 8                          # SDA_SNAP_QUADS: 16-byte quads per lane and chunk
CHUNK = THREADS * QUADS * 16       # kChunk: 32 KiB
CHUNKS_PER_WG = 4                  # SDA_SNAP_CHUNKS_PER_WG
GUARD = 256                        # bytes past dst_len the tests allocate and the model carries
M64 = (1 << 64) - 1
Q15 = M64 ^ 15

FAULTS = (
    "tail_drops_last_byte",        # 1  tail bound off by one: E + i < e - 1
    "body_guard_le",               # 2  body guard d <= d_hi: one quad past the body
    "head_le",                     # 3  head written for a + t <= A
    "body_shift_mod4",             # 4  the body's source shift taken mod 4 instead of mod 16
    "later_chunks_minus16",        # 5  chunk k >= 1 of a blob starts at k * C - 16
    "walk_stuck_on_one_chunk",     # 6  the walk does not advance off a blob of exactly one chunk
    "search_first_ge",             # 7  the binary search returns the first b with chunk_start[b] >= lo
    "tail_stale_blob",             # 8  after a switch the tail reads through the previous blob's shift
    "tail_lanes_16_31",            # 9  the tail on lanes 16-31 with the index expression of lanes 64-79
)

Plan = namedtuple("Plan", "P n chunk clerk_base clerk_off dst_len blobs chunk_start grid record")


def fill_pattern(size):
    """the fixed pattern dst holds before the call"""
    return ((np.arange(size, dtype=np.uint64) * 37 + 11) & 0xFF).astype(np.uint8)


def grid_for(total):
    """launch_snapshot_transpose: 4 chunks per workgroup, more once that would pass 2^31 - 1 workgroups, and no
    more workgroups than keep the kernel's total * (w + 1) inside 64 bits"""
    if not total:
        return 0
    cpw = CHUNKS_PER_WG if total // CHUNKS_PER_WG < 0x7FFFFFFF else total // 0x7FFFFFFF + 1
    return min((total + cpw - 1) // cpw, M64 // total)


def plan(part_off, P, n, chunk=CHUNK):
    """sda_snapshot_transpose_dev's host side for HOST offsets part_off[P * n + 1]"""
    off = [int(x) for x in part_off]
    assert len(off) == P * n + 1 and all(a <= b for a, b in zip(off, off[1:]))
    clerk_base, clerk_off, total = [], [], 0
    for c in range(n):
        clerk_base.append(total)
        row = [0]
        for p in range(P):
            row.append(row[-1] + off[p * n + c + 1] - off[p * n + c])
        clerk_off.append(row)
        total += ((row[P] + 15) & ~15) + 16          # the job 16-byte aligned and followed by 16 readable bytes
    blobs, chunk_start, shifts = [], [0], 0
    for c in range(n):
        for p in range(P):
            ln = off[p * n + c + 1] - off[p * n + c]
            if not ln:
                continue                             # empty blobs never reach the device
            src, dst = off[p * n + c], clerk_base[c] + clerk_off[c][p]
            blobs.append((src, dst, ln))
            chunk_start.append(chunk_start[-1] + (ln + chunk - 1) // chunk)
            shifts |= 1 << ((src - dst) & 15)
    grid = grid_for(chunk_start[-1]) if blobs else 0
    record = (len(blobs), chunk_start[-1], grid, chunk, shifts)
    return Plan(P, n, chunk, clerk_base, clerk_off, total, blobs, chunk_start, grid, record)


def wg_range(total, G, w):
    """the kernel's lo = total * w / G, hi = total * (w + 1) / G, the products in wrapping 64 bits"""
    return ((total * w) & M64) // G, ((total * (w + 1)) & M64) // G


def wg_ranges(total, G):
    return [wg_range(total, G, w) for w in range(G)]


def walk(pl, w, fault=None):
    """snapshot_transpose_kernel: the (blob, chunk in blob) pairs of workgroup w, in order"""
    cs, nb = pl.chunk_start, len(pl.blobs)
    lo, hi = wg_range(cs[-1], pl.grid, w)
    if lo >= hi:
        return []
    if fault == "search_first_ge":
        l, r = 0, nb - 1                             # first b with chunk_start[b] >= lo
        while l < r:
            mid = (l + r) // 2
            if cs[mid] >= lo:
                r = mid
            else:
                l = mid + 1
    else:
        l, r = 0, nb - 1                             # last b with chunk_start[b] <= lo
        while l < r:
            mid = (l + r + 1) // 2
            if cs[mid] <= lo:
                l = mid
            else:
                r = mid - 1
    b, nxt = l, cs[l + 1]
    out = []
    for ch in range(lo, hi):
        if ch >= nxt and not (fault == "walk_stuck_on_one_chunk" and cs[b + 1] - cs[b] == 1):
            b += 1
            nxt = cs[b + 1]
        out.append((b, (ch - cs[b]) & M64))
    return out


def chunk_geometry(blob, chunk, C=CHUNK, fault=None):
    """copy_chunk's (a, A, E, e): the chunk's dst bytes [a, e), its head [a, A), body quads [A, E), tail [E, e)"""
    _, d0, ln = blob
    c0 = (chunk * C) & M64
    if fault == "later_chunks_minus16" and chunk >= 1:
        c0 = (c0 - 16) & M64
    c1 = (c0 + C) & M64 if (c0 + C) & M64 < ln else ln
    a, e = (d0 + c0) & M64, (d0 + c1) & M64
    A, E = ((a + 15) & M64) & Q15, e & Q15
    if A > E:
        A = E = e                                    # the chunk lies inside one quad: all bytes are head bytes
    return a, A, E, e


def copy_chunk_model(src, dst, blob, chunk, fault=None, stale=None, C=CHUNK):
    """copy_chunk(src, dst, c, chunk) for one workgroup, lane by lane.  `stale`: the blob the walk held before its
    last switch (only the tail_stale_blob fault looks at it)."""
    strict = fault is None

    def load(i, k):
        if 0 <= i and i + k <= src.size:
            return src[i:i + k]
        assert not strict, f"reads src[{i}:{i + k}] of {src.size}"
        return np.zeros(k, np.uint8)

    def store(i, v):
        if 0 <= i and i + v.size <= dst.size:
            dst[i:i + v.size] = v
        else:
            assert not strict, f"writes dst[{i}:{i + v.size}] of {dst.size}"

    a, A, E, e = chunk_geometry(blob, chunk, C, fault)
    shift = blob[0] - blob[1]                        # int64 in the kernel; source byte = dst byte + shift
    tail_shift = stale[0] - stale[1] if fault == "tail_stale_blob" and stale is not None else shift
    for t in range(16):                              # head: lanes 0-15
        ok = a + t <= A if fault == "head_le" else a + t < A
        if ok:
            store(a + t, load((a + t + shift) & M64, 1))
    for t in (range(16, 32) if fault == "tail_lanes_16_31" else range(64, 80)):   # tail: lanes 64-79
        i = (t - 64) & 0xFFFFFFFF                    # uint32 t - 64
        pos = (E + i) & M64
        ok = pos + 1 < e if fault == "tail_drops_last_byte" else pos < e
        if ok:
            store(pos, load((pos + tail_shift) & M64, 1))
    if A >= E:
        return
    O = shift & 15                                   # the switch: copy_body<O>
    bshift = shift - O + (O & 3) if fault == "body_shift_mod4" else shift
    for it in range(QUADS):
        for t in range(THREADS):
            d = A + (it * THREADS + t) * 16
            if not (d <= E if fault == "body_guard_le" else d < E):
                return                               # d grows with (it, t): every later lane's guard fails too
            s = (d + bshift) & M64
            if O == 0:
                s &= Q15                             # the aligned load
            store(d, load(s, 16))


def transpose_model(src, part_off, P, n, fill=fill_pattern, fault=None, C=CHUNK):
    """dst[dst_len + GUARD] after sda_snapshot_transpose_dev on a buffer that held fill(size): every workgroup's
    walk in grid order (the workgroups of the kernel as written touch disjoint bytes, so their order is free)"""
    pl = plan(part_off, P, n, C)
    dst = fill(pl.dst_len + GUARD).copy()
    src = np.asarray(src, np.uint8)
    assert src.size >= int(part_off[P * n]) + 32
    src = src[:int(part_off[P * n]) + 32]            # what the header lets the kernel read
    for w in range(pl.grid):
        stale, prev = None, None
        for b, k in walk(pl, w, fault):
            if prev is not None and b != prev:
                stale = pl.blobs[prev]
            prev = b
            copy_chunk_model(src, dst, pl.blobs[b], k, fault, stale, C)
    return dst


def clerk_slices(buf, pl):
    """[clerk][participation] bytes of a dst buffer laid out by the plan"""
    raw = buf.tobytes()
    return [[raw[pl.clerk_base[c] + pl.clerk_off[c][p]:pl.clerk_base[c] + pl.clerk_off[c][p + 1]]
             for p in range(pl.P)] for c in range(pl.n)]


def blob_mask(pl, size):
    """True where dst belongs to a blob"""
    m = np.zeros(size, bool)
    for _, d, ln in pl.blobs:
        m[d:d + ln] = True
    return m
