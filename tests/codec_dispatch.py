"""The share payload codec's dispatch, restated once for the tests (CPU only, numpy; no product import).

Everything here is computed from a job's payload bytes and blob offsets alone -- the same inputs
`decode_combine()` (sda_amd/csrc/engine_codec.cpp) and the launchers of sda_amd/csrc/codec_decode.hip decide from:

  regions        16 KiB regions aligned to the byte buffer (kRegionBytes; varint_plan);
  terminators    bytes without 0x80 inside a blob, and a blob's last byte when it continues (a truncated tail
                 counts as one element: make_window_cm's lastbit);
  wide           what raises the slot decode's wide flag: an element longer than 5 bytes, a 5-byte element whose
                 zigzag value is >= 2^32 (its fifth group above 15), or a region with more than kSlotCap = 4096
                 terminators (varint_decode_kernel<int32_t, SPARSE>);
  irregular      a run of >= 11 continuation bytes inside a blob (varint_count_kernel's r11: the sequential decoder);
  long           a run of >= 5 continuation bytes inside a blob (r5): an element of >= 6 bytes -- or a truncated
                 tail of five continuation bytes, which the count pass cannot tell apart;
  slot_c0        the c0 of slot_plan_kernel's entry for every (tile, blob);
  predict        the (path, width, fell_back, passes) record sda_codec_last_launch must report for a job and the
                 knobs it ran under, and the kernels that produced it, spelled as scripts/code_objects.py
                 demangles them.
"""
import numpy as np

REGION = 16384            # codec_decode.hip: kRegionBytes
SUB_REGION = 4096         # codec_decode.hip: kSubBytes
SLOT_CAP = 4096           # codec_decode.hip: kSlotCap
GRID_Y = 65535            # the y0 slices of every per-blob grid
ENC_CHUNK = 2048          # codec_encode.hip: kEncChunk
THREADS = 256             # codec_common.h: kThreads

# sda_codec_last_launch (include/sda_engine.h)
NONE, SLOTS, SLOTS_GROUPED, FUSED, FUSED_MULTI, MATRIX32, MATRIX64 = range(7)
FB_SLOT_WIDE, FB_FUSED_IRREGULAR, FB_NARROW_WIDE, FB_SEQUENTIAL = 1, 2, 4, 8
PATH_NAMES = ["NONE", "SLOTS", "SLOTS_GROUPED", "FUSED", "FUSED_MULTI", "MATRIX32", "MATRIX64"]


def _b(x):
    return "true" if x else "false"


class Job:
    """A job's bytes (np.uint8, at least off[-1] of them) and offsets, with the facts the dispatcher derives."""

    def __init__(self, buf, off):
        self.off = np.asarray(off, dtype=np.int64)
        self.buf = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
        self.n = self.off.size - 1
        lo, hi = int(self.off[0]), int(self.off[-1])
        body = self.buf[lo:hi]
        self.cont = body >= 0x80                                   # continuation bytes, index = byte - lo
        term = ~self.cont
        ends = self.off[1:][self.off[1:] > self.off[:-1]] - 1 - lo  # last byte of every non-empty blob
        term[ends] = True
        self.term_pos = np.flatnonzero(term) + lo                  # absolute byte of every element's last byte
        # blobs are contiguous and each ends in a terminator: an element starts after the previous one's end
        self.start_pos = np.concatenate([[lo], self.term_pos[:-1] + 1]) if self.term_pos.size else self.term_pos
        self.length = self.term_pos - self.start_pos + 1
        self.blob_of = np.searchsorted(self.off, self.term_pos, side="right") - 1
        self.counts = np.bincount(self.blob_of, minlength=self.n)[:self.n] if self.n else np.zeros(0, np.int64)

    # ---- regions ----
    def blob_regions(self):
        """regions per blob (varint_plan): 0 for an empty blob"""
        s, e = self.off[:-1], self.off[1:]
        return np.where(e > s, (e - 1) // REGION - s // REGION + 1, 0)

    def region_counts(self):
        """{(blob, region index in the buffer): terminators}"""
        key = self.blob_of * (1 << 32) + self.term_pos // REGION
        k, c = np.unique(key, return_counts=True)
        return k >> 32, k & 0xFFFFFFFF, c

    # ---- flags ----
    def _runs(self, k):
        """per blob: a run of >= k continuation bytes inside it"""
        lo = int(self.off[0])
        idx = np.arange(self.cont.size)
        starts = self.off[:-1][self.off[:-1] < self.off[-1]] - lo
        first = np.zeros(self.cont.size, np.int64)                 # where the run a byte belongs to may begin:
        first[starts] = starts                                     # at its blob's first byte,
        first = np.maximum(first, np.where(self.cont, 0, idx + 1))  # or after the last byte that does not continue
        run = np.where(self.cont, idx - np.maximum.accumulate(first) + 1, 0)
        hit = np.flatnonzero(run >= k) + lo
        out = np.zeros(self.n, bool)
        out[np.searchsorted(self.off, hit, side="right") - 1] = True
        return out

    def irregular(self):
        return self._runs(11)

    def long(self):
        return self._runs(5)

    def fifth_group(self):
        """the fifth byte's 7-bit group of every 5-byte element (else 0)"""
        g = np.zeros(self.length.size, np.int64)
        five = self.length == 5
        g[five] = self.buf[self.term_pos[five]] & 0x7F
        return g

    def fits_int32(self):
        """every element has <= 5 bytes and a zigzag value below 2^32 (the int32 decodes' narrow_fail)"""
        return bool((self.length <= 5).all() and (self.fifth_group() <= 15).all())

    def max_region_count(self):
        _, _, c = self.region_counts()
        return int(c.max()) if c.size else 0

    def slot_wide(self):
        return not self.fits_int32() or self.max_region_count() > SLOT_CAP

    # ---- slot plan ----
    def slot_c0(self, tile):
        """[(blob, tile index, c0, elements of the tile)] as slot_plan_kernel computes c0: the elements of the
        tile that sit in the region holding its first element"""
        out = []
        blob, reg, cnt = self.region_counts()
        for b in range(self.n):
            sel = blob == b
            c = cnt[sel]                                            # np.unique sorted them by region
            base = np.concatenate([[0], np.cumsum(c)])
            dim = int(base[-1])
            for t in range((dim + tile - 1) // tile):
                r = int(np.searchsorted(base, t * tile, side="right") - 1)
                e1 = int(base[r + 1])
                out.append((b, t, min(e1 - t * tile, tile), min(dim - t * tile, tile)))
        return out


def slices(n_blobs):
    return (n_blobs + GRID_Y - 1) // GRID_Y


def dec_kernel(out32, sparse, knobs):
    """codec_decode.hip dec_kernel<OutT, SPARSE>(): SDA_DEC_NT = 0 / 1 forces the store kind, else nontemporal for the slots"""
    e = knobs.get("SDA_DEC_NT")
    nt = (e[0] == "1") if e and e[0] in "01" else sparse
    return f"varint_decode_kernel<{'int' if out32 else 'long'}, {_b(sparse)}, {_b(nt)}>"


def slot_cpl(knobs):
    v = knobs.get("SDA_SLOT_CPL")
    return int(v) if v in ("1", "2") else 4


def dc_depth(knobs):
    v = knobs.get("SDA_DC_DEPTH")
    return int(v) if v in ("2", "8") else 4


def write_kernel(knobs):
    e = knobs.get("SDA_ENC_NT")
    return f"varint_write_kernel<{_b(not (e and e[0] == '0'))}>"


def decode_dev_kernel(knobs):
    """sda_varint_decode_dev: the i64 decode"""
    return dec_kernel(False, False, knobs)


def predict(job, m, knobs):
    """((path, width, fell_back, passes), [kernels]) of sda_clerk_decode_combine_dev over `job` (blobs of equal
    element count, modulus m > 0) under the environment `knobs` -- decode_combine() line by line."""
    path = knobs.get("SDA_CODEC_PATH")
    narrow_ok = knobs.get("SDA_CODEC_NARROW") != "0"
    force_fused = path == "fused"
    n = job.n
    small_m = abs(m) <= 1 << 62
    kernels, fb = [], 0
    if n == 0:
        return (NONE, 0, 0, 0), kernels
    if narrow_ok and not force_fused and path != "matrix":
        kernels.append(dec_kernel(True, True, knobs))
        if not job.slot_wide():
            G = min(int(knobs.get("SDA_CODEC_GROUP", "0")), GRID_Y)
            grouped = G != 0 and G < n
            cpl = slot_cpl(knobs)
            if int(job.counts[0]):
                kernels.append(f"slot_combine_kernel<{cpl}, 8, {_b(small_m)}>")
            passes = (n + G - 1) // G if grouped else (slices(n) if int(job.blob_regions().sum()) else 0)
            return (SLOTS_GROUPED if grouped else SLOTS, cpl, 0, passes), kernels
        fb |= FB_SLOT_WIDE
    if int(job.counts[0]) == 0:
        return (NONE, 0, 0, 0), kernels
    irregular = bool(job.irregular().any())
    if force_fused:
        if not irregular:
            multi = bool(job.long().any())
            depth = 2 if multi else dc_depth(knobs)
            kernels.append(f"varint_decode_combine_kernel<{depth}, {_b(multi)}>")
            return (FUSED_MULTI if multi else FUSED, depth, fb, slices(n)), kernels
        fb |= FB_FUSED_IRREGULAR
    if narrow_ok and not irregular:
        kernels.append(dec_kernel(True, False, knobs))
        if job.fits_int32():
            return (MATRIX32, 0, fb, slices(n)), kernels
        fb |= FB_NARROW_WIDE
    kernels.append(dec_kernel(False, False, knobs))
    if irregular:
        fb |= FB_SEQUENTIAL
    return (MATRIX64, 0, fb, slices(n)), kernels


def predict_blobs(blobs, m, knobs):
    """predict()'s record for payloads packed back to back from offset 0"""
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])])
    return predict(Job(b"".join(blobs), off), m, knobs)[0]
