"""A whole aggregation over the role-level job calls, one call per role (several where the plan tiles the clerk), and
the case matrix tests/test_job_aggregation_model.py and tests/test_gpu_job_aggregation.py run it over.

run_job_aggregation walks the reference workflow as tests/pipeline.py does --
  participate  client/src/participate.rs:53-98    mask, mask payload, shares, one payload per clerk
  snapshot     server/src/stores.rs:86-101        [participation][clerk] -> [clerk][participation]
  clerk        client/src/clerk.rs:63-107         decode, combine in snapshot order, result payload
  reveal       client/src/receive.rs:98-157       decode, mask combine, reconstruct, unmask, positive
-- over one of three backends:

  device  sda_participant_job_dev -> sda_snapshot_transpose_dev -> sda_clerk_job_dev -> sda_recipient_job_dev or
          sda_recipient_job_decoded_dev.  Nothing leaves the device between the calls.  Every participant writes its
          clerk payloads straight behind the previous participant's, so that buffer is the snapshot's source as it
          stands, and its mask payload behind the previous mask payload, so that buffer is the Full-mask fold's
          (bytes, blob_off) pair and the recipient's (seed_bytes, seed_off) pair as it stands.  A clerk's job is the
          snapshot's dst + clerk_base[c] with clerk_off[c].  The clerks' result payloads land back to back in one
          buffer in the order the clerk jobs run, and the recipient gets that buffer with running host offsets.  No
          entry point's alignment rule forbade a running offset, so there is no device-to-device copy anywhere: only
          buffer starts are 16-byte aligned (the snapshot's src and dst, the clerk's and the recipient's byte
          buffers).  What the (bytes, off[n + 1]) form cannot express is a reordered subset of blobs; the plan's clerk
          subset is therefore run first and in the recipient's order, which a clerk committee is free to do.  With
          Full masking the mask payloads are folded by sda_clerk_job_dev(ms.modulus, ..., payload = NULL) under the
          plan's tiling and the recipient takes that state.  Every buffer lies between guards of the project's poison
          patterns (0xA5 bytes, 0x5A.. words); the guards, and the unused tail of every byte buffer, are checked at
          the end of the chain.
  host    sda_participant_job -> list indexing (the server's host path is no engine call) -> sda_clerk_job ->
          sda_recipient_job or sda_recipient_job_decoded.  The host clerk job has one form: the tiling is ignored.
  oracle  CPU only, from the pieces the suite already trusts: the draws of tests/draws_model.py, the Additive keyed
          model of tests/test_additive_keyed_model.py and the packed keyed model (oracle.packed_generate over the draws
          model, as test_gpu_packed_keyed.py's CPU anchor composes it), oracle.full_mask / chacha_mask,
          oracle.varint_encode, oracle.snapshot_transpose, oracle.combine in snapshot order, oracle.chacha_mask_combine,
          oracle.packed_reconstruct (combine for Additive), unmask, positive; the decoded reveal is
          tests/recipient_decoded_model.py.  Its role methods are the override points of the deliberately faulty
          backends in tests/test_job_aggregation_model.py.

The reference is none of them: with secrets s_p in (-m, m) the recipient's positive output is (sum_p s_p[i]) mod m in
Python integers (expected()).  The driver asserts the precondition of that identity, 2 <= m <= 2^62 with the masking
modulus equal to m: above 2^62 the reference's wrapping `(r + v) % m` (combiner.rs:16-28) may leave i64 and the result
is then defined by the oracle alone, not by the sum.  PackedShamir clerk results are read over [0, B), so a longer
result (a clerk that folded a longer vector) is not an error of the recipient job; the chain never produces one.

A (key, stream id) pair never serves two jobs: every participant has its own 256-bit key from the case id and its
own two stream ids, and the driver asserts it.

Faulty clerks (Plan.faulty) misbehave by running the real clerk job on wrong inputs: "stale" leaves the last
participation out, "double" folds participation 0 a second time (a continuing call on the device), "modulus" combines
under m - 2.
"""
import ctypes as C
import itertools
import zlib
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from sda_amd import engine as E
from sda_amd import schemes as S
from tests import draws_model as DM

EXACT, CANONICAL = E.REVEAL_EXACT, E.REVEAL_CANONICAL
TILINGS = ("one", "two", "each+finish")
FAULT_KINDS = ("stale", "double", "modulus")
POISON8, POISON16, POISON32, POISON64 = 0xA5, 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD_BYTES = 64                  # on each side of every device buffer: a multiple of 16, and the 32 readable bytes
M_MAX = 1 << 62                   # the snapshot's src needs


# =================================================================================================== plan and trace
@dataclass(frozen=True)
class Plan:
    tiling: str = "one"           # the clerk jobs' and the Full-mask fold's: one | two | each+finish
    recipient: str = "job"        # job: sda_recipient_job in `mode`; decoded: sda_recipient_job_decoded
    mode: int = EXACT
    clerks: tuple = ()            # the recipient's clerk subset in its order; () = all, in index order
    faulty: tuple = ()            # ((clerk, kind), ...), kind one of FAULT_KINDS
    every_tiling: bool = False    # device backend: run the clerk stage under all three tilings (Trace.tilings)
    alongside: bool = False       # decoded: also run the plain job over the same payloads (Trace.job_output)


@dataclass
class Trace:
    participant_payloads: list = field(default_factory=list)    # [P][n] bytes
    mask_payloads: list = field(default_factory=list)           # [P] bytes
    transposed: list = field(default_factory=list)              # [n][P] bytes, each clerk's column in snapshot order
    transposed_bytes: Optional[np.ndarray] = None               # device: the snapshot's dst, uint8 [dst_len]
    clerk_base: Optional[np.ndarray] = None                     # device: as sda_snapshot_transpose_dev returned them
    clerk_off: Optional[np.ndarray] = None
    part_off: Optional[np.ndarray] = None                       # device: the snapshot's part_off
    clerk_states: list = field(default_factory=list)            # [n] int64 arrays, under the plan's tiling
    clerk_payloads: list = field(default_factory=list)          # [n] bytes
    combined_mask: Optional[np.ndarray] = None                  # the folded Full mask (None where no backend call
    output: Optional[np.ndarray] = None                         # makes one)
    job_output: Optional[np.ndarray] = None                     # Plan.alongside
    decode: Optional[tuple] = None                              # E.ShareDecode, verdict, wrong of the decoded job
    verdict: Optional[np.ndarray] = None
    wrong: Optional[np.ndarray] = None
    tilings: dict = field(default_factory=dict)                 # tiling -> (states [n], payloads [n], mask)
    clerk_calls: list = field(default_factory=list)             # device: (tiling, clerk, b0, b1, first, pay, job
    records: dict = field(default_factory=dict)                 # record, codec record) of every clerk call


def expected(secrets, m):
    """(sum_p s_p[i]) mod m in Python integers: the reference of the whole chain"""
    P, D = np.asarray(secrets).shape
    return np.asarray([sum(int(secrets[p][i]) for p in range(P)) % m for i in range(D)], np.int64)


def is_packed(ss):
    return isinstance(ss, S.PackedShamir)


def width(ss, D):
    """values per clerk row: D columns, or B batches"""
    return (D + ss.secret_count - 1) // ss.secret_count if is_packed(ss) else D


def clerk_order(ss, plan):
    """the order the clerk jobs run in: the recipient's clerks first, in its order"""
    sel = list(plan.clerks) if plan.clerks else list(range(ss.output_size()))
    return sel, sel + [c for c in range(ss.output_size()) if c not in sel]


def tiles(tiling, P):
    """[(b0, b1, wants the payload)] of a clerk job over P blobs; b0 == b1 is the n_blobs == 0 finish call"""
    if tiling == "one":
        return [(0, P, True)]
    if tiling == "two":
        h = max(1, P // 2)
        return [(0, h, False), (h, P, True)]
    assert tiling == "each+finish"
    return [(p, p + 1, False) for p in range(P)] + [(P, P, True)]


# =================================================================================================== the driver
def run_job_aggregation(backend, masking, sharing, secrets, keys, seeds, plan):
    """secrets [P][D]; keys [P] of (key words [8], mask stream id, share stream id); seeds [P] of ChaCha seed words
    (None without ChaCha masking).  Returns the backend's Trace."""
    m = sharing.modulus
    secrets = np.ascontiguousarray(secrets, dtype=np.int64)
    P, D = secrets.shape
    assert P >= 1 and D >= 1
    assert 2 <= m <= M_MAX, "the sum identity needs 2 <= m <= 2^62"
    assert all(-m < int(v) < m for v in (secrets.min(), secrets.max())), "secrets must lie in (-m, m)"
    assert not masking.has_mask() or masking.modulus == m
    assert len(keys) == P and len(seeds) == P
    pairs = {(tuple(int(w) for w in key), int(s)) for key, ms_id, ss_id in keys for s in (ms_id, ss_id)}
    assert len(pairs) == 2 * P, "a (key, stream) pair must never serve two jobs"
    assert plan.tiling in TILINGS and plan.recipient in ("job", "decoded")
    assert all(kind in FAULT_KINDS for _, kind in plan.faulty) and (P >= 2 or not plan.faulty)
    sel, order = clerk_order(sharing, plan)
    assert len(set(sel)) == len(sel)
    backend.begin(masking, sharing, P, D, plan)
    for p in range(P):
        backend.participant(p, secrets[p], keys[p][0], keys[p][1], keys[p][2], seeds[p])
    backend.snapshot()
    for tiling in (TILINGS if plan.every_tiling else (plan.tiling,)):
        backend.clerks(tiling, order)
    backend.recipient(sel)
    return backend.finish()


class Backend:
    name = "?"

    def begin(self, ms, ss, P, D, plan):
        self.ms, self.ss, self.P, self.D, self.plan = ms, ss, P, D, plan
        self.m, self.n, self.W = ss.modulus, ss.output_size(), width(ss, D)
        self.faulty = dict(plan.faulty)
        self.tr = Trace()

    def finish(self):
        return self.tr

    def _keep_tiling(self, tiling, states, payloads, mask):
        self.tr.tilings[tiling] = (states, payloads, mask)
        if tiling == self.plan.tiling:
            self.tr.clerk_states, self.tr.clerk_payloads, self.tr.combined_mask = states, payloads, mask


# =================================================================================================== oracle
class OracleBackend(Backend):
    name = "oracle"

    def __init__(self, O):
        self.O = O

    def begin(self, ms, ss, P, D, plan):
        super().begin(ms, ss, P, D, plan)
        if is_packed(ss):
            self.pp = self.O.packed_params(ss.secret_count, ss.share_count, ss.privacy_threshold(), ss.prime_modulus,
                                           ss.omega_secrets, ss.omega_shares)

    # ---- participant
    def participant(self, p, secrets, key, mask_stream, share_stream, seed):
        from tests import test_additive_keyed_model as AM
        O, m, D = self.O, self.m, self.D
        if isinstance(self.ms, S.FullMasking):
            mask = DM.draws(key, mask_stream, 0, D, m)
            masked, mask_payload = O.full_mask(m, mask, secrets), O.varint_encode(mask)
        elif isinstance(self.ms, S.ChaChaMasking):
            masked = O.chacha_mask(m, np.asarray(seed, np.uint32), secrets)
            mask_payload = O.varint_encode(np.asarray(seed, np.int64))
        else:
            masked, mask_payload = secrets, b""
        if is_packed(self.ss):
            t = self.ss.privacy_threshold()
            shares = O.packed_generate(self.pp, masked, DM.draws(key, share_stream, 0, self.W * t, m - 1))
        else:
            shares = AM.expected(m, self.n, masked, key=key, stream_id=share_stream)
        self.tr.participant_payloads.append([O.varint_encode(r) for r in shares])
        self.tr.mask_payloads.append(mask_payload)

    # ---- server
    def snapshot(self):
        self.tr.transposed = self.O.snapshot_transpose(self.tr.participant_payloads)

    # ---- clerks
    def clerk(self, c, blobs):
        """(state, payload) of clerk c over its column"""
        O, m = self.O, self.m
        kind = self.faulty.get(c)
        if kind == "stale":
            blobs = blobs[:-1]
        elif kind == "double":
            blobs = list(blobs) + [blobs[0]]
        elif kind == "modulus":
            m = m - 2
        state = O.combine(m, np.stack([O.varint_decode(b) for b in blobs]))
        return state, O.varint_encode(state)

    def fold_masks(self, payloads):
        return self.O.combine(self.m, np.stack([self.O.varint_decode(b) for b in payloads]))

    def clerks(self, tiling, order):
        done = {c: self.clerk(c, self.tr.transposed[c]) for c in order}
        mask = self.fold_masks(self.tr.mask_payloads) if isinstance(self.ms, S.FullMasking) else None
        self._keep_tiling(tiling, [done[c][0] for c in range(self.n)], [done[c][1] for c in range(self.n)], mask)

    # ---- recipient
    def indexed(self, sel):
        """[(clerk index, result payload)] as the recipient is handed them"""
        return [(c, self.tr.clerk_payloads[c]) for c in sel]

    def recipient(self, sel):
        from tests import recipient_decoded_model as RD
        O, m, D, tr = self.O, self.m, self.D, self.tr
        indexed = self.indexed(sel)
        idx = [c for c, _ in indexed]
        rows = [O.varint_decode(b) for _, b in indexed]
        if isinstance(self.ms, S.FullMasking):
            mask = tr.combined_mask
        elif isinstance(self.ms, S.ChaChaMasking):
            mask = O.chacha_mask_combine(m, D, np.stack([O.varint_decode(b) for b in tr.mask_payloads]))
        else:
            mask = None

        def job():
            if is_packed(self.ss):
                rc, masked = O.packed_reconstruct(self.pp, D, idx, np.stack([r[:self.W] for r in rows]))
                assert rc == 0
            else:
                masked = O.combine(m, np.stack(rows))
            return O.positive(m, masked if mask is None else O.unmask(m, mask, masked))

        if self.plan.recipient == "job":
            tr.output = job()
            return
        exp = RD.run(O, self.ms, None, self.ss, D, list(zip(idx, rows)), mask=[] if mask is None else mask)
        tr.output, tr.verdict, tr.wrong = exp.out, exp.verdict, exp.wrong
        tr.decode = E.ShareDecode(exp.redundancy, exp.radius, exp.bad_batches, exp.first_bad, exp.undecoded, exp.blame)
        if self.plan.alongside:
            tr.job_output = job()


# =================================================================================================== host
class HostBackend(Backend):
    name = "host"

    def __init__(self, engine):
        self.eng = engine

    def participant(self, p, secrets, key, mask_stream, share_stream, seed):
        rows, mask = self.eng.participant_job(self.ms, self.ss, secrets, key, mask_stream, share_stream, seed=seed,
                                              mode=EXACT)
        self.tr.participant_payloads.append(rows)
        self.tr.mask_payloads.append(mask)
        self.tr.records["participant_job"] = self.eng.participant_job_last_launch()

    def snapshot(self):
        pay = self.tr.participant_payloads
        self.tr.transposed = [[pay[p][c] for p in range(self.P)] for c in range(self.n)]

    def clerks(self, tiling, order):
        done = {}
        for c in order:
            blobs, scheme = self.tr.transposed[c], self.ss
            kind = self.faulty.get(c)
            if kind == "stale":
                blobs = blobs[:-1]
            elif kind == "double":
                blobs = list(blobs) + [blobs[0]]
            elif kind == "modulus":
                scheme = S.Additive(self.n, self.m - 2)
            done[c] = self.eng.clerk_job(scheme, blobs)
        self.tr.records["clerk_job"] = self.eng.clerk_job_last_launch()
        self._keep_tiling(tiling, [done[c][0] for c in range(self.n)], [done[c][1] for c in range(self.n)], None)

    def _job(self, indexed):
        """sda_recipient_job into a guarded host buffer, compared whole"""
        eng, D, G = self.eng, self.D, 16
        ms, ss = self.ms.c(), self.ss.c()
        masks = self.tr.mask_payloads if self.ms.has_mask() else []
        mbufs, mptrs, mlens, nm = E.Engine._blobs(masks)
        sbufs, sptrs, slens, ns = E.Engine._blobs([b for _, b in indexed])
        idx = np.asarray([c for c, _ in indexed], np.uint64)
        out = np.full(G + D + G, POISON64, np.int64)
        olen = C.c_uint64(0)
        E._check(eng.lib.sda_recipient_job(eng.h, C.byref(ms), mptrs, mlens, nm, C.byref(ss), D, E._ptr(idx, E._u64p),
                                           sptrs, slens, ns, self.m, self.plan.mode,
                                           C.cast(out.ctypes.data + 8 * G, E._i64p), D, C.byref(olen)))
        assert olen.value == D
        assert (out[:G] == POISON64).all() and (out[G + D:] == POISON64).all(), "host out guards"
        return out[G:G + D].copy()

    def recipient(self, sel):
        eng, tr = self.eng, self.tr
        indexed = [(c, tr.clerk_payloads[c]) for c in sel]
        if self.plan.recipient == "job":
            tr.output = self._job(indexed)
            tr.records["recipient_job"] = tuple(eng.recipient_job_last_launch())
            tr.records["recipient"] = tuple(eng.recipient_last_launch())
            return
        masks = tr.mask_payloads if self.ms.has_mask() else []
        tr.output, tr.decode, tr.verdict, tr.wrong = eng.recipient_job_decoded(self.ms, masks, self.ss, self.D, indexed,
                                                                               self.m)
        tr.records["recipient_job"] = tuple(eng.recipient_job_last_launch())
        tr.records["recipient_decoded"] = tuple(eng.recipient_decoded_last_launch())
        tr.records["packed_decode"] = eng.packed_decode_last_launch()
        if self.plan.alongside:
            tr.job_output = self._job(indexed)


# =================================================================================================== device
class _Guarded:
    """`n` elements of `dtype` on the device between guards, all poisoned"""
    POISON = {np.uint8: POISON8, np.uint16: POISON16, np.uint32: POISON32, np.int64: POISON64}
    SIGNED = {np.uint16: np.int16, np.uint32: np.int32}

    def __init__(self, torch, dtype, n, what):
        self.torch, self.dtype, self.n, self.what = torch, dtype, n, what
        self.size = np.dtype(dtype).itemsize
        self.g = GUARD_BYTES // self.size
        host = np.full(self.g + n + self.g, self.POISON[dtype], dtype)
        self.t = torch.from_numpy(host.view(self.SIGNED.get(dtype, dtype))).cuda()
        self.ptr = self.t.data_ptr() + GUARD_BYTES
        assert self.ptr % 16 == 0
        self.used = 0                                            # byte buffers: the bytes the chain has written

    def host(self, used=None):
        """the `used` (default: all n) elements, after checking that everything around them is still poison"""
        self.torch.cuda.synchronize()
        h = self.t.cpu().numpy().view(self.dtype)
        used = self.n if used is None else used
        poison = self.dtype(self.POISON[self.dtype])
        assert (h[:self.g] == poison).all(), f"{self.what}: the guard in front was written"
        assert (h[self.g + used:] == poison).all(), f"{self.what}: written past element {used}"
        return h[self.g:self.g + used].copy()


class DeviceBackend(Backend):
    name = "device"

    def __init__(self, engine):
        import torch
        self.eng, self.torch = engine, torch

    def begin(self, ms, ss, P, D, plan):
        super().begin(ms, ss, P, D, plan)
        row, mb = E.participant_job_payload_bound(ms, ss, D)
        self.row = row
        self.pay = _Guarded(self.torch, np.uint8, P * self.n * row, "participant payloads")
        self.mpay = _Guarded(self.torch, np.uint8, P * mb, "mask payloads")
        self.part_off, self.mask_off = [0], [0]
        self.stage = {}

    def participant(self, p, secrets, key, mask_stream, share_stream, seed):
        pay, mpay = self.pay, self.mpay
        sec = self.torch.from_numpy(np.ascontiguousarray(secrets)).cuda()
        rb, mlen = self.eng.participant_job_dev(self.ms, self.ss, sec.data_ptr(), self.D, key, mask_stream, share_stream,
                                                pay.ptr + pay.used, pay.n - pay.used, mpay.ptr + mpay.used,
                                                mpay.n - mpay.used, seed=seed, mode=EXACT)
        for b in rb:
            self.part_off.append(self.part_off[-1] + int(b))
        pay.used = self.part_off[-1]
        mpay.used += mlen
        self.mask_off.append(mpay.used)
        self.tr.records["participant_job"] = self.eng.participant_job_last_launch()

    def snapshot(self):
        eng, P, n = self.eng, self.P, self.n
        off = np.asarray(self.part_off, np.uint64)
        need, _, _ = eng.snapshot_transpose_dev(self.pay.ptr, off, P, n)
        self.dst = _Guarded(self.torch, np.uint8, need, "snapshot dst")
        dlen, self.base, self.coff = eng.snapshot_transpose_dev(self.pay.ptr, off, P, n, self.dst.ptr, need)
        assert dlen == need
        self.tr.records["snapshot"] = eng.snapshot_last_launch()

    def _calls(self, c, tiling):
        """[(b0, b1, first_participation, wants the payload, modulus)] of clerk c's job"""
        P, m = self.P, self.m
        kind = self.faulty.get(c)
        if kind == "stale":
            return [(0, P - 1, 0, True, m)]
        if kind == "double":
            return [(0, P, 0, False, m), (0, 1, P, True, m)]
        if kind == "modulus":
            return [(0, P, 0, True, m - 2)]
        return [(b0, b1, b0, pay, m) for b0, b1, pay in tiles(tiling, P)]

    def clerks(self, tiling, order):
        eng, W, n = self.eng, self.W, self.n
        states = _Guarded(self.torch, np.int64, n * W, f"clerk states ({tiling})")
        cpay = _Guarded(self.torch, np.uint8, n * W * 10, f"clerk payloads ({tiling})")
        poff = {}
        for c in order:
            for b0, b1, first, pay, mod in self._calls(c, tiling):
                dim, plen = eng.clerk_job_dev(mod, self.dst.ptr + int(self.base[c]), self.coff[c][b0:b1 + 1],
                                              states.ptr + 8 * W * c, W, first_participation=first,
                                              prior_dim=W if first else 0,
                                              payload_ptr=cpay.ptr + cpay.used if pay else None,
                                              payload_cap=cpay.n - cpay.used if pay else 0)
                assert dim == W, (c, b0, b1, dim)
                self.tr.clerk_calls.append((tiling, c, b0, b1, first, pay, eng.clerk_job_last_launch(),
                                            eng.codec_last_launch()))
                if pay:
                    poff[c] = (cpay.used, cpay.used + plen)
                    cpay.used += plen
        mstate = None
        if isinstance(self.ms, S.FullMasking):
            mstate = _Guarded(self.torch, np.int64, self.D, f"folded mask ({tiling})")
            off = np.asarray(self.mask_off, np.uint64)
            for b0, b1, _ in tiles(tiling, self.P):
                if b0 == b1:
                    continue                                     # no payload is asked for: nothing to finish
                dim, _ = eng.clerk_job_dev(self.ms.modulus, self.mpay.ptr, off[b0:b1 + 1], mstate.ptr, self.D,
                                           first_participation=b0, prior_dim=self.D if b0 else 0)
                assert dim == self.D
        self.stage[tiling] = (states, cpay, poff, mstate)

    def _inputs(self, sel):
        states, cpay, poff, mstate = self.stage[self.plan.tiling]
        coff = [poff[sel[0]][0]] + [poff[c][1] for c in sel]
        assert all(poff[a][1] == poff[b][0] for a, b in zip(sel, sel[1:])), "the recipient's blobs lie back to back"
        kw = {}
        if isinstance(self.ms, S.FullMasking):
            kw = dict(mask_ptr=mstate.ptr, mask_len=self.D)
        elif isinstance(self.ms, S.ChaChaMasking):
            kw = dict(seed_ptr=self.mpay.ptr, seed_off=np.asarray(self.mask_off, np.uint64))
        return cpay.ptr, np.asarray(coff, np.uint64), kw

    def _job(self, sel):
        eng, D = self.eng, self.D
        ptr, coff, kw = self._inputs(sel)
        out = _Guarded(self.torch, np.int64, D, "out")
        assert eng.recipient_job_dev(self.ms, self.ss, D, sel, ptr, coff, self.m, out.ptr, D, mode=self.plan.mode,
                                     **kw) == D
        return out.host()

    def recipient(self, sel):
        eng, D, tr = self.eng, self.D, self.tr
        if self.plan.recipient == "job":
            tr.output = self._job(sel)
            tr.records["recipient_job"] = tuple(eng.recipient_job_last_launch())
            tr.records["recipient"] = tuple(eng.recipient_last_launch())
            return
        ptr, coff, kw = self._inputs(sel)
        out = _Guarded(self.torch, np.int64, D, "decoded out")
        verdict = _Guarded(self.torch, np.uint16, self.W, "verdict")
        wrong = _Guarded(self.torch, np.uint32, self.W, "wrong")
        olen, tr.decode = eng.recipient_job_decoded_dev(self.ms, self.ss, D, sel, ptr, coff, self.m, out.ptr, D,
                                                        verdict_ptr=verdict.ptr, wrong_ptr=wrong.ptr, **kw)
        assert olen == D
        tr.output, tr.verdict, tr.wrong = out.host(), verdict.host(), wrong.host()
        tr.records["recipient_job"] = tuple(eng.recipient_job_last_launch())
        tr.records["recipient_decoded"] = tuple(eng.recipient_decoded_last_launch())
        tr.records["packed_decode"] = eng.packed_decode_last_launch()
        if self.plan.alongside:
            tr.job_output = self._job(sel)

    def finish(self):
        """read everything back; every guard and every unused tail must still be poison"""
        tr, P, n, W = self.tr, self.P, self.n, self.W
        raw = self.pay.host(self.pay.used).tobytes()
        po = self.part_off
        tr.participant_payloads = [[raw[po[p * n + c]:po[p * n + c + 1]] for c in range(n)] for p in range(P)]
        raw = self.mpay.host(self.mpay.used).tobytes()
        tr.mask_payloads = [raw[self.mask_off[p]:self.mask_off[p + 1]] for p in range(P)]
        tr.part_off = np.asarray(po, np.uint64)
        tr.transposed_bytes = self.dst.host()
        tr.clerk_base, tr.clerk_off = self.base.copy(), self.coff.copy()
        raw = tr.transposed_bytes.tobytes()
        tr.transposed = [[raw[int(self.base[c] + self.coff[c][p]):int(self.base[c] + self.coff[c][p + 1])]
                          for p in range(P)] for c in range(n)]
        for tiling, (states, cpay, poff, mstate) in self.stage.items():
            st = states.host().reshape(n, W)
            raw = cpay.host(cpay.used).tobytes()
            self._keep_tiling(tiling, [st[c] for c in range(n)], [raw[poff[c][0]:poff[c][1]] for c in range(n)],
                              mstate.host() if mstate is not None else None)
        return tr


# =================================================================================================== the cases
M32, M36, M61 = 2147482801, 68719676673, (1 << 61) - 1
SCHEME_NAMES = ("add32", "add36", "add61", "fl", "cp", "b16", "wide")
MASKINGS = ("none", "full", "chacha1", "chacha8")
PARTICIPANTS = (1, 2, 5, 33)      # a column shorter than, equal to, longer than the combine's 4-row step; past 32
DKINDS = ("1", "k-1", "k+1", "2049", "big")
RECIPIENTS = ("all-exact", "all-canon", "first-rev", "dec-all", "dec-r1", "dec-r2")
AXES = ("scheme", "masking", "P", "dkind", "tiling", "recipient")
VALUES = {"scheme": SCHEME_NAMES, "masking": MASKINGS, "P": PARTICIPANTS, "dkind": DKINDS, "tiling": TILINGS,
          "recipient": RECIPIENTS}
# each axis meets its neighbours; the scheme, which decides every route, also meets the dimension and the recipient
PAIRS = (("scheme", "masking"), ("masking", "P"), ("P", "dkind"), ("dkind", "tiling"), ("tiling", "recipient"),
         ("scheme", "dkind"), ("scheme", "recipient"))


def schemes():
    from tests import pipeline_matrix_cases as PC
    from tests.test_checked_reveal_model import SCHEMES as CHECKED
    # b16: the 16-share register bucket of tests/test_repair_tables.py.  It goes through sda_recipient_job only; the
    # decoded job's own file holds it over that bucket.
    return {"add32": S.Additive(3, M32), "add36": S.Additive(2, M36), "add61": S.Additive(3, M61),
            "fl": S.FULL_LOOP_PACKED, "cp": S.CONFIG_PACKED, "b16": CHECKED["b16"], "wide": PC.wide_scheme()}


def kt_of(ss):
    return ss.reconstruction_threshold()


@dataclass(frozen=True)
class Case:
    scheme: str
    masking: str
    P: int
    dkind: str
    tiling: str
    recipient: str
    faults: int = 0               # (f): the clerks that misbehave

    @property
    def ss(self):
        return schemes()[self.scheme]

    @property
    def k(self):
        return self.ss.secret_count if is_packed(self.ss) else 1

    @property
    def D(self):
        k = self.k
        return {"1": 1, "k-1": k - 1, "k+1": k + 1, "2049": 2049, "big": 2048 * k + 5}.get(self.dkind) or \
            int(self.dkind)

    @property
    def id(self):
        f = f"-e{self.faults}" if self.faults else ""
        return f"{self.scheme}-{self.masking}-P{self.P}-D{self.D}-{self.tiling}-{self.recipient}{f}"

    @property
    def ms(self):
        m = self.ss.modulus
        if self.masking == "none":
            return S.NoMasking()
        if self.masking == "full":
            return S.FullMasking(m)
        return S.ChaChaMasking(m, self.D, 32 * int(self.masking[6:]))

    @property
    def clerks(self):
        ss, n, kt = self.ss, self.ss.output_size(), kt_of(self.ss)
        if self.recipient == "first-rev":
            return tuple(reversed(range(kt)))
        if self.recipient in ("dec-r1", "dec-r2"):
            return tuple(range(n - kt - int(self.recipient[-1]), n))
        return ()

    @property
    def faulty(self):
        """(f): the misbehaving clerks, spread over basis and check positions, the three kinds rotating"""
        n = self.ss.output_size()
        where = [1, n - 1, n // 2, 0, n - 3, 5 % n]
        return tuple((where[i], FAULT_KINDS[i % 3]) for i in range(self.faults))

    def plan(self, every_tiling=False):
        return Plan(tiling=self.tiling, recipient="decoded" if self.recipient.startswith("dec") else "job",
                    mode=CANONICAL if self.recipient == "all-canon" else EXACT, clerks=self.clerks,
                    faulty=self.faulty, every_tiling=every_tiling, alongside=bool(self.faults))


def valid(c):
    ss = c.ss
    if c.dkind == "k-1" and c.k == 1:
        return False                                             # no dimension 0 aggregation
    if c.dkind == "big" and c.P > 5:
        return False                                             # the largest case stays in the tens of MB
    if c.recipient.startswith("dec"):
        if c.scheme not in ("fl", "cp") or c.dkind == "big":
            return False                                         # the decoded job: k <= 8, at most 32 results
        if ss.output_size() < kt_of(ss) + (2 if c.recipient == "dec-r2" else 1):
            return False
        if c.recipient == "dec-r1" and ss.output_size() == kt_of(ss) + 1:
            return False                                         # FULL_LOOP_PACKED from all 8 is redundancy 1
    if c.scheme == "wide" and c.dkind in ("2049", "big") and c.recipient != "first-rev":
        return False                                             # the oracle reveals a 242-clerk batch in 5 ms
    return True


def _fill(fixed, i):
    """the case with `fixed` axes as given and the others rotating with the case index, advanced to the next valid
    combination"""
    free = [a for a in AXES if a not in fixed]
    for shift in sorted(itertools.product(range(7), repeat=len(free)), key=lambda s: (sum(s), s)):
        pick = {a: VALUES[a][(i + AXES.index(a) + s) % len(VALUES[a])] for a, s in zip(free, shift)}
        cand = Case(**fixed, **pick)
        if valid(cand):
            return cand
    return None


def _cases():
    out = []
    for a, b in PAIRS:
        for va in VALUES[a]:
            for vb in VALUES[b]:
                if any(getattr(c, a) == va and getattr(c, b) == vb for c in out):
                    continue
                cand = _fill({a: va, b: vb}, len(out))
                if cand is not None:
                    out.append(cand)
    return out


CASES = _cases()
# (f): CONFIG_PACKED from 26 results (r = 11, e_max = 5) with 1, e_max and e_max + 1 misbehaving clerks, and
# FULL_LOOP_PACKED from 8 (r = 1, e_max = 0) with one
FAULT_CASES = [Case("cp", "full", 5, "83", "two", "dec-all", faults=1),
               Case("cp", "chacha8", 5, "83", "each+finish", "dec-all", faults=5),
               Case("cp", "none", 5, "83", "one", "dec-all", faults=6),
               Case("fl", "full", 5, "83", "one", "dec-all", faults=1)]


def _rng(case_id, salt):
    return np.random.default_rng([zlib.crc32(case_id.encode()), salt])


def inputs(case):
    """(secrets [P][D], keys, seeds) of a case, from its id: secrets uniform in (-m, m) with column 0 holding 0, +-1
    and +-(m - 1) across the participants (rotated by the id, so that P = 1 meets each of them over the cases)"""
    m, P, D = case.ss.modulus, case.P, case.D
    secrets = _rng(case.id, 0).integers(-(m - 1), m, size=(P, D), dtype=np.int64)
    special = [0, 1, -1, m - 1, -(m - 1)]
    rot = zlib.crc32(case.id.encode())
    for p in range(P):
        secrets[p, 0] = special[(rot + p) % 5]
    keys, seeds = [], []
    for p in range(P):
        key = tuple(int(w) for w in _rng(case.id, 1 + p).integers(0, 1 << 32, size=8, dtype=np.uint64))
        keys.append((key, 2 * p + 1, 2 * p + 2))
        words = case.ms.seed_words() if isinstance(case.ms, S.ChaChaMasking) else 0
        seeds.append([int(w) for w in _rng(case.id, 1000 + p).integers(0, 1 << 32, size=words, dtype=np.uint64)]
                     if words else None)
    return secrets, keys, seeds


def run_case(backend, case, every_tiling=False):
    secrets, keys, seeds = inputs(case)
    return run_job_aggregation(backend, case.ms, case.ss, secrets, keys, seeds, case.plan(every_tiling))
