"""In-process measurement of the robust recipient job: configs[2]'s scheme (PackedShamir k=8 n=26
t=7) at D = 1M from 26 and from 17 clerk results, 1000 Full masks or 256 ChaCha seeds.  One process; the variants of
a leg are interleaved block by block with their order rotated from round to round, and each baseline's own spread
over its blocks (max - min) is printed next to every comparison.  A block is one warm call and then 2 timed calls of a
host form (0.1 to 8 s each) or 200 timed calls of a device form (0.1 to 1 ms each).
    python scripts/recipient_decoded_inproc.py [rounds] [--baseline-lib PATH]
Legs:
    host form     sda_recipient_job_decoded against today's robust sequence -- sda_varint_decode per blob,
                  sda_secret_reconstruct_decoded, sda_mask_combine, sda_secret_unmask, sda_recipient_positive --
                  run through the library at --baseline-lib (another build, e.g. the parent commit's; default: this
                  build, whose sequence calls are unchanged).  PASS: faster by more than the sequence's spread.
    device form   sda_recipient_job_decoded_dev against sda_recipient_job_dev (not robust) on the same buffers:
                  what the robustness costs in the recipient's call.  Ratio only.
    route         SDA_RECIPIENT_FUSE_UNMASK=1 against =0 on the device form.  Route 1 ships as the default only if
                  it is not slower than route 2 by more than route 2's spread.
    two wrong     the host and device legs at 26 results, Full masks, clerks 5 and 20 answering with their
                  neighbours' payloads: every batch corrected.
Every call's counts are asserted, and its output is compared once with the plain job's on the clean payloads.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402
from sda_amd import engine as E  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = int(args[0]) if args else 4
base_lib = sys.argv[sys.argv.index("--baseline-lib") + 1] if "--baseline-lib" in sys.argv else None
torch.cuda.init()
eng = Engine(0)
old = Engine(0, lib_path=base_lib) if base_lib else eng
st = torch.cuda.current_stream().cuda_stream

sch = S.CONFIG_PACKED
p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
D = 1_000_000
B = D // k
N_FULL, N_SEEDS, DISTINCT = 1000, 256, 4
DEV_REPS = 200                 # calls per timed block of the device legs: 30 ms and more of work a block


def med(x):
    s = sorted(x)
    return s[len(s) // 2]


# ---- inputs: one sharing, its payloads, the masks' payloads ----
sec = torch.empty((1, D), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(sec.data_ptr(), 1, D, 0x5DC1, 0, p, st)
drw = torch.empty((B, t), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(drw.data_ptr(), B, t, 0x5DC2, 0, p - 1, st)
sh = torch.empty((n, B), dtype=torch.int64, device="cuda")
eng.packed_generate_dev(sch, sec.data_ptr(), D, 1, drw.data_ptr(), sh.data_ptr(), st)
torch.cuda.synchronize()
rows = sh.cpu().numpy()
clerk_blobs = [eng.varint_encode(r) for r in rows]
rng = np.random.default_rng(0x5DC3)
# 1000 Full masks: DISTINCT different payloads, each passed N_FULL / DISTINCT times (the call reads every one)
full_rows = [rng.integers(0, p, D, dtype=np.int64) for _ in range(DISTINCT)]
full_blobs = [eng.varint_encode(r) for r in full_rows]
seed_rows = [rng.integers(0, 2**32, 8, dtype=np.int64) for _ in range(N_SEEDS)]
seed_blobs = [eng.varint_encode(r) for r in seed_rows]
MASKS = {
    "full": (S.FullMasking(p), [full_blobs[i % DISTINCT] for i in range(N_FULL)]),
    "chacha": (S.ChaChaMasking(p, D, 256), seed_blobs),
}


def blob_args(blobs):
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    ptrs = (E._u8p * max(len(bufs), 1))(*[b.ctypes.data_as(E._u8p) for b in bufs])
    lens = (C.c_uint64 * max(len(bufs), 1))(*[len(b) for b in blobs])
    return bufs, ptrs, lens, len(bufs)


def host_new(kind, cnt, blobs, expect):
    ms, mblobs = MASKS[kind]
    msc, ssc = ms.c(), sch.c()
    mkeep, mptrs, mlens, nm = blob_args(mblobs)
    ckeep, cptrs, clens, nc = blob_args(blobs[:cnt])
    idx = np.arange(cnt, dtype=np.uint64)
    out = np.zeros(D, np.int64)
    olen = C.c_uint64()
    cs = [C.c_uint64() for _ in range(5)]
    blame = np.zeros(cnt, np.uint64)

    def run():
        E._check(eng.lib.sda_recipient_job_decoded(eng.h, C.byref(msc), mptrs, mlens, nm, C.byref(ssc), D,
                                                   E._ptr(idx, E._u64p), cptrs, clens, nc, p, E._ptr(out), D,
                                                   C.byref(olen), None, None, *[C.byref(c) for c in cs],
                                                   E._ptr(blame, E._u64p)))
        assert (cs[2].value, cs[4].value) == expect, [c.value for c in cs]
        return out
    run.keep = (mkeep, ckeep)
    return run


def host_sequence(kind, cnt, blobs, expect):
    ms, mblobs = MASKS[kind]

    def run():
        crow = [old.varint_decode(b) for b in blobs[:cnt]]
        mrow = [old.varint_decode(b) for b in mblobs]
        secrets, dec, _, _ = old.secret_reconstruct_decoded(sch, D, list(zip(range(cnt), crow)), want_verdict=False,
                                                            want_wrong=False)
        assert (dec.bad_batches, dec.undecoded) == expect, dec
        mask = old.mask_combine(ms, mrow)
        return old.positive(p, old.secret_unmask(ms, (mask, secrets)))
    return run


class DevJob:
    def __init__(self, kind, cnt, blobs):
        self.ms, mblobs = MASKS[kind]
        self.cnt = cnt
        lens = [len(b) for b in blobs[:cnt]]
        self.coff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.cbytes = torch.frombuffer(bytearray(b"".join(blobs[:cnt]) + bytes(32)), dtype=torch.uint8).cuda()
        self.kw = {}
        if kind == "full":
            m = sum(r * (N_FULL // DISTINCT) for r in full_rows) % p       # the fold of full.rs:38-51, canonical
            self.mask = torch.from_numpy(m).cuda()
            self.kw = dict(mask_ptr=self.mask.data_ptr(), mask_len=D)
        else:
            self.soff = np.concatenate([[0], np.cumsum([len(b) for b in mblobs])]).astype(np.uint64)
            self.sbytes = torch.frombuffer(bytearray(b"".join(mblobs) + bytes(32)), dtype=torch.uint8).cuda()
            self.kw = dict(seed_ptr=self.sbytes.data_ptr(), seed_off=self.soff)
        self.out = torch.empty(D, dtype=torch.int64, device="cuda")

    def decoded(self, expect):
        def run():
            _, dec = eng.recipient_job_decoded_dev(self.ms, sch, D, list(range(self.cnt)), self.cbytes.data_ptr(),
                                                   self.coff, p, self.out.data_ptr(), D, stream=st, **self.kw)
            assert (dec.bad_batches, dec.undecoded) == expect, dec
            return self.out
        return run

    def plain(self):
        def run():
            eng.recipient_job_dev(self.ms, sch, D, list(range(self.cnt)), self.cbytes.data_ptr(), self.coff, p,
                                  self.out.data_ptr(), D, stream=st, **self.kw)
            return self.out
        return run


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def compare(title, variants, reps, gate=None, env=None):
    """variants: {name: callable}; the LAST one is the baseline.  Prints every block, the medians, the baseline's
    spread and the first variant's ratio to it; gate: 'faster' (first faster than baseline by more than the spread)
    or 'not_slower' (first not slower than baseline by more than the spread)."""
    names = list(variants)
    res = {nm: [] for nm in names}
    for r in range(rounds):
        for i in range(len(names)):
            nm = names[(i + r) % len(names)]
            for var, val in (env or {}).get(nm, {}).items():
                os.environ[var] = val
            ms = wall(variants[nm], reps)
            for var in (env or {}).get(nm, {}):
                del os.environ[var]
            res[nm].append(ms)
            print(f"{title} round {r} {nm:10s}: {ms:.3f} ms", flush=True)
    a, b = res[names[0]], res[names[-1]]
    spread = max(b) - min(b)
    verdict = ""
    if gate == "faster":
        verdict = ": PASS" if med(b) - med(a) > spread else ": FAIL"
    if gate == "not_slower":
        verdict = ": route 1 ships" if med(a) - med(b) <= spread else ": route 2 ships"
    print(f"{title}: {names[0]} median {med(a):.3f} ms (min {min(a):.3f}, max {max(a):.3f}); {names[-1]} median "
          f"{med(b):.3f} ms (min {min(b):.3f}, max {max(b):.3f}, spread {spread:.3f}); {names[0]} / {names[-1]} = "
          f"{med(a) / med(b):.3f}; difference {med(a) - med(b):+.3f} ms vs spread {spread:.3f} ms{verdict}", flush=True)


def clean_output(kind, cnt):
    ms, mblobs = MASKS[kind]
    return eng.recipient_job(ms, mblobs, sch, D, list(zip(range(cnt), clerk_blobs[:cnt])), p)


two_wrong = list(clerk_blobs)
two_wrong[5], two_wrong[20] = clerk_blobs[6], clerk_blobs[21]
for kind in ("full", "chacha"):
    for cnt, blobs, expect, tag in ((26, clerk_blobs, (0, 0), "consistent"), (17, clerk_blobs, (0, 0), "consistent"),
                                    (26, two_wrong, (B, 0), "two wrong")):
        if tag == "two wrong" and kind != "full":
            continue
        want = clean_output(kind, cnt)
        leg = f"{kind} {cnt} results {tag}"
        new, seq = host_new(kind, cnt, blobs, expect), host_sequence(kind, cnt, blobs, expect)
        assert np.array_equal(new(), want) and np.array_equal(seq(), want), leg
        compare(f"host form, {leg}", {"decoded": new, "sequence": seq}, 2, gate="faster")
        job = DevJob(kind, cnt, blobs)
        dec, plain = job.decoded(expect), job.plain()
        assert np.array_equal(dec().cpu().numpy(), want), leg
        compare(f"device form, {leg}", {"decoded": dec, "job_dev": plain}, DEV_REPS)
        print(f"record: {eng.recipient_decoded_last_launch()} {eng.packed_decode_last_launch()}")
        compare(f"route, {leg}", {"fused": dec, "separate": dec}, DEV_REPS, gate="not_slower",
                env={"fused": {"SDA_RECIPIENT_FUSE_UNMASK": "1"}, "separate": {"SDA_RECIPIENT_FUSE_UNMASK": "0"}})
        del job
