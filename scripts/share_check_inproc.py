"""In-process comparison of the share consistency check with the canonical reveal it precedes ("Share
consistency check"): configs[2]'s scheme (PackedShamir k=8 n=26 t=7), 1000 x 1M (B = 125,000), i64 and int32 share
rows, from all 26 clerks and from 17.  One process; the variants are interleaved launch block by launch block (one
warm launch, then 10 timed between HIP events on the launch stream), so buffer placement and box state are shared
by every variant.  The yardstick of a check is the CANONICAL reveal from the same shares, never the check itself.
    python scripts/share_check_inproc.py [rounds]
The check is the all-consistent one with verdict == NULL; every timed call is asserted to find nothing bad, and the
reveals to return the secrets.  Afterwards, as figures without a gate: the looped path (80 clerks of a k=8 t=7
n=80 scheme, 250 vectors) and the all-bad location pass (one clerk's row replaced, 26 clerks, 100 vectors).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402
from sda_amd import engine as E  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
REPS = 10
torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream


def make_shares(sch, V, D):
    p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
    B = D // k
    sec = torch.empty((V, D), dtype=torch.int64, device="cuda")
    eng.synth_fill_dev(sec.data_ptr(), V, D, 0x5DB2, 0, p, st)
    drw = torch.empty((V, B, t), dtype=torch.int64, device="cuda")
    eng.synth_fill_dev(drw.data_ptr(), V * B, t, 0x5DB3, 0, p - 1, st)
    sh = torch.empty((V, n, B), dtype=torch.int64, device="cuda")
    eng.packed_generate_dev(sch, sec.data_ptr(), D, V, drw.data_ptr(), sh.data_ptr(), st)
    torch.cuda.synchronize()
    return sec, sh


def timed(fn):
    fn()                                                                            # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


sch = S.CONFIG_PACKED
p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
V, D = 1000, 1_000_000
B = D // k
sec, sh26 = make_shares(sch, V, D)
rev = torch.empty((V, D), dtype=torch.int64, device="cuda")
inputs = {}
for cnt in (26, 17):
    idx = list(range(cnt))
    s64 = sh26 if cnt == n else sh26[:, :cnt, :].contiguous()
    inputs[cnt] = (idx, s64, s64.to(torch.int32))
torch.cuda.synchronize()


def variant(kind, width, cnt):
    idx, s64, s32 = inputs[cnt]
    buf = s32 if width == 32 else s64
    if kind == "check":
        fn = eng.packed_check32_dev if width == 32 else eng.packed_check_dev

        def run():
            got = fn(sch, D, idx, V, buf.data_ptr(), None, st)
            assert got.bad_batches == 0 and got.redundancy == cnt - (k + t), got
        nbytes = (width // 8) * V * cnt * B
    else:
        fn = eng.packed_reconstruct32_dev if width == 32 else eng.packed_reconstruct_dev

        def run():
            fn(sch, D, idx, V, buf.data_ptr(), rev.data_ptr(), E.REVEAL_CANONICAL, st)
        nbytes = (width // 8) * V * cnt * B + 8 * V * D
    return run, float(nbytes)


names = [(kind, width, cnt) for cnt in (26, 17) for width in (64, 32) for kind in ("check", "reveal")]
runs = {nm: variant(*nm) for nm in names}
res = {nm: [] for nm in names}
for r in range(rounds):
    for nm in names:
        run, nbytes = runs[nm]
        ms = timed(run)
        res[nm].append(ms)
        if r == 0 and nm[0] == "reveal":
            assert torch.equal(rev, sec), nm
        print(f"round {r} {nm[0]:6s} i{nm[1]} from {nm[2]}: {ms:.4f} ms  {nbytes / ms / 1e9:.3f} TB/s", flush=True)


def med(x):
    s = sorted(x)
    return s[len(s) // 2]


print(f"rec: {eng.packed_check_last_launch()}")
for cnt in (26, 17):
    for width in (64, 32):
        c, v = res[("check", width, cnt)], res[("reveal", width, cnt)]
        print(f"i{width} from {cnt}: check median {med(c):.4f} ms (min {min(c):.4f}, max {max(c):.4f}), canonical reveal "
              f"median {med(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f}), check / reveal = {med(c) / med(v):.3f}")

# ---- figures without a gate ----
# the all-bad location pass: clerk 5's row replaced by clerk 6's, 100 vectors of the job above
Vb = 100
idx, s64, _ = inputs[26]
bad = s64[:Vb].clone()
bad[:, 5, :] = bad[:, 6, :]
torch.cuda.synchronize()
got = None


def all_bad():
    global got
    got = eng.packed_check_dev(sch, D, idx, Vb, bad.data_ptr(), None, st)


ms = [timed(all_bad) for _ in range(3)]
assert got.bad_batches == Vb * B and got.blame[5] == Vb * B and got.first_bad == 0, got
print(f"all-bad (one wrong row, 26 clerks, {Vb} x 1M = {Vb * B} batches, log overflowed -> full pass): "
      f"median {med(ms):.3f} ms per call, {Vb * B / med(ms) / 1e3:.2f} M batches/s; record {eng.packed_check_last_launch()}")
del bad, rev, sec, sh26, inputs, runs
torch.cuda.empty_cache()

# the looped kernel: all 80 clerks of a k=8 t=7 n=80 scheme, 250 vectors
sch80 = S.PackedShamir(8, 80, 7, 2147478481, 697142131, 2080937233)
V80 = 250
_, sh80 = make_shares(sch80, V80, D)
sh80_32 = sh80.to(torch.int32)
idx80 = list(range(80))
for width, buf, fn in ((64, sh80, eng.packed_check_dev), (32, sh80_32, eng.packed_check32_dev)):
    def looped():
        g = fn(sch80, D, idx80, V80, buf.data_ptr(), None, st)
        assert g.bad_batches == 0 and g.redundancy == 65, g
    ms = [timed(looped) for _ in range(3)]
    nbytes = (width // 8) * V80 * 80 * B
    print(f"looped i{width} from 80 ({V80} x 1M): median {med(ms):.3f} ms, {nbytes / med(ms) / 1e9:.3f} TB/s of share "
          f"bytes; record {eng.packed_check_last_launch()}")
