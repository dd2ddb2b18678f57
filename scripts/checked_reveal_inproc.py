"""In-process comparison of the checked reveal with the two calls it replaces ("Checked reveal"):
configs[2]'s scheme (PackedShamir k=8 n=26 t=7), 1000 x 1M (B = 125,000), i64 and int32 share rows, from all 26
clerks and from 17, all consistent, verdict == NULL.  One process; per leg three variants --
    checked    sda_packed_reveal_checked_dev (one fused pass)
    sequence   sda_packed_check_dev, then sda_packed_reconstruct_dev CANONICAL (the yardstick)
    reveal     sda_packed_reconstruct_dev CANONICAL alone
-- interleaved launch block by launch block (one warm launch, then 10 timed between HIP events on the launch stream)
with the order of the variants rotated from round to round, so buffer placement, box state and position in the round
are shared by every variant.
    python scripts/checked_reveal_inproc.py [rounds]
Every timed call is asserted to find nothing bad and, once per variant, to return the secrets.  The requirement: in
all four legs the checked reveal is faster than the sequence by more than the sequence's own spread (max - min of its
block means); the script prints PASS or FAIL per leg.  Afterwards, as figures without a gate: the whole-row fault
(one clerk's row replaced, 26 clerks, 100 vectors) and the composed path (40 clerks of a k=8 t=7 n=80 scheme, 250
vectors).
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


def med(x):
    s = sorted(x)
    return s[len(s) // 2]


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
    chk = eng.packed_check32_dev if width == 32 else eng.packed_check_dev
    rec = eng.packed_reconstruct32_dev if width == 32 else eng.packed_reconstruct_dev
    fused = eng.packed_reveal_checked32_dev if width == 32 else eng.packed_reveal_checked_dev

    def clean(got):
        assert got.bad_batches == 0 and got.redundancy == cnt - (k + t), got

    if kind == "checked":
        return lambda: clean(fused(sch, D, idx, V, buf.data_ptr(), rev.data_ptr(), None, st))
    if kind == "sequence":
        def run():
            clean(chk(sch, D, idx, V, buf.data_ptr(), None, st))
            rec(sch, D, idx, V, buf.data_ptr(), rev.data_ptr(), E.REVEAL_CANONICAL, st)
        return run
    return lambda: rec(sch, D, idx, V, buf.data_ptr(), rev.data_ptr(), E.REVEAL_CANONICAL, st)


KINDS = ("checked", "sequence", "reveal")
legs = [(width, cnt) for cnt in (26, 17) for width in (64, 32)]
runs = {(kind,) + leg: variant(kind, *leg) for leg in legs for kind in KINDS}
res = {nm: [] for nm in runs}
for r in range(rounds):
    for leg in legs:
        for i in range(len(KINDS)):
            kind = KINDS[(i + r) % len(KINDS)]                                      # rotated from round to round
            nm = (kind,) + leg
            rev.zero_()
            ms = timed(runs[nm])
            res[nm].append(ms)
            if r == 0:
                assert torch.equal(rev, sec), nm
            print(f"round {r} {kind:8s} i{leg[0]} from {leg[1]}: {ms:.4f} ms", flush=True)

print(f"rec: {eng.packed_reveal_checked_last_launch()}")
for width, cnt in legs:
    c, s, v = (res[(kind, width, cnt)] for kind in KINDS)
    spread = max(s) - min(s)
    gain = med(s) - med(c)
    print(f"i{width} from {cnt}: checked median {med(c):.4f} ms (min {min(c):.4f}, max {max(c):.4f}); sequence median "
          f"{med(s):.4f} ms (min {min(s):.4f}, max {max(s):.4f}, spread {spread:.4f}); reveal median {med(v):.4f} ms "
          f"(min {min(v):.4f}, max {max(v):.4f}); checked / sequence = {med(c) / med(s):.3f}, checked / reveal = "
          f"{med(c) / med(v):.3f}; gain {gain:.4f} ms vs spread {spread:.4f} ms: "
          f"{'PASS' if max(c) < min(s) and gain > spread else 'FAIL'}")

# ---- figures without a gate ----
# the whole-row fault: clerk 5's row replaced by clerk 6's, 100 vectors of the job above
Vb = 100
idx, s64, _ = inputs[26]
bad = s64[:Vb].clone()
bad[:, 5, :] = bad[:, 6, :]
torch.cuda.synchronize()
got = None


def all_bad():
    global got
    got = eng.packed_reveal_checked_dev(sch, D, idx, Vb, bad.data_ptr(), rev.data_ptr(), None, st)


ms = [timed(all_bad) for _ in range(3)]
assert got.bad_batches == Vb * B and got.blame[5] == Vb * B and got.first_bad == 0, got
assert torch.equal(rev[:Vb], sec[:Vb])
print(f"whole-row fault (26 clerks, {Vb} x 1M = {Vb * B} batches, all corrected): median {med(ms):.3f} ms per call; "
      f"record {eng.packed_reveal_checked_last_launch()}")
del bad, rev, sec, sh26, inputs, runs
torch.cuda.empty_cache()

# the composed path: 40 clerks of a k=8 t=7 n=80 scheme, 250 vectors
sch80 = S.PackedShamir(8, 80, 7, 2147478481, 697142131, 2080937233)
V80 = 250
sec80, sh80 = make_shares(sch80, V80, D)
sh40 = sh80[:, :40, :].contiguous()
del sh80
rev80 = torch.empty((V80, D), dtype=torch.int64, device="cuda")
idx40 = list(range(40))


def composed():
    g = eng.packed_reveal_checked_dev(sch80, D, idx40, V80, sh40.data_ptr(), rev80.data_ptr(), None, st)
    assert g.bad_batches == 0 and g.redundancy == 25, g


def sequence80():
    g = eng.packed_check_dev(sch80, D, idx40, V80, sh40.data_ptr(), None, st)
    assert g.bad_batches == 0
    eng.packed_reconstruct_dev(sch80, D, idx40, V80, sh40.data_ptr(), rev80.data_ptr(), E.REVEAL_CANONICAL, st)


mc = [timed(composed) for _ in range(3)]
assert torch.equal(rev80, sec80)
ms = [timed(sequence80) for _ in range(3)]
print(f"composed i64 from 40 of 80 ({V80} x 1M): median {med(mc):.3f} ms; check + canonical reveal {med(ms):.3f} ms; "
      f"record {eng.packed_reveal_checked_last_launch()}")
