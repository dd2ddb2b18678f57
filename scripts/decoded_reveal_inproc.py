"""In-process measurement of the decoded reveal ("Decoded reveal") against the checked reveal:
configs[2]'s scheme (PackedShamir k=8 n=26 t=7), i64 and int32 share rows.  One process; the variants of a leg are
interleaved launch block by launch block (one warm launch, then 10 timed between HIP events on the launch stream) with
their order rotated from round to round, so buffer placement, box state and position in the round are shared.
    python scripts/decoded_reveal_inproc.py [rounds]
Legs:
    all consistent     1000 x 1M from 26 and from 17 clerks, verdict == wrong == NULL: sda_packed_reveal_decoded_dev
                       against sda_packed_reveal_checked_dev on the same buffers.  PASS: the decoded reveal's median is
                       within the checked reveal's own spread (max - min of its block means) of the checked reveal's.
    one wrong row      100 x 1M from 26 clerks, clerk 5's row replaced by clerk 6's: the same two calls.  PASS: the
                       decoded reveal is not slower than the checked reveal by more than the checked reveal's spread.
    two, five wrong    100 x 1M from 26 clerks, rows 5 and 20, then 2, 5, 9, 17 and 20 replaced: the decoded reveal,
                       and the CANONICAL reveal of the same shares; recorded only, as ratios.
Every timed call is asserted to return the right counts and, once per variant, the fault-free secrets.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402
from sda_amd import engine as E  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
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
    s64 = sh26 if cnt == n else sh26[:, :cnt, :].contiguous()
    inputs[cnt] = (list(range(cnt)), s64, s64.to(torch.int32))
torch.cuda.synchronize()


def call(kind, width):
    if kind == "decoded":
        fn = eng.packed_reveal_decoded32_dev if width == 32 else eng.packed_reveal_decoded_dev
        return lambda idx, nv, buf: fn(sch, D, idx, nv, buf.data_ptr(), rev.data_ptr(), None, None, st)
    fn = eng.packed_reveal_checked32_dev if width == 32 else eng.packed_reveal_checked_dev
    return lambda idx, nv, buf: fn(sch, D, idx, nv, buf.data_ptr(), rev.data_ptr(), None, st)


def interleave(title, legs, make):
    """legs: keys; make(kind, leg) -> callable.  Prints each block, then per leg the medians, the comparison leg's
    spread and PASS / FAIL: decoded not slower than checked by more than checked's spread."""
    kinds = ("decoded", "checked")
    runs = {(kind, leg): make(kind, leg) for leg in legs for kind in kinds}
    res = {nm: [] for nm in runs}
    for r in range(rounds):
        for leg in legs:
            for i in range(len(kinds)):
                kind = kinds[(i + r) % len(kinds)]
                rev.zero_()
                ms = timed(runs[(kind, leg)])
                res[(kind, leg)].append(ms)
                if r == 0:
                    nv = leg[2]
                    assert torch.equal(rev[:nv], sec[:nv]), (kind, leg)
                print(f"{title} round {r} {kind:8s} {leg}: {ms:.4f} ms", flush=True)
    out = {}
    for leg in legs:
        d, c = res[("decoded", leg)], res[("checked", leg)]
        spread = max(c) - min(c)
        ok = med(d) - med(c) <= spread
        print(f"{title} {leg}: decoded median {med(d):.4f} ms (min {min(d):.4f}, max {max(d):.4f}); checked median "
              f"{med(c):.4f} ms (min {min(c):.4f}, max {max(c):.4f}, spread {spread:.4f}); decoded / checked = "
              f"{med(d) / med(c):.3f}; decoded - checked = {med(d) - med(c):+.4f} ms vs spread {spread:.4f} ms: "
              f"{'PASS' if ok else 'FAIL'}")
        out[leg] = (med(d), med(c))
    return out


# ---- all consistent ----
def consistent(kind, leg):
    width, cnt, nv = leg
    idx, s64, s32 = inputs[cnt]
    buf = s32 if width == 32 else s64
    fn = call(kind, width)

    def run():
        got = fn(idx, nv, buf)
        assert got.bad_batches == 0 and got.redundancy == cnt - (k + t), got
    return run


interleave("all consistent", [(width, cnt, V) for cnt in (26, 17) for width in (64, 32)], consistent)
print(f"record: {eng.packed_decode_last_launch()}")

# ---- wrong rows: 100 vectors of the job above ----
Vb = 100
idx26, s64, _ = inputs[26]


def wrong_rows(rows):
    bad = s64[:Vb].clone()
    for j in rows:
        bad[:, j, :] = s64[:Vb, (j + 1) % n, :]
    torch.cuda.synchronize()
    return bad, bad.to(torch.int32)


one = wrong_rows([5])


def one_row(kind, leg):
    width = leg[0]
    buf = one[1] if width == 32 else one[0]
    fn = call(kind, width)

    def run():
        got = fn(idx26, Vb, buf)
        assert got.bad_batches == Vb * B and got.blame[5] == Vb * B and sum(got.blame) == Vb * B, got
    return run


base = interleave("one wrong row", [(64, 26, Vb), (32, 26, Vb)], one_row)
print(f"record: {eng.packed_decode_last_launch()}")

for rows in ([5, 20], [2, 5, 9, 17, 20]):
    bad = wrong_rows(rows)
    for width in (64, 32):
        buf = bad[1] if width == 32 else bad[0]
        fn = call("decoded", width)
        rec = eng.packed_reconstruct32_dev if width == 32 else eng.packed_reconstruct_dev

        def run():
            got = fn(idx26, Vb, buf)
            assert got.bad_batches == Vb * B and got.undecoded == 0, got
            assert all(got.blame[j] == (Vb * B if j in rows else 0) for j in range(n)), got

        rev.zero_()
        ms = [timed(run) for _ in range(3)]
        assert torch.equal(rev[:Vb], sec[:Vb])
        plain = [timed(lambda: rec(sch, D, idx26, Vb, buf.data_ptr(), rev.data_ptr(), E.REVEAL_CANONICAL, st))
                 for _ in range(3)]
        d1 = base[(width, 26, Vb)][0]
        print(f"{len(rows)} wrong rows i{width} (26 clerks, {Vb} x 1M = {Vb * B} batches, all corrected): median "
              f"{med(ms):.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}); / one wrong row = {med(ms) / d1:.3f}; "
              f"canonical reveal of the same shares {med(plain):.3f} ms, decoded / reveal = {med(ms) / med(plain):.3f}; "
              f"record {eng.packed_decode_last_launch()}")
    del bad
