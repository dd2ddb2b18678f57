"""In-process A/B of int32 share rows against i64 ones in packed-Shamir share generation and reveal
(sda_packed_generate32_dev / sda_packed_reconstruct32_dev against their i64 twins), at the shape the bench's
share-gen and reveal legs use: PackedShamir k=8 t=7 n=26 (configs[2]), 1000 vectors x 1M secrets, reveal from 15
clerks.  One process, one set of buffers; the legs are interleaved launch block by launch block over several
rounds, each block one warm-up launch and 10 timed ones between HIP events on the launch stream, so buffer
placement, clocks and box state are shared by every leg.  The yardstick of an int32 leg is the i64 leg of the
same round.
    python scripts/packed32_inproc.py [rounds] [out_file]
Legs: share-gen {canonical, exact} x {i64, int32}; reveal {canonical, exact} x {i64, int32}.
SDA_INPROC_ALT_LIB=<another build of libsda_engine.so> adds the share-gen and reveal legs from that library, loaded into
the same process (the A/B of two builds, e.g. against the parent commit's), and prints per leg whether this build's
median is within the other's median plus the other's own spread (max - min) in this run.  The two builds' legs trade
places every other round: a leg's place in the round is worth up to 1 % (profiles/gen_launch/ab_parent.txt).
Per leg: per-launch ms of every round, median, spread, algorithmic bytes, fraction of the 8 TB/s HBM peak, and for
the int32 legs the ratio to the i64 median next to the byte ratio.  Checks the int32 outputs against the i64 ones
(bit equality after widening).
SDA_INPROC_VECS / SDA_INPROC_DIM shrink the job (rehearsal).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402
from sda_amd import engine as E  # noqa: E402

PEAK = 8.0e12
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream
sch = S.CONFIG_PACKED
p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
V = int(os.environ.get("SDA_INPROC_VECS", 1000))
D = int(os.environ.get("SDA_INPROC_DIM", 1_000_000))
B = D // k
assert D % k == 0 and B % 4 == 0
sec = torch.empty((V, D), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(sec.data_ptr(), V, D, 0x5DB2, 0, p, st)
drw = torch.empty((V, B, t), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(drw.data_ptr(), V * B, t, 0x5DB3, 0, p - 1, st)
sh64 = torch.empty((V, n, B), dtype=torch.int64, device="cuda")
sh32 = torch.empty((V, n, B), dtype=torch.int32, device="cuda")
idx = list(range(n - (t + k), n))
m = len(idx)
sub64 = torch.empty((V, m, B), dtype=torch.int64, device="cuda")
sub32 = torch.empty((V, m, B), dtype=torch.int32, device="cuda")
rev = torch.empty((V, D), dtype=torch.int64, device="cuda")
MODES = (("canonical", E.REVEAL_CANONICAL), ("exact", E.REVEAL_EXACT))


ALT = os.environ.get("SDA_INPROC_ALT_LIB")
alt = Engine(0, lib_path=ALT) if ALT else None      # a second build of the library in this process


def gen64(mode, e=eng):
    e.packed_generate_mode_dev(sch, sec.data_ptr(), D, V, drw.data_ptr(), sh64.data_ptr(), mode, st)


def gen32(mode, e=eng):
    e.packed_generate32_dev(sch, sec.data_ptr(), D, V, drw.data_ptr(), sh32.data_ptr(), mode, st)


def rev64(mode, e=eng):
    e.packed_reconstruct_dev(sch, D, idx, V, sub64.data_ptr(), rev.data_ptr(), mode, st)


def rev32(mode, e=eng):
    e.packed_reconstruct32_dev(sch, D, idx, V, sub32.data_ptr(), rev.data_ptr(), mode, st)


gen_in = 8.0 * V * (D + B * t)
bytes_of = {"gen64": gen_in + 8.0 * V * n * B, "gen32": gen_in + 4.0 * V * n * B,
            "rev64": 8.0 * V * (m * B + D), "rev32": 4.0 * V * m * B + 8.0 * V * D}
# (name, launcher, byte key, twin)
LEGS = [("gen i64", gen64, "gen64", None),
        ("gen int32", gen32, "gen32", "gen i64")]
if alt:
    LEGS += [("gen i64 alt lib", lambda mode: gen64(mode, alt), "gen64", None),
             ("gen int32 alt lib", lambda mode: gen32(mode, alt), "gen32", "gen i64 alt lib")]
LEGS += [("reveal i64", rev64, "rev64", None),
         ("reveal int32", rev32, "rev32", "reveal i64")]
if alt:
    LEGS += [("reveal i64 alt lib", lambda mode: rev64(mode, alt), "rev64", None),
             ("reveal int32 alt lib", lambda mode: rev32(mode, alt), "rev32", "reveal i64 alt lib")]
BY_NAME = {leg[0]: leg for leg in LEGS}


def other_build(name):
    """the same leg from the other library; the leg itself where there is none"""
    o = name[:-len(" alt lib")] if name.endswith(" alt lib") else name + " alt lib"
    return o if o in BY_NAME else name


say(f"packed32_inproc: k={k} t={t} n={n} p={p}  V={V} D={D} B={B}  reveal from {m} clerks  rounds={rounds} "
    f"(1 warm-up + 10 timed launches per block)"
    + (f"  alt lib {os.path.basename(os.path.dirname(ALT))}/{os.path.basename(ALT)}" if alt else ""))
for mname, mode in MODES:
    # correctness first: the int32 outputs against the i64 ones (the other build's too, against this build's i64)
    gen64(mode)
    checks = []
    for e in (alt, eng) if alt else (eng,):
        sh32.fill_(0x5A5A5A5A)
        gen32(mode, e)
        torch.cuda.synchronize()
        checks.append(all(torch.equal(sh32[v0:v0 + 50].to(torch.int64), sh64[v0:v0 + 50]) for v0 in range(0, V, 50)))
    fix_gen = eng.packed_fixup_count()
    sub64.copy_(sh64[:, idx, :])
    sub32.copy_(sh32[:, idx, :])
    rev64(mode)
    ref = rev.clone()
    for fn, e in ((rev64, alt), (rev32, alt)) if alt else ():      # the other build's reveals, against this build's i64
        rev.fill_(0x5A5A5A5A)
        fn(mode, e)
        torch.cuda.synchronize()
        checks.append(torch.equal(rev, ref))
    rev.fill_(0x5A5A5A5A)
    rev32(mode)
    fix_rev = eng.packed_fixup_count()
    torch.cuda.synchronize()
    checks.append(torch.equal(rev, ref))
    checks.append(torch.equal(torch.remainder(rev, p), sec))
    del ref
    say(f"[{mname}] int32 == i64: gen {checks[1 if alt else 0]}, gen alt lib {checks[0] if alt else 'not given'}, "
        f"reveal {checks[-2]}, reveal alt lib (i64, int32) {tuple(checks[2:4]) if alt else 'not given'}, "
        f"reveals the secrets {checks[-1]}; fix-up batches gen32 {fix_gen} reveal32 {fix_rev}")
    assert all(checks)
    res = {leg[0]: [] for leg in LEGS}
    for r in range(rounds):
        for leg in LEGS:
            # the two builds' legs trade places every other round, so neither always follows the same leg
            name, fn, _, _ = BY_NAME[other_build(leg[0])] if r % 2 else leg
            fn(mode)                                                                    # warm
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn(mode)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / 10)
    med = {}
    for name, _, key, twin in LEGS:
        s = sorted(res[name])
        med[name] = s[len(s) // 2]
        nb = bytes_of[key]
        line = (f"[{mname}] {name:<24} median {med[name]:.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
                f"spread {100 * (s[-1] - s[0]) / med[name]:.2f} %  bytes {nb / 1e9:.3f} GB ({nb / V / B:.0f} B/batch)  "
                f"{nb / (med[name] * 1e-3) / PEAK:.3f} of 8 TB/s")
        if twin:
            line += (f"  time / i64 {med[name] / med[twin]:.3f}  (byte ratio "
                     f"{nb / bytes_of[key.replace('32', '64')]:.3f})")
        say(line)
        say(f"[{mname}] {name:<24} per-launch ms by round: " + " ".join(f"{x:.4f}" for x in res[name]))
    for name in ("gen i64", "gen int32", "reveal i64", "reveal int32") if alt else ():
        o = res[name + " alt lib"]
        bound = med[name + " alt lib"] + max(o) - min(o)
        say(f"[{mname}] {name:<24} median {med[name]:.4f} ms against the alt lib's {med[name + ' alt lib']:.4f} + "
            f"spread {max(o) - min(o):.4f} = {bound:.4f}: {'PASS' if med[name] <= bound else 'FAIL'}")
eng.close()
if alt:
    alt.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
