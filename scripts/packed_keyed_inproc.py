"""In-process measurement of packed-Shamir share generation with in-kernel draws (sda_packed_generate_keyed_dev and
its int32 form).  One process, one set of buffers, HIP events on the launch stream; the legs of a mode and width
are interleaved block by block over several rounds, each block one warm-up call and `reps` timed ones.
    python scripts/packed_keyed_inproc.py [rounds] [out_file]

Scheme: PackedShamir k=8 t=7 n=26 (configs[2]), 1000 vectors x 1M secrets (SDA_INPROC_VECS / SDA_INPROC_DIM
override), canonical and exact, i64 and int32 shares.  Per (mode, width):
  (a) the staged sequence: sda_draws_dev of V B t draws, then the unkeyed generate reading them;
  (b) the keyed generate: the draws made in the share kernels;
  (c) the unkeyed generate alone on pre-made draws -- the memory yardstick;
  (d) sda_draws_dev alone -- the VALU yardstick (the same ChaCha blocks).
(a) and (b) are compared for equality (shares and fix-up count) before timing.  Reported: every median and spread,
(b) / (a) against the gate 0.97 (the project's rule for keeping a tuning change: a gain larger than the box-to-box
spread), and (b) / max((c), (d)) without a gate.  The exit status is 1 when a leg misses the gate.
SDA_INPROC_ALT_LIB=<another build of libsda_engine.so> adds (b) and (c) from that library, loaded into the same process
(the A/B of two builds, e.g. against the parent commit's), and prints per leg whether this build's median is within
the other's median plus the other's own spread (max - min) in this run.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402
from sda_amd import engine as E  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
REPS = 5
GATE = 0.97
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_dev(fn, reps):
    fn()                                                                                # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    s = sorted(v)
    return s[len(s) // 2]


def report(tag, name, v, extra=""):
    s = sorted(v)
    say(f"[{tag}] {name:<40} median {med(v):.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
        f"spread {100 * (s[-1] - s[0]) / med(v):.2f} %{extra}")
    say(f"[{tag}] {name:<40} per-call ms by round: " + " ".join(f"{x:.4f}" for x in v))


torch.cuda.init()
eng = Engine(0)
ALT = os.environ.get("SDA_INPROC_ALT_LIB")
alt = Engine(0, lib_path=ALT) if ALT else None      # a second build of the library in this process
st = torch.cuda.current_stream().cuda_stream
sch = S.CONFIG_PACKED
p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
V = int(os.environ.get("SDA_INPROC_VECS", 1000))
D = int(os.environ.get("SDA_INPROC_DIM", 1_000_000))
B = D // k
assert D % k == 0 and B % 2 == 0
KEY = np.array([0x5DA0 + i for i in range(8)], np.uint32)
STREAM = 3
nd = V * B * t
sec = torch.empty((V, D), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(sec.data_ptr(), V, D, 0x5DB2, 0, p, st)
drw = torch.empty(nd, dtype=torch.int64, device="cuda")
say(f"packed_keyed_inproc: k={k} t={t} n={n} p={p}  V={V} D={D} B={B}  {nd} draws  rounds={rounds} "
    f"(1 warm-up + {REPS} timed calls per block)")

all_ok = True
for wname, dtype, unkeyed, keyed in (("i64", torch.int64, eng.packed_generate_mode_dev, eng.packed_generate_keyed_dev),
                                     ("int32", torch.int32, eng.packed_generate32_dev,
                                      eng.packed_generate_keyed32_dev)):
    out = torch.empty((V, n, B), dtype=dtype, device="cuda")
    for mname, mode in (("canonical", E.REVEAL_CANONICAL), ("exact", E.REVEAL_EXACT)):
        tag = f"{mname} {wname}"

        def draws_alone():
            eng.draws_dev(KEY, STREAM, 0, nd, p - 1, drw.data_ptr(), st)

        def gen_alone():
            unkeyed(sch, sec.data_ptr(), D, V, drw.data_ptr(), out.data_ptr(), mode, st)

        def staged():
            draws_alone()
            gen_alone()

        def fused():
            keyed(sch, sec.data_ptr(), D, V, KEY, STREAM, out.data_ptr(), mode, stream=st)

        # (a) == (b) first: the shares (in slices of 50 vectors) and the fix-up count
        ref = torch.empty_like(out)
        staged()
        ref.copy_(out)
        fix_a = eng.packed_fixup_count()
        out.fill_(0x5A5A5A5A)
        fused()
        fix_b = eng.packed_fixup_count()
        torch.cuda.synchronize()
        same = all(torch.equal(out[v0:v0 + 50], ref[v0:v0 + 50]) for v0 in range(0, V, 50))
        del ref
        rec = eng.packed_keyed_last_launch()
        say(f"[{tag}] (a) and (b) give the same shares: {same}; fix-up batches (a) {fix_a} (b) {fix_b}; "
            f"keyed record {rec}")
        assert same and fix_a == fix_b and rec == (1, 0)
        legs = {"(a) draws_dev + unkeyed generate": staged, "(b) keyed generate": fused,
                "(c) unkeyed generate, pre-made draws": gen_alone, "(d) draws_dev alone": draws_alone}
        if alt:
            a_unkeyed, a_keyed = getattr(alt, unkeyed.__name__), getattr(alt, keyed.__name__)
            legs["(b) keyed generate, alt lib"] = lambda: a_keyed(sch, sec.data_ptr(), D, V, KEY, STREAM,
                                                                  out.data_ptr(), mode, stream=st)
            legs["(c) unkeyed generate, alt lib"] = lambda: a_unkeyed(sch, sec.data_ptr(), D, V, drw.data_ptr(),
                                                                      out.data_ptr(), mode, st)
        res = {name: [] for name in legs}
        # the two builds' legs trade places every other round, so neither always follows the same leg
        twin = {name: next((o for o in legs if o != name and o[:3] == name[:3]), name) for name in legs}
        for r in range(rounds):
            for name in legs:
                name = twin[name] if r % 2 else name
                res[name].append(timed_dev(legs[name], REPS))
        tm = {name[:3]: med(v) for name, v in res.items() if not name.endswith("alt lib")}
        width = out.element_size()
        model = {"(a)": 8.0 * V * (D + 2 * B * t) + width * V * n * B, "(b)": 8.0 * V * D + width * V * n * B,
                 "(c)": 8.0 * V * (D + B * t) + width * V * n * B, "(d)": 8.0 * nd}
        for name, v in res.items():
            b = model[name[:3]]
            report(tag, name, v, f"  {b / 1e9:.1f} GB by the byte model, {b / (med(v) * 1e-3) / 1e12:.3f} TB/s")
        ratio = tm["(b)"] / tm["(a)"]
        yard = max(tm["(c)"], tm["(d)"])
        ok = ratio <= GATE
        all_ok = all_ok and ok
        say(f"[{tag}] (b)/(a) = {ratio:.3f} (gate {GATE}: {'PASS' if ok else 'FAIL'})  "
            f"(b)/max((c),(d)) = {tm['(b)'] / yard:.3f} ({'memory (c)' if tm['(c)'] > tm['(d)'] else 'VALU (d)'} "
            f"yardstick)  (c)+(d) = {tm['(c)'] + tm['(d)']:.4f} ms")
        for name in [name for name in res if name.endswith("alt lib")]:
            o = res[name]
            bound = med(o) + max(o) - min(o)
            say(f"[{tag}] {name[:3]} median {tm[name[:3]]:.4f} ms against the alt lib's {med(o):.4f} + spread "
                f"{max(o) - min(o):.4f} = {bound:.4f}: {'PASS' if tm[name[:3]] <= bound else 'FAIL'}")
    del out
say(f"gate (b) <= {GATE} (a) in all four legs: {'PASS' if all_ok else 'FAIL'}")
eng.close()
if alt:
    alt.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if all_ok else 1)
