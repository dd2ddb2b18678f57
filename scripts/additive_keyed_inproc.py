"""In-process measurement of Additive share generation with in-kernel draws (sda_additive_generate_keyed_dev).  One
process, one set of buffers, HIP events on the launch stream for the device legs, the host clock around the
synchronous host call; the legs of a shape are interleaved block by block over several rounds, each block one
warm-up call and `reps` timed ones.
    python scripts/additive_keyed_inproc.py [rounds] [out_file] [parent_lib]

[kernel] per shape (D, n) at m = 2147482801:
  (a) the two-kernel sequence: sda_draws_dev of D (n - 1) draws, then sda_additive_generate_dev reading them;
  (b) sda_additive_generate_keyed_dev (i64 rows);
  (c) sda_additive_generate_keyed32_dev (int32 rows);
  (d) sda_draws_dev alone for the same number of draws -- the VALU yardstick (same ChaCha blocks);
  (e) sda_synth_fill_dev of (b)'s output bytes, 8 D n -- the write yardstick.
Reported: every median and spread, (b) / (a), (c) / (b), (b) / max((d), (e)), and the condition for the host call:
(b) <= (a) + (a)'s own round-to-round spread (max - min) at every shape.
[host] sda_share_generate_keyed on Additive(3, m) at D = 10M; with parent_lib (a build of the parent commit's
library) the same call through it, interleaved, and the two results compared.
SDA_INPROC_SCALE divides every D (rehearsal).
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
parent_lib = sys.argv[3] if len(sys.argv) > 3 else None
scale = int(os.environ.get("SDA_INPROC_SCALE", 1))
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


def timed_host(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def med(v):
    s = sorted(v)
    return s[len(s) // 2]


def report(tag, name, v, extra=""):
    s = sorted(v)
    say(f"[{tag}] {name:<34} median {med(v):.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
        f"spread {100 * (s[-1] - s[0]) / med(v):.2f} %{extra}")
    say(f"[{tag}] {name:<34} per-call ms by round: " + " ".join(f"{x:.4f}" for x in v))


torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream
M = 2147482801
KEY = np.array([0x5DA0 + i for i in range(8)], np.uint32)
say(f"additive_keyed_inproc: m = {M}; rounds={rounds} (1 warm-up + 5 timed calls per block)")

# ---- the kernel ----
all_ok = True
for D, n in ((10_000_000 // scale, 3), (10_000_000 // scale, 2), (1_000_000 // scale, 26)):
    tag = f"kernel D={D} n={n}"
    nd = D * (n - 1)
    secrets = torch.as_tensor(np.random.default_rng(D + n).integers(0, M, size=D, dtype=np.int64)).cuda()
    draws = torch.empty(nd, dtype=torch.int64, device="cuda")
    out_a = torch.empty((n, D), dtype=torch.int64, device="cuda")
    out_b = torch.empty((n, D), dtype=torch.int64, device="cuda")
    out_c = torch.empty((n, D), dtype=torch.int32, device="cuda")

    def two_kernels():
        eng.draws_dev(KEY, 0, 0, nd, M, draws.data_ptr(), st)
        eng.additive_generate_dev(M, n, secrets.data_ptr(), D, draws.data_ptr(), out_a.data_ptr(), st)

    legs = {
        "(a) draws_dev + additive_generate_dev": two_kernels,
        "(b) additive_generate_keyed_dev": lambda: eng.additive_generate_keyed_dev(
            M, n, secrets.data_ptr(), D, KEY, 0, out_b.data_ptr(), D, stream=st),
        "(c) additive_generate_keyed32_dev": lambda: eng.additive_generate_keyed32_dev(
            M, n, secrets.data_ptr(), D, KEY, 0, out_c.data_ptr(), D, stream=st),
        "(d) draws_dev alone": lambda: eng.draws_dev(KEY, 0, 0, nd, M, draws.data_ptr(), st),
        "(e) synth_fill_dev, 8 D n bytes": lambda: eng.synth_fill_dev(out_a.data_ptr(), n, D, 0x5DA, 0, M, st),
    }
    legs["(b) additive_generate_keyed_dev"]()
    legs["(c) additive_generate_keyed32_dev"]()
    two_kernels()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_a, out_b)) and bool(torch.equal(out_b.to(torch.int32), out_c))
    say(f"[{tag}] {nd} draws; (a), (b) and (int32) (c) give the same shares: {same}")
    assert same
    res = {name: [] for name in legs}
    for r in range(rounds):
        for name, fn in legs.items():
            res[name].append(timed_dev(fn, 5))
    t = {name[:3]: med(v) for name, v in res.items()}
    model = {"(a)": 8 * D * (3 * n - 1), "(b)": 8 * D * (n + 1), "(c)": 8 * D + 4 * D * n, "(d)": 8 * nd,
             "(e)": 8 * D * n}
    for name, v in res.items():
        b = model[name[:3]]
        report(tag, name, v, f"  {b / 1e6:.0f} MB by the byte model, {b / (med(v) * 1e-3) / 1e12:.3f} TB/s")
    sa = sorted(res["(a) draws_dev + additive_generate_dev"])
    spread_a = sa[-1] - sa[0]
    ok = t["(b)"] <= t["(a)"] + spread_a
    all_ok = all_ok and ok
    yard = max(t["(d)"], t["(e)"])
    say(f"[{tag}] (b)/(a) = {t['(b)'] / t['(a)']:.3f}  (c)/(b) = {t['(c)'] / t['(b)']:.3f}  "
        f"(b)/max((d),(e)) = {t['(b)'] / yard:.3f} ({'VALU' if t['(d)'] > t['(e)'] else 'write'} yardstick)")
    say(f"[{tag}] host-call condition (b) <= (a) + spread(a) = {t['(a)']:.4f} + {spread_a:.4f} ms: "
        f"{'PASS' if ok else 'FAIL'}")
    del secrets, draws, out_a, out_b, out_c
say(f"[kernel] host-call condition at all three shapes: {'PASS' if all_ok else 'FAIL'}")

# ---- the host call ----
PD = 10_000_000 // scale
sch = S.Additive(3, M)
sc = sch.c()
hsecrets = np.random.default_rng(2).integers(0, M, size=PD, dtype=np.int64)
i64p, u32p = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)


def ptr(a, ty=i64p):
    return a.ctypes.data_as(ty)


def keyed_call(lib, h, o):
    def call():
        assert lib.sda_share_generate_keyed(h, C.byref(sc), ptr(hsecrets), PD, ptr(KEY, u32p), 1, ptr(o), o.size) == 0
    return call


outs = {"share_generate_keyed": np.zeros(3 * PD, np.int64)}
hlegs = {"share_generate_keyed": keyed_call(eng.lib, eng.h, outs["share_generate_keyed"])}
ph = None
if parent_lib:
    # the parent build has none of the new symbols: bind the two calls this needs by hand
    plib = C.CDLL(parent_lib)
    plib.sda_engine_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    plib.sda_engine_destroy.argtypes = [C.c_void_p]
    plib.sda_engine_destroy.restype = None
    plib.sda_share_generate_keyed.argtypes = [C.c_void_p, C.POINTER(S.SharingSchemeC), i64p, C.c_uint64, u32p,
                                              C.c_uint32, i64p, C.c_uint64]
    ph = C.c_void_p()
    assert plib.sda_engine_create(0, C.byref(ph)) == 0
    outs["share_generate_keyed (parent)"] = np.zeros(3 * PD, np.int64)
    hlegs["share_generate_keyed (parent)"] = keyed_call(plib, ph, outs["share_generate_keyed (parent)"])
for fn in hlegs.values():
    fn()
if parent_lib:
    same = bool(np.array_equal(*outs.values()))
    say(f"[host] Additive(3, m), D={PD}: this build's shares == the parent build's: {same}")
    assert same
hres = {name: [] for name in hlegs}
for r in range(rounds):
    for name, fn in hlegs.items():
        hres[name].append(timed_host(fn, 3))
for name in hlegs:
    report("host", name, hres[name])
if parent_lib:
    say(f"[host] this build / parent = "
        f"{med(hres['share_generate_keyed']) / med(hres['share_generate_keyed (parent)']):.3f}")
    plib.sda_engine_destroy(ph)
eng.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if all_ok else 1)
