"""In-process measurement of the device-side draws (sda_draws_dev, sda_share_generate_keyed).  One process, one set
of buffers, HIP events on the launch stream for the device legs, the host clock around the synchronous host calls;
the legs of a section are interleaved block by block over several rounds, each block one warm-up call and `reps`
timed ones.
    python scripts/draws_inproc.py [rounds] [out_file]

[kernel] sda_draws_dev for configs[2]'s 1000 x 125,000 x 7 = 8.75e8 draws at bound = p - 1, beside two yardsticks:
  (a) sda_chacha_mask_combine_dev at 256 seeds x 1M: the same VALU work per ChaCha block without a store -- its
      block rate gives the time the draws' blocks would take at that rate;
  (b) sda_synth_fill_dev of the same element count: the 8-byte write rate.
The expectation is the larger of blocks / (a) and (b); the ratio measured / expected is reported, no threshold (the
mask combine amortises its key set-up over seeds).
[host] at configs[2]'s scheme, D = 10M: sda_share_generate_keyed against the unchanged sda_share_generate fed with
pre-drawn draws (host RNG time excluded, which favours the old path).  The keyed call copies 70 MB less to the
device; the gate is keyed <= 1.03 x plain (medians), and the two results must be identical.
SDA_INPROC_DRAWS / SDA_INPROC_DIM / SDA_INPROC_PDIM shrink the job (rehearsal).
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
    say(f"[{tag}] {name:<28} median {med(v):.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
        f"spread {100 * (s[-1] - s[0]) / med(v):.2f} %{extra}")
    say(f"[{tag}] {name:<28} per-call ms by round: " + " ".join(f"{x:.4f}" for x in v))


torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream
sch = S.CONFIG_PACKED
p, k, t, n = sch.prime_modulus, sch.secret_count, sch.privacy_threshold(), sch.share_count
KEY = np.array([0x5DA0 + i for i in range(8)], np.uint32)

# ---- the kernel ----
ND = int(os.environ.get("SDA_INPROC_DRAWS", 1000 * 125_000 * 7))
MD = int(os.environ.get("SDA_INPROC_DIM", 1_000_000))
NS = 256
buf = torch.empty(ND, dtype=torch.int64, device="cuda")
acc = torch.empty(MD, dtype=torch.int64, device="cuda")
seeds = torch.as_tensor(np.random.default_rng(1).integers(0, 1 << 32, size=(NS, 4), dtype=np.uint64)
                        .astype(np.uint32).view(np.int32)).cuda()
rows = 1000 if ND % 1000 == 0 else 1
legs = {
    "draws_dev": lambda: eng.draws_dev(KEY, 0, 0, ND, p - 1, buf.data_ptr(), st),
    "chacha_mask_combine_dev (a)": lambda: eng.chacha_mask_combine_dev(p, MD, seeds.data_ptr(), 4, NS, acc.data_ptr(), st),
    "synth_fill_dev (b)": lambda: eng.synth_fill_dev(buf.data_ptr(), rows, ND // rows, 0x5DA, 0, p - 1, st),
}
say(f"draws_inproc: {ND} draws at bound p - 1 = {p - 1}; mask combine {NS} seeds x {MD}; rounds={rounds} "
    f"(1 warm-up + 5 timed calls per block)")
res = {name: [] for name in legs}
for r in range(rounds):
    for name, fn in legs.items():
        res[name].append(timed_dev(fn, 5))
blocks = (ND + 7) // 8
mc_blocks = NS * ((MD + 7) // 8)
t_d, t_a, t_b = med(res["draws_dev"]), med(res["chacha_mask_combine_dev (a)"]), med(res["synth_fill_dev (b)"])
rate_a = mc_blocks / (t_a * 1e-3)
by_a = blocks / rate_a * 1e3
report("kernel", "draws_dev", res["draws_dev"],
       f"  {ND / (t_d * 1e-3) / 1e9:.1f} G draws/s  {8.0 * ND / (t_d * 1e-3) / 1e12:.3f} TB/s written")
report("kernel", "chacha_mask_combine_dev (a)", res["chacha_mask_combine_dev (a)"],
       f"  {rate_a / 1e9:.2f} G blocks/s -> {blocks} blocks in {by_a:.4f} ms")
report("kernel", "synth_fill_dev (b)", res["synth_fill_dev (b)"], f"  {8.0 * ND / (t_b * 1e-3) / 1e12:.3f} TB/s written")
expect = max(by_a, t_b)
say(f"[kernel] expectation max(blocks / (a), (b)) = {expect:.4f} ms ({'VALU' if by_a > t_b else 'store'} side); "
    f"measured / expected = {t_d / expect:.3f}")
del buf, acc

# ---- the host call ----
PD = int(os.environ.get("SDA_INPROC_PDIM", 10_000_000))
B = (PD + k - 1) // k
secrets = np.random.default_rng(2).integers(0, p, size=PD, dtype=np.int64)
draws = eng.draws(KEY, 1, 0, B * t, p - 1)
out = {"share_generate (pre-drawn)": np.zeros(n * B, np.int64), "share_generate_keyed": np.zeros(n * B, np.int64)}
i64p, u32p = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
sc = sch.c()


def ptr(a, ty=i64p):
    return a.ctypes.data_as(ty)


def plain():
    o = out["share_generate (pre-drawn)"]
    assert eng.lib.sda_share_generate(eng.h, C.byref(sc), ptr(secrets), PD, ptr(draws), draws.size, ptr(o), o.size) == 0


def keyed():
    o = out["share_generate_keyed"]
    assert eng.lib.sda_share_generate_keyed(eng.h, C.byref(sc), ptr(secrets), PD, ptr(KEY, u32p), 1, ptr(o), o.size) == 0


hlegs = {"share_generate (pre-drawn)": plain, "share_generate_keyed": keyed}
for fn in hlegs.values():
    fn()
same = bool(np.array_equal(*out.values()))
say(f"[host] k={k} t={t} n={n}, D={PD} B={B}: {B * t} draws ({8 * B * t / 1e6:.1f} MB the keyed call does not copy); "
    f"keyed shares == shares from sda_draws of the same key: {same}")
assert same
hres = {name: [] for name in hlegs}
for r in range(rounds):
    for name, fn in hlegs.items():
        hres[name].append(timed_host(fn, 3))
for name in hlegs:
    report("host", name, hres[name])
ratio = med(hres["share_generate_keyed"]) / med(hres["share_generate (pre-drawn)"])
say(f"[host] keyed / pre-drawn = {ratio:.3f} (gate: <= 1.03): {'PASS' if ratio <= 1.03 else 'FAIL'}")
eng.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ratio <= 1.03 else 1)
