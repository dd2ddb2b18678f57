"""In-process A/B of the int32 payload encoder against the i64 one (sda_varint_encode32_dev against
sda_varint_encode_dev), on the same values: a 1000 x 1M i64 matrix from sda_synth_fill_dev, uniform in (-p, p) for
configs[2]'s prime, narrowed once with sda_narrow32_dev.  One process, one set of buffers; the two launches are
interleaved block by block over several rounds, each block one warm-up launch and 5 timed ones between HIP events on
the launch stream (each launch ends in the entry point's wait for the row sizes, as a caller sees it).  The yardstick
of the int32 launch is the i64 launch of the same round.
    python scripts/encode32_inproc.py [rounds] [out_file]
Prints the median time per launch of each, their ratio next to the byte model's (4 + 4 + payload against
8 + 8 + payload bytes per value: the size pass and the write pass each read every value), and the payload bytes,
which must be equal.  Then the same for one sda_participant_share_dev against sda_participant_share32_dev
(ChaCha masking, configs[2]'s scheme, with a payload) at configs[4]'s dimension, 10M.
SDA_INPROC_ALT_LIB=<another build of libsda_engine.so> adds both encode legs from that library, loaded into the same
process (Engine(lib_path=...)): the A/B of the int32 chunk size (EXTRA=-DSDA_ENC32_CHUNK=4096), or of this tree
against its parent's library, each encoder with its twin of the other build as the yardstick;
SDA_INPROC_ALT_NOTE is printed next to its file name to say what that build is.
SDA_INPROC_ROWS / SDA_INPROC_DIM / SDA_INPROC_PDIM shrink the job (rehearsal); SDA_INPROC_PDIM=0 leaves the
participant pipeline out.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402

PEAK = 8.0e12
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    fn()                                                                                # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def report(tag, res, legs, bytes_of, unit):
    med = {}
    for name, twin in legs:
        s = sorted(res[name])
        med[name] = s[len(s) // 2]
        nb = bytes_of[name]
        line = (f"[{tag}] {name:<22} median {med[name]:.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
                f"spread {100 * (s[-1] - s[0]) / med[name]:.2f} %  bytes {nb / 1e9:.3f} GB ({nb / unit:.2f} B/value)  "
                f"{nb / (med[name] * 1e-3) / PEAK:.3f} of 8 TB/s")
        if twin:
            line += f"  time / {twin} {med[name] / med[twin]:.3f}  (byte ratio {nb / bytes_of[twin]:.3f})"
        say(line)
        say(f"[{tag}] {name:<22} per-launch ms by round: " + " ".join(f"{x:.4f}" for x in res[name]))


torch.cuda.init()
eng = Engine(0)
ALT = os.environ.get("SDA_INPROC_ALT_LIB")
alt = Engine(0, lib_path=ALT) if ALT else None      # a second build of the library in this process
st = torch.cuda.current_stream().cuda_stream
sch = S.CONFIG_PACKED
p = sch.prime_modulus
N = int(os.environ.get("SDA_INPROC_ROWS", 1000))
D = int(os.environ.get("SDA_INPROC_DIM", 1_000_000))

# ---- the encoders ----
x64 = torch.empty((N, D), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(x64.data_ptr(), N, D, 0x5DA + 6, -(p - 1), p, st)
x32 = torch.empty((N, D), dtype=torch.int32, device="cuda")
flag = torch.zeros(1, dtype=torch.int64, device="cuda")
eng.narrow32_dev(x64.data_ptr(), N, D, D, x32.data_ptr(), D, flag.data_ptr(), st)
torch.cuda.synchronize()
assert int(flag.item()) == 0
cap = N * D * 5 + 32
LEGS = [("encode i64", None), ("encode int32", "encode i64")]
if alt:
    LEGS += [("encode i64 alt lib", "encode i64"), ("encode int32 alt lib", "encode int32")]
bufs = {name: torch.zeros(cap, dtype=torch.uint8, device="cuda") for name, _ in LEGS}
sizes = {}


def enc(name):
    b = bufs[name]
    e = alt if name.endswith("alt lib") else eng
    if name.startswith("encode i64"):
        sizes[name] = e.varint_encode_dev(x64.data_ptr(), N, D, D, b.data_ptr(), cap, st)
    else:
        sizes[name] = e.varint_encode32_dev(x32.data_ptr(), N, D, D, b.data_ptr(), cap, st)


say(f"encode32_inproc: {N} x {D} values uniform in (-p, p), p={p}  rounds={rounds} (1 warm-up + 5 timed launches "
    f"per block)" + (f"  alt lib {os.path.basename(ALT)}: {os.environ.get('SDA_INPROC_ALT_NOTE', 'another build')}"
                     if alt else ""))
for name, _ in LEGS:
    enc(name)
torch.cuda.synchronize()
total = int(sizes["encode i64"].sum())
same = {name: bool(np.array_equal(sizes[name], sizes["encode i64"])) and
        all(torch.equal(bufs[name][a:min(a + (1 << 28), total)], bufs["encode i64"][a:min(a + (1 << 28), total)])
            for a in range(0, total, 1 << 28)) for name, _ in LEGS[1:]}
say(f"[encode] payload bytes: " + "  ".join(f"{name} {int(sizes[name].sum())}" for name, _ in LEGS) +
    f"  ({total / N / D:.3f} B/value); payload == i64 payload: {same}")
assert all(same.values())
res = {name: [] for name, _ in LEGS}
for r in range(rounds):
    for name, _ in LEGS:
        res[name].append(timed(lambda: enc(name), 5))
nv = float(N) * D
bytes_of = {name: (16.0 if name.startswith("encode i64") else 8.0) * nv + total for name, _ in LEGS}
report("encode", res, LEGS, bytes_of, nv)
del x64, x32, bufs


def finish():
    eng.close()
    if alt:
        alt.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


# ---- the participant pipeline ----
PD = int(os.environ.get("SDA_INPROC_PDIM", 10_000_000))
if PD == 0:
    finish()
    sys.exit(0)
ms = S.ChaChaMasking(p, PD, 128)
k, t, n = sch.secret_count, sch.privacy_threshold(), sch.share_count
B = (PD + k - 1) // k
sec = torch.empty(PD, dtype=torch.int64, device="cuda")
eng.synth_fill_dev(sec.data_ptr(), 1, PD, 0x5DB2, 0, p, st)
drw = torch.empty(B * t, dtype=torch.int64, device="cuda")
eng.synth_fill_dev(drw.data_ptr(), B, t, 0x5DB3, 0, p - 1, st)
seed = np.array([0x5DA, 7, 11, 13], np.uint32)
sh64 = torch.empty((n, B), dtype=torch.int64, device="cuda")
sh32 = torch.empty((n, B), dtype=torch.int32, device="cuda")
pcap = n * B * 5 + 32
pay = {w: torch.zeros(pcap, dtype=torch.uint8, device="cuda") for w in ("participant i64", "participant int32")}
prb = {}


def part(name):
    if name == "participant i64":
        prb[name] = eng.participant_share_dev(ms, sch, sec.data_ptr(), PD, drw.data_ptr(), sh64.data_ptr(), seed=seed,
                                              payload_ptr=pay[name].data_ptr(), payload_cap=pcap, stream=st)
    else:
        prb[name] = eng.participant_share32_dev(ms, sch, sec.data_ptr(), PD, drw.data_ptr(), sh32.data_ptr(),
                                                seed=seed, payload_ptr=pay[name].data_ptr(), payload_cap=pcap,
                                                stream=st)


PLEGS = [("participant i64", None), ("participant int32", "participant i64")]
for name, _ in PLEGS:
    part(name)
torch.cuda.synchronize()
ptotal = int(prb["participant i64"].sum())
ok = (np.array_equal(prb["participant i64"], prb["participant int32"]) and
      torch.equal(pay["participant i64"][:ptotal], pay["participant int32"][:ptotal]) and
      torch.equal(sh64.to(torch.int32), sh32))
say(f"[participant] ChaCha masking, k={k} t={t} n={n}, D={PD} B={B}: payload bytes i64 {ptotal} int32 "
    f"{int(prb['participant int32'].sum())}; int32 shares and payload == i64: {ok}")
assert ok
pres = {name: [] for name, _ in PLEGS}
for r in range(rounds):
    for name, _ in PLEGS:
        pres[name].append(timed(lambda: part(name), 5))
# secrets in and masked out and in again (8 + 8 + 8), draws, shares written and read twice by the encoder, payload
pin = 24.0 * PD + 8.0 * B * t
pbytes = {"participant i64": pin + 24.0 * n * B + ptotal, "participant int32": pin + 12.0 * n * B + ptotal}
report("participant", pres, PLEGS, pbytes, float(n) * B)
finish()
