"""In-process timing of the clerk job (sda_clerk_job_dev) against the calls it replaces, on the same payloads:
N x D field shares uniform in (-p, p) for configs[2]'s prime from sda_synth_fill_dev, encoded once with
sda_varint_encode_dev into one device buffer of N blobs.  One process, one set of buffers; the legs are interleaved
block by block over several rounds, each block one warm-up call and 5 timed ones between HIP events on the launch
stream (every call ends in its own wait, as a caller sees it).
    python scripts/clerk_job_inproc.py [rounds] [out_file]
(a) at 1000 x 1M and 1000 x 16,384:
      job            sda_clerk_job_dev with a payload: one call, one wait (the device-length encode, route 1)
      two calls      sda_clerk_decode_combine_dev + sda_varint_encode_dev(rows = 1): two waits -- the yardstick
      two calls (2)  the same sequence again, as a leg of its own: the spread between the two, and between the rounds
                     of each, is what the run can resolve
      combine        sda_clerk_decode_combine_dev alone
      combine alt    the same through SDA_INPROC_ALT_LIB (the parent commit's libsda_engine.so), when given
    The job must not be slower than the two calls by more than that sequence's own spread.
(b) the same 1000 blobs as 4 continuing tiles of 250 (the payload from the last) against the one call, next to the
    cost model: 3 more reads and 3 more writes of the 8 D-byte state, and 3 more calls' launches and waits.
SDA_INPROC_ROWS / SDA_INPROC_DIMS (comma separated) shrink the job (rehearsal).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, schemes as S  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=5):
    fn()                                                                                # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


torch.cuda.init()
eng = Engine(0)
ALT = os.environ.get("SDA_INPROC_ALT_LIB")
alt = Engine(0, lib_path=ALT) if ALT else None
st = torch.cuda.current_stream().cuda_stream
p = S.CONFIG_PACKED.prime_modulus
N = int(os.environ.get("SDA_INPROC_ROWS", 1000))
DIMS = [int(d) for d in os.environ.get("SDA_INPROC_DIMS", "1000000,16384").split(",")]
TILES = 4
say(f"clerk_job_inproc: {N} blobs of field shares uniform in (-p, p), p={p}  rounds={rounds} (1 warm-up + 5 timed "
    f"calls per block)" + (f"  alt lib {os.path.basename(os.path.dirname(ALT))}/{os.path.basename(ALT)}" if alt else ""))

for D in DIMS:
    x = torch.empty((N, D), dtype=torch.int64, device="cuda")
    eng.synth_fill_dev(x.data_ptr(), N, D, 0x5DA + 9, -(p - 1), p, st)
    cap = N * D * 5 + 32
    blobs = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    rb = eng.varint_encode_dev(x.data_ptr(), N, D, D, blobs.data_ptr(), cap, st)
    del x
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(rb, dtype=np.uint64)])
    assert int(off[-1]) + 32 <= cap
    state = {k: torch.zeros(D, dtype=torch.int64, device="cuda") for k in ("job", "two", "tiles", "alt")}
    pcap = D * 10 + 16
    pay = {k: torch.zeros(pcap, dtype=torch.uint8, device="cuda") for k in ("job", "two", "tiles")}
    plen = {}

    def job():
        plen["job"] = eng.clerk_job_dev(p, blobs.data_ptr(), off, state["job"].data_ptr(), D,
                                        payload_ptr=pay["job"].data_ptr(), payload_cap=pcap, stream=st)[1]

    def two():
        n = eng.clerk_decode_combine_dev(p, blobs.data_ptr(), off, state["two"].data_ptr(), D, st)
        plen["two"] = int(eng.varint_encode_dev(state["two"].data_ptr(), 1, n, n, pay["two"].data_ptr(), pcap, st)[0])

    def combine():
        eng.clerk_decode_combine_dev(p, blobs.data_ptr(), off, state["two"].data_ptr(), D, st)

    def combine_alt():
        alt.clerk_decode_combine_dev(p, blobs.data_ptr(), off, state["alt"].data_ptr(), D, st)

    per = (N + TILES - 1) // TILES

    def tiles():
        for b0 in range(0, N, per):
            b1 = min(b0 + per, N)
            last = b1 == N
            r = eng.clerk_job_dev(p, blobs.data_ptr(), off[b0:b1 + 1], state["tiles"].data_ptr(), D,
                                  first_participation=b0, prior_dim=D,
                                  payload_ptr=pay["tiles"].data_ptr() if last else None,
                                  payload_cap=pcap if last else 0, stream=st)
        plen["tiles"] = r[1]

    job()
    route = eng.clerk_job_last_launch()
    two()
    tiles()
    torch.cuda.synchronize()
    same = (plen["job"] == plen["two"] == plen["tiles"] and torch.equal(state["job"], state["two"])
            and torch.equal(state["tiles"], state["two"])
            and torch.equal(pay["job"][:plen["two"]], pay["two"][:plen["two"]])
            and torch.equal(pay["tiles"][:plen["two"]], pay["two"][:plen["two"]]))
    say(f"[{N} x {D}] payload in {int(off[-1])} B ({int(off[-1]) / N / D:.3f} B/share); result payload {plen['two']} B; "
        f"job record {route}; job, 4 tiles and two calls agree bit for bit: {same}")
    assert same and route[:2] == (0, 1)
    legs = [("job", job), ("two calls", two), ("two calls (2)", two), ("combine", combine), ("4 tiles", tiles)]
    if alt:
        legs.append(("combine alt", combine_alt))
    res = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, fn in legs:
            res[name].append(timed(fn))
    med = {}
    for name, _ in legs:
        s = sorted(res[name])
        med[name] = s[len(s) // 2]
        say(f"[{N} x {D}] {name:<14} median {med[name]:.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
            f"spread {100 * (s[-1] - s[0]) / med[name]:.2f} %  by round: " + " ".join(f"{v:.4f}" for v in res[name]))
    both = sorted(res["two calls"] + res["two calls (2)"])
    spread = both[-1] - both[0]
    say(f"[{N} x {D}] (a) job / two calls = {med['job'] / med['two calls']:.4f} (median), "
        f"{min(res['job']) / min(res['two calls']):.4f} (min); job - two calls = "
        f"{1e3 * (med['job'] - med['two calls']):+.1f} us; the two-call sequence's own spread over its "
        f"{len(both)} blocks = {1e3 * spread:.1f} us ({100 * spread / med['two calls']:.2f} %): "
        f"{'within' if med['job'] - med['two calls'] <= spread else 'OUTSIDE'}")
    if alt:
        say(f"[{N} x {D}] (a) combine / combine alt = {med['combine'] / med['combine alt']:.4f} (median)")
    # (b): every continuing tile reads and rewrites the 8 D-byte state once more than the one call writes it, at
    # the 4.0 TB/s a read + write stream reaches, and pays one more call: its launches, two copies and a wait,
    # taken here as what the encode-free remainder of a small call costs (the 16,384 job's `combine` leg bounds it)
    model_us = (TILES - 1) * 2 * 8.0 * D / 4.0e12 * 1e6
    say(f"[{N} x {D}] (b) 4 tiles / job = {med['4 tiles'] / med['job']:.4f} (median), "
        f"{min(res['4 tiles']) / min(res['job']):.4f} (min); 4 tiles - job = "
        f"{1e3 * (med['4 tiles'] - med['job']):+.1f} us; model: {TILES - 1} more reads and writes of the state = "
        f"{model_us:.1f} us at 4 TB/s, + {TILES - 1} calls' launches and waits")
    del blobs, state, pay

eng.close()
if alt:
    alt.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
