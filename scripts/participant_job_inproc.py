"""In-process timing of the participant job (sda_full_mask_keyed_dev, sda_participant_job_dev, sda_participant_job)
against what a caller does today for the same job: configs[2]'s scheme (PackedShamir k=8 n=26 t=7), D secrets, Full
masking and ChaCha masking.  One process, one set of buffers; the legs are interleaved block by block over several
rounds (the device legs in an order that rotates, `rounds` times through every rotation); every leg's output is
compared with the others' byte for byte.
    python scripts/participant_job_inproc.py [rounds] [out_file]
Kernel legs (one warm-up call and 5 timed ones between HIP events on the launch stream per block):
      fused i64      sda_full_mask_keyed_dev: mask and masked secrets in one pass, the mask as i64
      fused int32    sda_full_mask_keyed32_dev: the same with the mask as int32 (what the job runs at this modulus)
      draws          sda_draws_dev alone: the lower bound of any sequence that makes the mask first
      draws + add    sda_draws_dev, then the add over [secrets; mask].  The engine has no device entry point for the
                     bare add sda_secret_mask_keyed launches, so sda_combine_dev over the two rows stands in for it:
                     the same 16 bytes read and 8 written per element
      draws + add (2) the same sequence again, as a leg of its own: its spread is what the run can resolve
Device legs (the same timing):
      job            sda_participant_job_dev
      sequence       sda_draws_dev (Full) + sda_participant_share32_keyed_dev + sda_varint_encode_dev of the mask
                     (the i64 mask sda_draws_dev leaves: no narrowing pass is charged to the yardstick); ChaCha: the
                     share call alone (the seed words' encode is a host loop on both sides)
      sequence (2)   the same again: its spread
    A gate holds when the new leg is not slower than its sequence by more than the sequence's own block-to-block spread.
Host legs (one warm-up call and 1 timed one per block, host clock around calls that return synchronised):
      job host       sda_participant_job
      today host     sda_secret_mask_keyed (ChaCha: sda_secret_mask) + sda_share_generate_keyed + one sda_varint_encode
                     per clerk row and one for the mask
SDA_INPROC_DIM shrinks the job (rehearsal); SDA_INPROC_HOST=0 leaves the host legs out.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine, engine as E, schemes as S  # noqa: E402

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


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(tag, legs, new, seq, floor=None):
    """legs: (name, fn, host); `new` legs are gated against `seq` (whose second copy is `seq + ' (2)'`)."""
    res = {name: [] for name, _, _ in legs}
    dev = [l for l in legs if not l[2]]
    for r in range(rounds * len(dev)):
        k = r % len(dev)
        for name, fn, _ in dev[k:] + dev[:k]:
            res[name].append(timed(fn))
    for r in range(rounds):
        for name, fn, host in legs:
            if host:
                res[name].append(timed_host(fn))
    med = {}
    for name, _, _ in legs:
        s = sorted(res[name])
        med[name] = s[len(s) // 2]
        say(f"[{tag}] {name:<15} median {med[name]:.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
            f"spread {100 * (s[-1] - s[0]) / med[name]:.2f} %  by round: " + " ".join(f"{v:.4f}" for v in res[name]))
    both = sorted(res[seq] + res[seq + " (2)"])
    spread = both[-1] - both[0]
    for name in new:
        say(f"[{tag}] {name} / {seq} = {med[name] / med[seq]:.4f} (median); {name} - {seq} = "
            f"{1e3 * (med[name] - med[seq]):+.1f} us; the sequence's own spread over its {len(both)} blocks = "
            f"{1e3 * spread:.1f} us ({100 * spread / med[seq]:.2f} %): "
            f"{'within' if med[name] - med[seq] <= spread else 'OUTSIDE'}")
        if floor:
            say(f"[{tag}] {name} / {floor} = {med[name] / med[floor]:.4f} (median)")
    return med


torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream
ss = S.CONFIG_PACKED
p, k, n = ss.prime_modulus, ss.secret_count, ss.share_count
D = int(os.environ.get("SDA_INPROC_DIM", 10_000_000))
HOST = os.environ.get("SDA_INPROC_HOST", "1") != "0"
B = (D + k - 1) // k
KEY = np.random.default_rng(0x5DA).integers(0, 2**32, size=8, dtype=np.uint64).astype(np.uint32)
MASK_STREAM, SHARE_STREAM = 1, 2
SEED = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]
say(f"participant_job_inproc: PackedShamir k={k} n={n} t={ss.privacy_threshold()} p={p}, D={D} ({B} batches); "
    f"rounds={rounds}")

secrets = torch.empty(D, dtype=torch.int64, device="cuda")
eng.synth_fill_dev(secrets.data_ptr(), 1, D, 0x5DA + 31, 0, p, st)
torch.cuda.synchronize()
secrets_host = secrets.cpu().numpy()

# ---------------------------------------------------------------- the kernel
two = torch.zeros((2, D), dtype=torch.int64, device="cuda")     # [secrets; mask] of the sequence
two[0].copy_(secrets)
masked = {x: torch.zeros(D, dtype=torch.int64, device="cuda") for x in ("f64", "f32", "seq")}
mask64 = torch.zeros(D, dtype=torch.int64, device="cuda")
mask32 = torch.zeros(D, dtype=torch.int32, device="cuda")


def fused64():
    eng.full_mask_keyed_dev(p, secrets.data_ptr(), D, KEY, MASK_STREAM, masked["f64"].data_ptr(), mask64.data_ptr(),
                            stream=st)


def fused32():
    eng.full_mask_keyed_dev(p, secrets.data_ptr(), D, KEY, MASK_STREAM, masked["f32"].data_ptr(), mask32.data_ptr(),
                            mask32=True, stream=st)


def draws():
    eng.draws_dev(KEY, MASK_STREAM, 0, D, p, two[1].data_ptr(), st)


def draws_add():
    eng.draws_dev(KEY, MASK_STREAM, 0, D, p, two[1].data_ptr(), st)
    eng.combine_dev(p, two.data_ptr(), 2, D, D, masked["seq"].data_ptr(), st)


fused64(), fused32(), draws_add()
torch.cuda.synchronize()
same = (torch.equal(mask64, two[1]) and torch.equal(mask32.to(torch.int64), two[1]) and
        torch.equal(masked["f64"], masked["seq"]) and torch.equal(masked["f32"], masked["seq"]))
say(f"[kernel] per element the fused kernel reads 8 B and writes 16 B (i64 mask) or 12 B (int32 mask); draws + add "
    f"moves 8 + 24 B; outputs agree bit for bit: {same}")
assert same
report("kernel", [("fused i64", fused64, False), ("fused int32", fused32, False), ("draws", draws, False),
                  ("draws + add", draws_add, False), ("draws + add (2)", draws_add, False)],
       new=("fused i64", "fused int32"), seq="draws + add", floor="draws")
del two, masked, mask64, mask32

# ---------------------------------------------------------------- the two job forms
for masking in ("full", "chacha"):
    ms = S.FullMasking(p) if masking == "full" else S.ChaChaMasking(p, D, 128)
    seed = SEED if masking == "chacha" else None
    row_bound, mask_bound = E.participant_job_payload_bound(ms, ss, D)
    cap = n * row_bound
    pay = {x: torch.zeros(cap + 32, dtype=torch.uint8, device="cuda") for x in ("job", "seq")}
    mpay = {x: torch.zeros(mask_bound + 32, dtype=torch.uint8, device="cuda") for x in ("job", "seq")}
    shares32 = torch.zeros((n, B), dtype=torch.int32, device="cuda")
    full = torch.zeros(D, dtype=torch.int64, device="cuda") if masking == "full" else None
    got = {}

    def job():
        got["job"] = eng.participant_job_dev(ms, ss, secrets.data_ptr(), D, KEY, MASK_STREAM, SHARE_STREAM,
                                             pay["job"].data_ptr(), cap, mpay["job"].data_ptr(), mask_bound, seed=seed,
                                             stream=st)

    def sequence():
        if full is not None:
            eng.draws_dev(KEY, MASK_STREAM, 0, D, p, full.data_ptr(), st)
        rb = eng.participant_share32_keyed_dev(ms, ss, secrets.data_ptr(), D, KEY, SHARE_STREAM, shares32.data_ptr(),
                                               seed=seed, full_masks_ptr=full.data_ptr() if full is not None else None,
                                               payload_ptr=pay["seq"].data_ptr(), payload_cap=cap, stream=st)
        ml = 0
        if full is not None:
            ml = int(eng.varint_encode_dev(full.data_ptr(), 1, D, D, mpay["seq"].data_ptr(), mask_bound, st)[0])
        got["seq"] = (rb, ml)

    job(), sequence()
    torch.cuda.synchronize()
    rb, ml = got["job"]
    total = int(rb.sum())
    same = (rb.tolist() == got["seq"][0].tolist() and torch.equal(pay["job"][:total], pay["seq"][:total]))
    if masking == "full":
        same = same and ml == got["seq"][1] and torch.equal(mpay["job"][:ml], mpay["seq"][:ml])
    say(f"[{masking}] clerk payloads {total} B ({total / (n * B):.3f} B/share), mask payload {ml} B; job record "
        f"{tuple(eng.participant_job_last_launch())}; the job's bytes equal the sequence's: {same}")
    assert same
    legs = [("job", job, False), ("sequence", sequence, False), ("sequence (2)", sequence, False)]
    if HOST:
        hgot = {}

        def job_host():
            hgot["job"] = eng.participant_job(ms, ss, secrets_host, KEY, MASK_STREAM, SHARE_STREAM, seed=seed)

        def today_host():
            if masking == "full":
                mask, msk = eng.secret_mask_keyed(ms, secrets_host, KEY, MASK_STREAM)
            else:
                mask, msk = eng.secret_mask(ms, secrets_host, seed=seed)
            sh = eng.share_generate_keyed(ss, msk, KEY, SHARE_STREAM)
            hgot["today"] = ([eng.varint_encode(sh[c]) for c in range(n)], eng.varint_encode(mask))

        job_host(), today_host()
        hrec = tuple(eng.participant_job_last_launch())
        dev_rows = pay["job"][:total].cpu().numpy().tobytes()
        same = (b"".join(hgot["job"][0]) == dev_rows and hgot["job"][1] == mpay["job"][:ml].cpu().numpy().tobytes()
                and hgot["today"][0] == hgot["job"][0] and hgot["today"][1] == hgot["job"][1])
        say(f"[{masking}] host job record {hrec}; host legs' bytes equal the device job's: {same}")
        assert same
        legs += [("job host", job_host, True), ("today host", today_host, True)]
        mask_vals = D if masking == "full" else len(SEED)
        today_up = 8 * D + 8 * D + 8 * (n * B + mask_vals)       # mask call, generate call, the encodes
        today_down = 8 * (D + mask_vals) + 8 * n * B + total + ml
        say(f"[{masking}] PCIe bytes: job host {8 * D} up + {total + ml} down = {8 * D + total + ml}; today host "
            f"{today_up} up + {today_down} down = {today_up + today_down}")
    med = report(masking, legs, new=("job",), seq="sequence")
    if HOST:
        say(f"[{masking}] job host / today host = {med['job host'] / med['today host']:.4f} (median): "
            f"{med['job host']:.1f} ms against {med['today host']:.1f} ms")
    del pay, mpay, shares32, full

eng.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
