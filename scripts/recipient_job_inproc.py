"""In-process timing of the recipient job (sda_recipient_job_dev, sda_recipient_job) against what a caller does
today, on the same payloads: configs[2]'s scheme (PackedShamir k=8 n=26 t=7), D values revealed from 15 clerk
results, masked by N Full masks or by S ChaCha seeds.  Everything is made on the device (sda_synth_fill_dev), encoded
once with sda_varint_encode_dev, and copied to the host once for the host legs.  One process, one set of buffers; the
legs are interleaved block by block over several rounds (the device legs in an order that rotates, `rounds` times
through every rotation); every leg's output is compared with the others' bit for bit.
    python scripts/recipient_job_inproc.py [rounds] [out_file]
Device legs (one warm-up call and 5 timed ones between HIP events on the launch stream per block):
      job            sda_recipient_job_dev: one call, one wait before the reveal
      two calls      sda_varint_decode_dev (clerk results -> i64 rows) + sda_recipient_reveal_dev: two waits -- the
                     yardstick.  Full masking: both sides take the mask folded once by sda_clerk_job_dev as their one
                     mask (row); ChaCha: the job takes the seed blobs, the two calls the key words packed on the host
                     as [S][8] rows, zero padded -- the matrix the job's seed kernel makes, so the same kernels run
      two calls w4   ChaCha only: the same with the key words as [S][4] rows, what a caller who knows that every seed
                     has 4 words passes (the mask combine reads 4 key words a seed instead of 8)
      two calls (2)  the same sequence again, as a leg of its own: its spread is what the run can resolve
    The job must not be slower than the two calls by more than that sequence's own spread.
Host legs (one warm-up call and 1 timed one per block, host clock around calls that return synchronised):
      job host       sda_recipient_job on the opened payloads
      today host     one sda_varint_decode per blob, then sda_recipient_reveal on the rows
SDA_INPROC_DIM / SDA_INPROC_MASKS / SDA_INPROC_SEEDS shrink the job (rehearsal); SDA_INPROC_HOST=0 leaves the host
legs out.
"""
import ctypes as C
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


torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream
ss = S.CONFIG_PACKED
p = ss.prime_modulus
D = int(os.environ.get("SDA_INPROC_DIM", 1_000_000))
N = int(os.environ.get("SDA_INPROC_MASKS", 1000))
NS = int(os.environ.get("SDA_INPROC_SEEDS", 256))
HOST = os.environ.get("SDA_INPROC_HOST", "1") != "0"
idx = list(range(ss.reconstruction_threshold()))
n_idx, B = len(idx), (D + ss.secret_count - 1) // ss.secret_count
say(f"recipient_job_inproc: PackedShamir k={ss.secret_count} n={ss.share_count} t={ss.privacy_threshold()} p={p}, "
    f"D={D} ({B} batches), {n_idx} clerk results; {N} Full masks / {NS} ChaCha seeds; rounds={rounds}")


def encode(rows, n, length):
    """n rows of `length` values on the device -> (payload tensor, host offsets)"""
    cap = n * length * 5 + 32
    blobs = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    rb = eng.varint_encode_dev(rows.data_ptr(), n, length, length, blobs.data_ptr(), cap, st)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(rb, dtype=np.uint64)])
    return blobs, off


def host_blobs(blobs, off):
    """the payload on the host and the (pointer, length) arrays of its blobs"""
    host = blobs[: int(off[-1])].cpu().numpy()
    n = off.size - 1
    ptrs = (E._u8p * n)(*[C.cast(host.ctypes.data + int(o), E._u8p) for o in off[:-1]])
    lens = (C.c_uint64 * n)(*[int(off[i + 1] - off[i]) for i in range(n)])
    return host, ptrs, lens


def decode_each(host_ptrs, lens, n, width):
    """what a caller does today: one sda_varint_decode per blob -> rows [n][width] on the host"""
    rows = np.zeros((n, width), np.int64)
    olen = C.c_uint64(0)
    for i in range(n):
        E._check(eng.lib.sda_varint_decode(eng.h, host_ptrs[i], lens[i], E._ptr(rows[i]), width, C.byref(olen)))
        assert olen.value == width
    return rows


# ---- the clerk results: 15 rows of B field shares
x = torch.empty((n_idx, B), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(x.data_ptr(), n_idx, B, 0x5DA + 21, -(p - 1), p, st)
clerk, coff = encode(x, n_idx, B)
del x
crow = torch.zeros((n_idx, B), dtype=torch.int64, device="cuda")
idx_arr = np.asarray(idx, np.uint64)


def report(tag, legs):
    res = {name: [] for name, _, _ in legs}
    # the device legs first, their order rotated from round to round: a block that follows an idle device or another
    # leg's buffers measured up to 4 % slower than the same block two places later, so every leg takes every place
    dev = [l for l in legs if not l[2]]
    for r in range(rounds * len(dev)):
        k = r % len(dev)
        for name, fn, _ in dev[k:] + dev[:k]:
            res[name].append(timed(fn))
    for r in range(rounds):
        for name, fn, host in legs:
            if host:
                fn()
                res[name].append(timed_host(fn))
    med = {}
    for name, _, _ in legs:
        s = sorted(res[name])
        med[name] = s[len(s) // 2]
        say(f"[{tag}] {name:<14} median {med[name]:.4f} ms  min {s[0]:.4f}  max {s[-1]:.4f}  "
            f"spread {100 * (s[-1] - s[0]) / med[name]:.2f} %  by round: " + " ".join(f"{v:.4f}" for v in res[name]))
    both = sorted(res["two calls"] + res["two calls (2)"])
    spread = both[-1] - both[0]
    say(f"[{tag}] job / two calls = {med['job'] / med['two calls']:.4f} (median), "
        f"{min(res['job']) / min(res['two calls']):.4f} (min); job - two calls = "
        f"{1e3 * (med['job'] - med['two calls']):+.1f} us; the two-call sequence's own spread over its {len(both)} "
        f"blocks = {1e3 * spread:.1f} us ({100 * spread / med['two calls']:.2f} %): "
        f"{'within' if med['job'] - med['two calls'] <= spread else 'OUTSIDE'}")
    if "job host" in med:
        say(f"[{tag}] job host / today host = {med['job host'] / med['today host']:.4f} (median): "
            f"{med['job host']:.1f} ms against {med['today host']:.1f} ms")
    else:
        say(f"[{tag}] job host / today host: not measured")


for masking in ("full", "chacha"):
    out = {k: torch.zeros(D, dtype=torch.int64, device="cuda") for k in ("job", "two", "w4")}
    hout = {k: np.zeros(D, np.int64) for k in ("job", "today")}
    olen = C.c_uint64(0)
    if masking == "full":
        ms = S.FullMasking(p)
        n_masks = N
        m = torch.empty((N, D), dtype=torch.int64, device="cuda")
        eng.synth_fill_dev(m.data_ptr(), N, D, 0x5DA + 22, 0, p, st)
        mblobs, moff = encode(m, N, D)
        del m
        # the mask payloads folded once, in 4 tiles, by the clerk's job: the state both device legs take
        state = torch.zeros(D, dtype=torch.int64, device="cuda")
        per = (N + 3) // 4

        def fold():
            for b0 in range(0, N, per):
                b1 = min(b0 + per, N)
                eng.clerk_job_dev(p, mblobs.data_ptr(), moff[b0:b1 + 1], state.data_ptr(), D, first_participation=b0,
                                  prior_dim=D, stream=st)
        say(f"[full] {N} mask payloads in {int(moff[-1])} B ({int(moff[-1]) / N / D:.3f} B/value); folded by "
            f"sda_clerk_job_dev in 4 tiles: {timed(fold, reps=1):.3f} ms")

        def job():
            eng.recipient_job_dev(ms, ss, D, idx, clerk.data_ptr(), coff, p, out["job"].data_ptr(), D,
                                  mask_ptr=state.data_ptr(), mask_len=D, stream=st)

        def two():
            eng.varint_decode_dev(clerk.data_ptr(), coff, crow.data_ptr(), B, st)
            eng.recipient_reveal_dev(ms, state.data_ptr(), 1, D, ss, D, idx, crow.data_ptr(), B, p,
                                     out["two"].data_ptr(), D, stream=st)
    else:
        ms = S.ChaChaMasking(p, D, 128)
        n_masks = NS
        words = np.random.default_rng(0x5DA).integers(0, 2**32, size=(NS, 4), dtype=np.int64)
        sd = torch.as_tensor(words).cuda()
        mblobs, moff = encode(sd, NS, 4)
        dwords4 = torch.as_tensor(words.astype(np.uint32).view(np.int32)).cuda()
        padded = np.zeros((NS, 8), np.uint32)
        padded[:, :4] = words
        dwords = torch.as_tensor(padded.view(np.int32)).cuda()

        def job():
            eng.recipient_job_dev(ms, ss, D, idx, clerk.data_ptr(), coff, p, out["job"].data_ptr(), D,
                                  seed_ptr=mblobs.data_ptr(), seed_off=moff, stream=st)

        def two():
            eng.varint_decode_dev(clerk.data_ptr(), coff, crow.data_ptr(), B, st)
            eng.recipient_reveal_dev(ms, dwords.data_ptr(), NS, 8, ss, D, idx, crow.data_ptr(), B, p,
                                     out["two"].data_ptr(), D, stream=st)

        def two_w4():
            eng.varint_decode_dev(clerk.data_ptr(), coff, crow.data_ptr(), B, st)
            eng.recipient_reveal_dev(ms, dwords4.data_ptr(), NS, 4, ss, D, idx, crow.data_ptr(), B, p,
                                     out["w4"].data_ptr(), D, stream=st)

    job()
    rec = (tuple(eng.recipient_job_last_launch()), tuple(eng.recipient_last_launch()))
    two()
    torch.cuda.synchronize()
    same = torch.equal(out["job"], out["two"])
    legs = [("job", job, False), ("two calls", two, False), ("two calls (2)", two, False)]
    if masking == "chacha":
        two_w4()
        torch.cuda.synchronize()
        same = same and torch.equal(out["w4"], out["two"])
        legs.append(("two calls w4", two_w4, False))
    if HOST:
        mhost, mptrs, mlens = host_blobs(mblobs, moff)
        chost, cptrs, clens = host_blobs(clerk, coff)
        msc, ssc = ms.c(), ss.c()

        def job_host():
            E._check(eng.lib.sda_recipient_job(eng.h, C.byref(msc), mptrs, mlens, n_masks, C.byref(ssc), D,
                                               E._ptr(idx_arr, E._u64p), cptrs, clens, n_idx, p, E.REVEAL_EXACT,
                                               E._ptr(hout["job"]), D, C.byref(olen)))

        def today_host():
            width = D if masking == "full" else 4
            mrows = decode_each(mptrs, mlens, n_masks, width)
            srows = decode_each(cptrs, clens, n_idx, B)
            rp = (E._i64p * n_masks)(*[E._ptr(mrows[i]) for i in range(n_masks)])
            rl = (C.c_uint64 * n_masks)(*([width] * n_masks))
            sp = (E._i64p * n_idx)(*[E._ptr(srows[i]) for i in range(n_idx)])
            sl = (C.c_uint64 * n_idx)(*([B] * n_idx))
            E._check(eng.lib.sda_recipient_reveal(eng.h, C.byref(msc), rp, rl, n_masks, C.byref(ssc), D,
                                                  E._ptr(idx_arr, E._u64p), sp, sl, n_idx, p, E.REVEAL_EXACT,
                                                  E._ptr(hout["today"]), D, C.byref(olen)))

        job_host()
        hrec = tuple(eng.recipient_job_last_launch())
        today_host()
        dev = out["two"].cpu().numpy()
        same = same and np.array_equal(hout["job"], dev) and np.array_equal(hout["today"], dev)
        legs += [("job host", job_host, True), ("today host", today_host, True)]
        say(f"[{masking}] host job record {hrec}")
    say(f"[{masking}] clerk payloads {int(coff[-1])} B; device job records {rec}; every leg's output agrees bit for "
        f"bit: {same}")
    assert same
    report(masking, legs)
    del out, mblobs

eng.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
