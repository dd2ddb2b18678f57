"""In-process A/B of the int32 combine against the i64 combine: one 10k x 1M i64 buffer (synth fill), one
sda_narrow32_dev of it, then the launches interleaved block by block, HIP events on the launch stream, so buffer
placement and box state are shared by every variant (the conventions of combine_pipe_inproc.py):
    i64          sda_combine_dev on the i64 rows
    int32        sda_combine32_dev: 4 columns per lane (16-byte loads), software-pipelined, balanced grid
    int32_vec2   the same entry point with SDA_COMBINE32_VEC=2: the codec's 2-column unpipelined kernel
Prints per-round lines, then ONE JSON line with the medians, the fractions of HBM peak (8 N D + 8 D bytes for
i64, 4 N D + 8 D for int32, 12 N D for the narrowing) and whether the results are bit-equal.
    python scripts/combine32_inproc.py [rounds] [label:VAR=value ...]
Every extra `label:VAR=value` is one more int32 variant launched with that variable set.
SDA_INPROC_ROWS / SDA_INPROC_COLS shrink the job (default 10000 x 1000000).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sda_amd import Engine  # noqa: E402

M = 2147482801
HBM_PEAK = 8.0e12
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(os.environ.get("SDA_INPROC_ROWS", 10_000))
D = int(os.environ.get("SDA_INPROC_COLS", 1_000_000))
# label -> (int32 rows?, environment of the launch)
variants = {"i64": (False, {}), "int32": (True, {}), "int32_vec2": (True, {"SDA_COMBINE32_VEC": "2"})}
for extra in sys.argv[2:]:
    label, kv = extra.split(":", 1)
    k, v = kv.split("=", 1)
    variants[label] = (True, {k: v})
knobs = sorted({k for _, env in variants.values() for k in env})

torch.cuda.init()
eng = Engine(0)
st = torch.cuda.current_stream().cuda_stream
x = torch.empty((N, D), dtype=torch.int64, device="cuda")
eng.synth_fill_dev(x.data_ptr(), N, D, 0x5DB, -(M - 1), M, st)      # signed: the order-dependent worst case
x32 = torch.empty((N, D), dtype=torch.int32, device="cuda")
flag = torch.zeros(1, dtype=torch.int64, device="cuda")


def timed(fn, reps):
    fn()                                                                            # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


narrow_ms = sorted(timed(lambda: eng.narrow32_dev(x.data_ptr(), N, D, D, x32.data_ptr(), D, flag.data_ptr(), st), 3)
                   for _ in range(rounds))
assert int(flag.item()) == 0, "the synthetic shares must fit int32"
outs = {v: torch.zeros(D, dtype=torch.int64, device="cuda") for v in variants}


def launch(v):
    narrow, _ = variants[v]
    if narrow:
        eng.combine32_dev(M, x32.data_ptr(), N, D, D, outs[v].data_ptr(), st)
    else:
        eng.combine_dev(M, x.data_ptr(), N, D, D, outs[v].data_ptr(), st)


res = {v: [] for v in variants}
for r in range(rounds):
    for v, (narrow, env) in variants.items():
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(env)
        ms = timed(lambda: launch(v), 10)
        res[v].append(ms)
        print(f"round {r} {v} {ms:.4f} ms  {(4.0 if narrow else 8.0) * N * D / ms / 1e9:.3f} TB/s", flush=True)
for k in knobs:
    os.environ.pop(k, None)
same = all(torch.equal(outs[v], outs["i64"]) for v in variants)
med = {v: sorted(t)[len(t) // 2] for v, t in res.items()}
nm = narrow_ms[len(narrow_ms) // 2]
line = {"script": "combine32_inproc", "rows": N, "cols": D, "rounds": rounds, "bit_identical": same,
        "narrow32_ms": round(nm, 4), "narrow32_hbm_frac": round(12.0 * N * D / (nm * 1e-3) / HBM_PEAK, 4)}
for v, (narrow, _) in variants.items():
    bytes_ = (4.0 if narrow else 8.0) * N * D + 8.0 * D
    line[f"{v}_ms"] = round(med[v], 4)
    line[f"{v}_min_ms"] = round(min(res[v]), 4)
    line[f"{v}_hbm_frac"] = round(bytes_ / (med[v] * 1e-3) / HBM_PEAK, 4)
line["int32_vs_i64"] = round(med["i64"] / med["int32"], 4)
line["int32_vs_vec2"] = round(med["int32_vec2"] / med["int32"], 4)
print(json.dumps(line))
sys.exit(0 if same else 1)
