"""bench.py's command line: a plain run prints the headline line only, --dump-outputs writes what the last
timed step computed (seeded inputs, so the oracle can recompute it), and the dump's 64 MB cut is a fixed
sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sda_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    import bench
    a = torch.arange(-500, 500, dtype=torch.int64) * 2147483
    b = torch.arange(300, dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "whole"), {"a": a, "b": b})
    got = np.load(tmp_path / "whole" / "a.npy")
    assert got.dtype == np.float64 and np.array_equal(got, a.numpy())
    assert np.array_equal(np.load(tmp_path / "whole" / "b.npy"), b.numpy())
    # 1300 elements against a budget of 128 per array: the same sorted sample of each, run to run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 128 * 8)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    for name, src in (("a", a), ("b", b)):
        s1, s2 = np.load(tmp_path / "s1" / (name + ".npy")), np.load(tmp_path / "s2" / (name + ".npy"))
        assert s1.dtype == np.float64 and s1.shape == (128,) and np.array_equal(s1, s2)
        pos = np.searchsorted(src.numpy(), s1)          # both sources are strictly increasing
        assert np.array_equal(src.numpy()[pos], s1) and (np.diff(pos) > 0).all()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, oracle):
    """67 x 40,009 (odd sizes, several workgroups): the line carries the headline fields and none of the
    --full legs; combine.npy is the exact combine of the seeded matrix, element for element."""
    import bench
    N, D, m = 67, 40009, bench.MODULUS
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", str(N), "--dim", str(D), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == bench.METRIC and rec["unit"] == "GB/s" and rec["dtype"] == "int64"
    assert rec["higher_is_better"] is True and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    # value = the job's bytes per step / the step time; the line rounds ms_per_step to 1e-4 ms, value to 1e-3
    rel = 5e-5 / (rec["ms_per_step"] - 5e-5) + 1e-9
    assert abs(rec["value"] - 8.0 * (N * D + D) / (rec["ms_per_step"] * 1e-3) / 1e9) <= rel * rec["value"] + 1e-3
    for leg in ("cpu_baseline", "combine_signed", "host_path", "multi_device", "shamir", "chacha", "codec",
                "snapshot", "pipelines"):
        assert leg not in rec
    assert sorted(os.listdir(out)) == ["combine.npy"]
    got = np.load(out / "combine.npy")
    assert got.dtype == np.float64 and got.shape == (D,)
    exp = oracle.combine(m, synth.fill(N, D, bench.SEED_BASE + 1, 0, m))
    assert np.array_equal(got, exp.astype(np.float64))
