"""bench.py --dump-outputs on the GPU: two runs with the same arguments dump the same arrays, and they are the flags of the CPU
oracle on the bench's slab."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--workload", "era5_1deg_90",
           "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_and_match_oracle(tmp_path):
    import bench
    import oracle
    r1, r2 = _bench(tmp_path / "a", 3), _bench(tmp_path / "b", 2)
    assert r1["steps"] == 3 and r2["steps"] == 2 and r1["ms_per_step"] > 0
    names = r1["dumped_outputs"]["files"]
    assert r1["dumped_outputs"]["bytes"] <= 64 << 20
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert got[n].dtype == np.float64
        assert np.array_equal(got[n], np.load(tmp_path / "b" / n)), n
    wl = bench.WORKLOADS["era5_1deg_90"]
    a, w = bench.make_slab(wl)
    thr = np.full(wl["T"], np.float64(np.float32(wl["threshold"])))
    want, nw = oracle.run_contrack(a, thr, wl["gorl"], w, wl["overlap"], wl["persistence"], wl["twosided"])
    assert got["n_tracked.npy"].tolist() == [float(nw)] == [float(r1["config"]["n_tracked"])]
    t = got["flag_sample_t.npy"].astype(np.int64)
    assert np.array_equal(got["flag_sample.npy"], want[t])
    assert np.array_equal(got["flag_per_step.npy"][:, 0], np.count_nonzero(want, axis=(1, 2)))
    assert np.array_equal(got["flag_per_step.npy"][:, 1], want.sum(axis=(1, 2), dtype=np.int64))
