"""bench.py with and without --full: a plain run ends with the figures of its timed steps, --full adds every other leg of the
line; both track the same slab to the same count."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "kernels_ms"}
# what only --full measures (era5_1deg_90: the 0.25 deg block belongs to the default workload alone)
FULL_ONLY = {"roofline", "stream_ceiling", "streaming", "pmc_live", "e2e", "concurrent_members", "cpu_baseline"}


def _bench(*more):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--workload", "era5_1deg_90"] + list(more)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_help_names_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout


@pytest.mark.gpu
def test_bench_plain_run_and_full_run():
    plain = _bench()
    assert HEADLINE <= set(plain) and not FULL_ONLY & set(plain) and "secondary_025deg" not in plain
    assert "coverage" not in plain["config"]
    assert plain["metric"] == "timesteps/sec labeled+tracked" and plain["unit"] == "timesteps/s" and plain["higher_is_better"] is True
    assert plain["steps"] == 4 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(90 / (plain["ms_per_step"] * 1e-3))
    # four timed steps: one event pair for each of the two streaming kernels
    assert plain["kernels_ms"]["k_threshold"] > 0 and plain["kernels_ms"]["k_relabel"] > 0

    full = _bench("--full", "--no-live-pmc")
    assert HEADLINE | (FULL_ONLY - {"pmc_live"}) <= set(full) and full["pmc_live"] is None
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup"):
        assert full[k] == plain[k], k
    assert full["config"]["n_tracked"] == plain["config"]["n_tracked"] > 0
    assert 0 < full["config"]["coverage"] < 1
    assert full["value"] == pytest.approx(90 / (full["ms_per_step"] * 1e-3))
    assert full["roofline"]["achieved"] > 0 and full["cpu_baseline"]["value"] > 0 and full["e2e"]["ms_per_call"] > 0
    assert full["concurrent_members"]["n_tracked"] == plain["config"]["n_tracked"]
    timed = {k for k, v in plain["kernels_ms"].items() if v > 0}
    assert timed < {k for k, v in full["kernels_ms"].items() if v > 0}          # the per-group times of the extra passes
