"""bench.py at N = 1 with the real renderer: a plain run prints the headline line only, --full adds the CPU baseline on the host.  The
workload is the reference's Box scene at test size; what is checked is which legs run, not the figures."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(extra, tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "PT_BENCH_STANDIN"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "box", "--size", "64", "--spp", "4", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "dump")] + extra, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0]), r.stderr


def test_plain_run_is_the_headline_only(tmp_path):
    out, _ = _run([], tmp_path)
    assert out["metric"] == "Msamples/s (all bounces)" and out["unit"] == "Msamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert abs(out["value"] - 64 * 64 * 4 / (out["ms_per_step"] / 1e3) / 1e6) <= 1e-9 * out["value"], "value and ms_per_step describe the same steps"
    assert "cpu_baseline" not in out and "weak" not in out
    assert out["roofline"]["launches_per_step"] >= 1, "roofline comes from the timed steps' own counters"
    assert os.listdir(str(tmp_path / "dump")) == ["image.npy"]


def test_full_run_adds_the_cpu_baseline(tmp_path):
    out, _ = _run(["--full", "--cpu-seconds", "0.5"], tmp_path)
    assert out["value"] > 0 and out["steps"] == 2
    base = out["cpu_baseline"]
    assert base["value"] > 0 and base["unit"] == "Msamples/s" and base["kind"] in ("reference", "port") and base["cores"] >= 1
