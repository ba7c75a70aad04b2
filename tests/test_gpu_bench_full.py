"""bench.py without and with --full: a plain run prints the headline line and measures nothing after its timed region; --full adds
the clock probe, the other kernels' averages and the CPU baseline.  Small batch (which also leaves out the secondary
configurations and the live traffic passes), one rank."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"osc_frame_totals", "osc_scan", "osc_frame_synth", "noise_frame"}


def bench_line(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "16", *extra], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["avg_launch_ms"] == line["kernel_ms"]["osc_frame_synth"] > 0
    return line


def test_plain_run_measures_only_the_timed_region():
    line = bench_line()
    assert set(line["kernel_ms"]) == {"osc_frame_synth"} and set(line["per_rank_kernel_ms"]) == {"osc_frame_synth"}
    for k in ("clock_ghz", "kernel_Mcycles", "configs", "cpu_baseline"):
        assert k not in line, k
    assert "noise_frame" not in line["roofline"] and line["roofline"]["valu"]["frac_at_clock"] is None


def test_full_run_adds_the_figures_after_the_timed_region():
    line = bench_line("--full")
    assert set(line["kernel_ms"]) == KERNELS and set(line["per_rank_kernel_ms"]) == KERNELS
    assert all(v > 0 for v in line["kernel_ms"].values())
    assert line["clock_ghz"] is None or 1.0 < line["clock_ghz"] < 3.0
    assert line["roofline"]["noise_frame"]["avg_launch_ms"] == line["kernel_ms"]["noise_frame"]
    assert line["cpu_baseline"]["value"] > 0 and "configs" not in line
