"""bench.py --dump-outputs: the audio of the last timed step, at most 64 MB, on inputs that are the same on every run.  The GPU
test regenerates that step's inputs (controls from their seed, the in-kernel noise stream from its Philox seed and offset) and
checks sampled rows of the dump against the CPU oracle."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dumped(directory):
    files = sorted(os.listdir(directory))
    assert files == ["audio.npy", "audio_rows.npy"], files
    assert sum(os.path.getsize(os.path.join(directory, f)) for f in files) <= 64_000_000
    audio, rows = np.load(os.path.join(directory, "audio.npy")), np.load(os.path.join(directory, "audio_rows.npy"))
    assert audio.dtype == np.float32 and rows.dtype == np.float64 and audio.shape[0] == rows.shape[0]
    return audio, rows.astype(np.int64)


@pytest.mark.parametrize("batch,expect_rows", [(512, 128), (200, 200), (1, 1)])
def test_dump_outputs_fits_and_samples_with_a_fixed_seed(tmp_path, batch, expect_rows):
    bench = load_bench()
    y = torch.arange(batch, dtype=torch.float32)[:, None].expand(batch, 64000).contiguous()     # row i holds i
    bench.dump_outputs(str(tmp_path / "a"), y)
    bench.dump_outputs(str(tmp_path / "b"), y)
    audio, rows = dumped(tmp_path / "a")
    audio_b, rows_b = dumped(tmp_path / "b")
    assert audio.shape == (expect_rows, 64000) and np.array_equal(rows, rows_b) and np.array_equal(audio, audio_b)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < batch
    assert np.array_equal(audio[:, 0], rows.astype(np.float32)) and np.array_equal(audio[:, -1], rows.astype(np.float32))


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_step():
    """`--steps K --warmup W` runs K timed steps; the dump is step W + K - 1 of the timed pass (noise offset (W + K - 1) << 32),
    whatever number of clock-settle steps ran before it."""
    import tempfile
    from ddsp_pytorch_amd import synthetic as syn
    from oracle import oracle
    steps, warmup = 3, 2
    with tempfile.TemporaryDirectory() as d:
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--no-cpu-baseline", "--no-secondary", "--no-live-pmc", "--dump-outputs", d],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        line = lines[0]
        assert line["steps"] == steps and line["clock_settle"]["timed_launches"]["count"] == steps and line["ms_per_step"] > 0
        audio, rows = dumped(d)
    shape = syn.CFG4_PER_GPU
    assert audio.shape == (128, shape.samples) and np.isfinite(audio).all()
    ctl = syn.make_controls(shape, 1004, "all_live")
    pick = [0, len(rows) // 2, len(rows) - 1]
    sel = rows[pick]
    ref = oracle.osc_forward(ctl["f0"][sel], ctl["c"][sel], ctl["a"][sel], shape.hop, shape.sample_rate)
    # the Philox stream is indexed by row: regenerate the whole batch's draw, keep the sampled rows
    noise = oracle.philox_uniform(1234, (warmup + steps - 1) << 32, shape.batch, shape.frames, shape.hop)[sel]
    ref += oracle.noise_forward(ctl["H"][sel], noise, shape.hop)
    assert float(np.max(np.abs(audio[pick] - ref))) <= 1e-5
