#!/usr/bin/env python
"""Times the inharmonic analysis (partials.partial_analysis) and analysis + residual (partials.partial_residual) at 16 clips of 2 s
at 44.1 kHz, hop 512, window 2048, 100 partials, on the HIP kernels; in the same run the package's own torch-op path on the same
device (the path CPU tensors and out-of-range shapes take) and analysis.harmonic_analysis at the same shape are measured again.
Every GPU step is a child process of its own under its own time limit, and a step that fails or runs out of time ends the run:
nothing more is started on the device.  Device events on the stream, warm-up first, `--repeats` timed windows per step (their
minimum, median and maximum are the run-to-run spread inside the process); prints one JSON line.  There is no threshold:
DESIGN.md section 14e records the times.

    python tools/bench_partials.py [--batch 16] [--seconds 2.0] [--iters 200] [--torch-iters 5] [--repeats 5] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("analysis", "analysis_reassign", "residual", "torch_analysis", "torch_residual", "harmonic_analysis")
SR, HOP, WINDOW, PARTIALS = 44100, 512, 2048, 100


def inputs(batch, frames, seed=0):
    """Stiff-string + noise clips (B = 1e-4) along a slow glide around 110 Hz, all partials below Nyquist: fp32 device tensors
    audio [B, N], f [B, T, K], f0 [B, T, 1]."""
    import torch
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[None, :] / frames
    f0 = 110.0 * 2.0 ** (rng.uniform(-0.3, 0.3, (batch, 1)) * np.sin(2 * np.pi * (t + rng.uniform(0, 1, (batch, 1)))))
    k = np.arange(1, PARTIALS + 1)
    f = torch.from_numpy((f0[..., None] * (k * np.sqrt(1.0 + 1e-4 * k * k))).astype(np.float32)).cuda()
    audio = torch.zeros((batch, frames * HOP), dtype=torch.float64, device="cuda")
    for i in range(40):                                          # the 40 lowest partials sound
        phase = torch.cumsum(f[..., i].double().repeat_interleave(HOP, dim=1) / SR, dim=1)
        audio += torch.sin(2 * np.pi * (phase % 1.0) + float(rng.uniform(0, 6.28))) / (i + 1)
    audio = audio / audio.abs().max() + 0.02 * torch.randn_like(audio)
    return audio.float().contiguous(), f.contiguous(), torch.from_numpy(f0.astype(np.float32)).cuda()[..., None].contiguous()


def child(args):
    import torch
    sys.path.insert(0, ROOT)
    import ddsp_pytorch_amd as ddsp
    from ddsp_pytorch_amd import partials
    if not torch.cuda.is_available():
        raise SystemExit("bench_partials.py measures on the GPU; none is visible")
    frames = int(args.seconds * SR) // HOP
    audio, f, f0 = inputs(args.batch, frames)

    def torch_analysis():
        return partials._analysis_torch(audio, f, None, HOP, SR, WINDOW, False)[0]

    def torch_residual():
        C = torch_analysis()
        return audio - partials._resynth_torch(C, f, HOP, SR)

    work = dict(analysis=lambda: ddsp.partial_analysis(audio, f, HOP, SR, WINDOW, return_complex=True)["C"],
                analysis_reassign=lambda: ddsp.partial_analysis(audio, f, HOP, SR, WINDOW, reassign=True)["f_re"],
                residual=lambda: ddsp.partial_residual(audio, f, HOP, SR, WINDOW)[1],
                torch_analysis=torch_analysis, torch_residual=torch_residual,
                harmonic_analysis=lambda: ddsp.harmonic_analysis(audio, f0, HOP, SR, PARTIALS, WINDOW, return_complex=True)["C"])[args.child]
    iters = args.torch_iters if args.child.startswith("torch") else args.iters
    for _ in range(2):
        out = work()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            out = work()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / iters)
    check = float(out.abs().double().sum()) if out.is_complex() else float(out.double().abs().sum())
    print(json.dumps(dict(step=args.child, ms_min=round(min(times), 4), ms_median=round(float(np.median(times)), 4),
                          ms_max=round(max(times), 4), iters=iters, repeats=args.repeats, checksum=check)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a step may take")
    ap.add_argument("--child", choices=STEPS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    frames = int(args.seconds * SR) // HOP
    out = dict(shape=dict(batch=args.batch, frames=frames, hop=HOP, win_length=WINDOW, n_partials=PARTIALS, sample_rate=SR), steps={})
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--batch", str(args.batch), "--seconds", str(args.seconds),
               "--iters", str(args.iters), "--torch-iters", str(args.torch_iters), "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out["failed"] = f"{step}: no result within {args.limit:g} s; nothing more was started"
            break
        if r.returncode != 0:
            out["failed"] = f"{step}: exit status {r.returncode}; nothing more was started: {r.stderr.strip()[-400:]}"
            break
        out["steps"][step] = json.loads(r.stdout.strip().splitlines()[-1])
    s = out["steps"]
    if "analysis" in s and "torch_analysis" in s:
        out["analysis_speedup_over_torch_ops"] = round(s["torch_analysis"]["ms_median"] / s["analysis"]["ms_median"], 1)
    if "residual" in s and "torch_residual" in s:
        out["residual_speedup_over_torch_ops"] = round(s["torch_residual"]["ms_median"] / s["residual"]["ms_median"], 1)
    if "analysis" in s and "harmonic_analysis" in s:
        out["analysis_over_harmonic_analysis"] = round(s["analysis"]["ms_median"] / s["harmonic_analysis"]["ms_median"], 2)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
