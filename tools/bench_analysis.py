#!/usr/bin/env python
"""Times harmonic analysis + residual (analysis.harmonic_residual) at the reference's dataset shape -- 16 clips of 2 s at
44.1 kHz, hop 512, window 2048, 180 harmonics -- on the HIP kernels against the package's own torch-op path on the same device
(the path CPU tensors and out-of-range shapes take, chunked over frames and samples so that it fits).  Device events on the
stream, warm-up first; prints one JSON line.  There is no threshold: DESIGN.md section 14 records both times.  --refine N runs N
steps of the f0 refinement (section 14a) in front of the analysis on both paths, from the track rounded to the 20-cent pitch grid.

    python tools/bench_analysis.py [--batch 16] [--seconds 2.0] [--iters 400] [--torch-iters 10] [--refine 0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd import analysis              # noqa: E402


def inputs(batch, frames, hop, sr, H, seed=0):
    """Harmonic + noise clips along a slow glide around 110 Hz (all 180 harmonics below Nyquist), as fp32 device tensors."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[None, :] / frames
    f0 = (110.0 * 2.0 ** (rng.uniform(-0.3, 0.3, (batch, 1)) * np.sin(2 * np.pi * (t + rng.uniform(0, 1, (batch, 1)))))).astype(np.float32)
    f0 = torch.from_numpy(f0).cuda()[..., None]
    theta = torch.cumsum(f0[..., 0].double().repeat_interleave(hop, dim=1) / sr, dim=1)
    audio = torch.zeros_like(theta)
    for k in range(1, 41):
        audio += torch.sin(2 * np.pi * ((k * theta) % 1.0) + float(rng.uniform(0, 6.28))) / k
    audio = audio / audio.abs().max() + 0.02 * torch.randn_like(audio)
    return audio.float().contiguous(), f0.contiguous()


def timed(fn, warmup, iters):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--torch-iters", type=int, default=10)
    ap.add_argument("--refine", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_analysis.py measures on the GPU; none is visible")
    sr, hop, W, H = 44100, 512, 2048, 180
    frames = int(args.seconds * sr) // hop
    audio, f0 = inputs(args.batch, frames, hop, sr, H)
    true = f0
    if args.refine:                                              # what a decoder hands over: the centres of 20-cent bins
        f0 = (10.0 * 2.0 ** ((20.0 * torch.round((1200.0 * torch.log2(f0.double() / 10.0) - 1997.3794084376191) / 20.0)
                              + 1997.3794084376191) / 1200.0)).float().contiguous()

    def kernels():
        return ddsp.harmonic_residual(audio, f0, hop, sr, H, W, return_complex=True, refine=args.refine)

    def torch_ops():
        track = f0
        for _ in range(args.refine):
            track = analysis._refine_torch(audio, track, f0, None, hop, sr, H, W, 50.0)
        C, a, c = analysis._analysis_torch(audio, track, None, hop, sr, H, W)
        harm = analysis._resynth_torch(C, track, hop, sr)
        return harm, audio - harm, dict(C=C, a=a, c=c, f0=track)

    ms_kernel, got = timed(kernels, 3, args.iters)
    ms_torch, want = timed(torch_ops, 1, args.torch_iters)
    out = dict(shape=dict(batch=args.batch, frames=frames, hop=hop, win_length=W, n_harmonics=H, sample_rate=sr), refine=args.refine,
               kernel_ms=round(ms_kernel, 4), torch_ops_ms=round(ms_torch, 3), speedup=round(ms_torch / ms_kernel, 1),
               max_abs_C_difference=float((got[2]["C"] - want[2]["C"]).abs().max()),
               max_abs_harm_difference=float((got[0] - want[0]).abs().max()),
               residual_rms_over_signal_rms=float((got[1].double().pow(2).mean() / audio.double().pow(2).mean()).sqrt()))
    if args.refine:
        lead = (W - hop) // 2                                    # the frames whose window lies inside the clip are measured; the
        inside = slice(-(-lead // hop), (frames * hop - W + lead) // hop + 1)   # ends follow the nearest of them by its ratio
        cents = lambda f: float((1200.0 * torch.log2(f.double() / true.double()))[:, inside].abs().max())      # noqa: E731
        out.update(max_cents_off_before=cents(f0), max_cents_off_after=cents(got[2]["f0"]),
                   max_abs_f0_difference=float((got[2]["f0"] - want[2]["f0"]).abs().max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
