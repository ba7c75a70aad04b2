#!/usr/bin/env python
"""Times the control transformation (analysis.transform_controls) at the reference's dataset shape -- 16 clips of 172 frames (2 s
at 44.1 kHz, hop 512), 180 harmonics, 195 noise bands, stretched by 1.5 and moved up 7 semitones with the formants kept -- on
the HIP kernel against the package's own torch-op path on the same device (the path CPU tensors and out-of-range shapes take).
Device events on the stream, warm-up first; prints one JSON line with both times, the kernel's bytes and the HBM rate they
make.  There is no threshold: DESIGN.md section 14b records both times.

    python tools/bench_transform.py [--batch 16] [--frames 172] [--iters 2000] [--torch-iters 50]
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


def inputs(batch, frames, H, F, seed=0):
    """Controls along a slow glide around 110 Hz (all 180 harmonics below Nyquist), as fp32 device tensors."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[None, :] / frames
    f0 = (110.0 * 2.0 ** (rng.uniform(-0.3, 0.3, (batch, 1)) * np.sin(2 * np.pi * (t + rng.uniform(0, 1, (batch, 1)))))).astype(np.float32)
    c = (rng.uniform(0.05, 1.0, (batch, frames, H)) / np.arange(1, H + 1)).astype(np.float32)
    ctrl = dict(f0=f0[..., None], a=rng.uniform(0.1, 1.0, (batch, frames, 1)).astype(np.float32), c=c,
                H=rng.uniform(0.0, 1.0, (batch, frames, F)).astype(np.float32))
    return {k: torch.from_numpy(v).cuda().contiguous() for k, v in ctrl.items()}


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
    ap.add_argument("--frames", type=int, default=172)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--torch-iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transform.py measures on the GPU; none is visible")
    sr, H, F, stretch, semitones = 44100, 180, 195, 1.5, 7.0
    ctrl = inputs(args.batch, args.frames, H, F)
    B, T = args.batch, args.frames

    def public():
        return ddsp.transform_controls(ctrl, sr, stretch=stretch, transpose=semitones, formant=0.0)

    T_out = public()["c"].shape[1]
    # the prepared arrays both paths take, so that the two launches alone can be timed too
    f0, a, c, N = ctrl["f0"][..., 0].contiguous(), ctrl["a"][..., 0].contiguous(), ctrl["c"], ctrl["H"]
    pos = ((torch.arange(T_out, dtype=torch.float64, device="cuda") + 0.5) * T / T_out - 0.5).clamp(0.0, T - 1.0).float()[None].expand(B, -1).contiguous()
    r = torch.full((B, T_out), float(np.float32(2.0 ** (semitones / 12.0))), device="cuda")
    q = torch.ones((B, T_out), device="cuda")

    def kernel():
        return analysis._transform_device(f0, a, c, N, pos, r, q, sr, H)

    def torch_ops():
        return analysis._transform_torch(f0, a, c, N, pos, r, q, sr, H)

    ms_public, got = timed(public, 5, args.iters)
    ms_kernel, alone = timed(kernel, 5, args.iters)
    ms_torch, want = timed(torch_ops, 2, args.torch_iters)
    moved = 4 * (B * T * (H + F + 2) + 3 * B * T_out + B * T_out * (H + F + 2))      # every input row once, every output once
    fetched = 4 * B * T_out * (2 * (H + F + 2) + 3 + H + F + 2)                     # what the wavefronts ask for (two rows each)
    amp = lambda o: (o[1][..., None] * o[2]).double()                                             # noqa: E731
    scale = float((ctrl["a"] * ctrl["c"]).max())
    out = dict(shape=dict(batch=B, frames=T, frames_out=T_out, n_harmonics=H, n_noise_filters=F, sample_rate=sr, stretch=stretch,
                          transpose=semitones, formant=0.0),
               call_ms=round(ms_public, 5), kernel_ms=round(ms_kernel, 5), torch_ops_ms=round(ms_torch, 4),
               compulsory_bytes=moved, requested_bytes=fetched, kernel_gbps_compulsory=round(moved / ms_kernel / 1e6, 1),
               kernel_gbps_requested=round(fetched / ms_kernel / 1e6, 1),
               max_amplitude_difference=float((amp(alone) - amp(want)).abs().max()) / scale,
               max_noise_difference=float((alone[3] - want[3]).abs().max()),
               same_as_public_call=bool(torch.equal(got["c"], alone[2]) and torch.equal(got["H"], alone[3])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
