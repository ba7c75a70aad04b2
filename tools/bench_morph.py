#!/usr/bin/env python
"""Times the control morph (analysis.morph_controls) at the reference's dataset shape -- 16 clips of 172 frames (2 s at 44.1 kHz,
hop 512) morphed with 16 clips of 215 frames onto 172 output frames, 180 harmonics, 195 noise bands, a per-frame mix ramp, 'hz'
coordinates -- four ways on the same device: the HIP launch alone, the public call, the package's own torch-op path (what CPU
tensors and out-of-range shapes take), and what the package offered before for a harmonic-by-harmonic morph: two
transform_controls calls and a torch blend of the amplitudes they play.  Device events on the stream, warm-up first, `--repeats`
repetitions of every timing (the median and the spread are printed); one JSON line with the times, the kernel's bytes and the HBM
rate they make at this shape and at `--large-batch` rows.  There is no threshold: DESIGN.md section 14c records the figures.

    python tools/bench_morph.py [--batch 16] [--iters 2000] [--torch-iters 50] [--repeats 5] [--large-batch 2048]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd import analysis              # noqa: E402


def inputs(batch, frames, H, F, seed):
    """Controls along a slow glide around 110 Hz (all 180 harmonics below Nyquist), as fp32 device tensors."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[None, :] / frames
    f0 = (110.0 * 2.0 ** (rng.uniform(-0.3, 0.3, (batch, 1)) * np.sin(2 * np.pi * (t + rng.uniform(0, 1, (batch, 1)))))).astype(np.float32)
    c = (rng.uniform(0.05, 1.0, (batch, frames, H)) / np.arange(1, H + 1)).astype(np.float32)
    ctrl = dict(f0=f0[..., None], a=rng.uniform(0.1, 1.0, (batch, frames, 1)).astype(np.float32), c=c,
                H=rng.uniform(0.0, 1.0, (batch, frames, F)).astype(np.float32))
    return {k: torch.from_numpy(v).cuda().contiguous() for k, v in ctrl.items()}


def timed(fn, warmup, iters, repeats):
    """-> (median ms per call over `repeats` timings of `iters` calls, their smallest and largest, the last result)."""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            out = fn()
        stop.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(stop) / iters)
    return statistics.median(ms), min(ms), max(ms), out


def prepared(ctrl_a, ctrl_b, T_out):
    """The arrays both paths take, so that the launch alone can be timed."""
    srcs = []
    for ctrl in (ctrl_a, ctrl_b):
        B, T = ctrl["f0"].shape[:2]
        pos = ((torch.arange(T_out, dtype=torch.float64, device="cuda") + 0.5) * T / T_out - 0.5).clamp(0.0, T - 1.0).float()[None].expand(B, -1).contiguous()
        srcs.append((ctrl["f0"][..., 0].contiguous(), ctrl["a"][..., 0].contiguous(), ctrl["c"], ctrl["H"], pos))
    return srcs


def moved_bytes(B, T_a, T_b, T_out, H, F):
    compulsory = 4 * (B * (T_a + T_b) * (H + F + 2) + 5 * B * T_out + B * T_out * (H + F + 2))    # every input row once, every output once
    requested = 4 * B * T_out * (4 * (H + F + 2) + 5 + H + F + 2)                                # what the wavefronts ask for (four rows each)
    return compulsory, requested


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--torch-iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--large-batch", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_morph.py measures on the GPU; none is visible")
    sr, H, F, T_a, T_b, T_out, B = 44100, 180, 195, 172, 215, 172, args.batch
    ctrl_a, ctrl_b = inputs(B, T_a, H, F, 0), inputs(B, T_b, H, F, 1)
    ramp = torch.linspace(0.0, 1.0, T_out, device="cuda")

    def public():
        return ddsp.morph_controls(ctrl_a, ctrl_b, sr, mix=ramp, coordinates='hz')

    src_a, src_b = prepared(ctrl_a, ctrl_b, T_out)
    w = ramp[None].expand(B, -1).contiguous()

    def kernel():
        return analysis._morph_device(src_a, src_b, w, w, w, sr, H, True)

    def torch_ops():
        return analysis._morph_torch(src_a, src_b, w, w, w, sr, H, True)

    def by_hand():
        # harmonic by harmonic, from the parts the package had before: each sound stretched onto T' frames, then a blend of
        # the played amplitudes, of the pitches (in log frequency) and of the bands
        ta = ddsp.transform_controls(ctrl_a, sr, positions=src_a[4])
        tb = ddsp.transform_controls(ctrl_b, sr, positions=src_b[4])
        m = ramp[None, :, None]
        amp = (1 - m) * ta["a"] * ta["c"] + m * tb["a"] * tb["c"]
        total = amp.sum(-1, keepdim=True)
        return dict(f0=torch.exp2((1 - m) * torch.log2(ta["f0"]) + m * torch.log2(tb["f0"])), a=total, c=amp / total,
                    H=(1 - m) * ta["H"] + m * tb["H"])

    t_public = timed(public, 5, args.iters, args.repeats)
    t_kernel = timed(kernel, 5, args.iters, args.repeats)
    t_torch = timed(torch_ops, 2, args.torch_iters, args.repeats)
    t_hand = timed(by_hand, 5, args.iters // 4, args.repeats)
    got, alone, want = t_public[3], t_kernel[3], t_torch[3]
    compulsory, requested = moved_bytes(B, T_a, T_b, T_out, H, F)
    amp = lambda o: (o[1][..., None] * o[2]).double()                                             # noqa: E731
    scale = float(max((ctrl_a["a"] * ctrl_a["c"]).max(), (ctrl_b["a"] * ctrl_b["c"]).max()))
    same_f0 = (alone[0] == want[0])[..., None]                   # (one ulp in f0' moves the read-out: compared where it is the same)
    out = dict(shape=dict(batch=B, frames_a=T_a, frames_b=T_b, frames_out=T_out, n_harmonics=H, n_noise_filters=F, sample_rate=sr,
                          coordinates='hz'),
               call_ms=round(t_public[0], 5), call_ms_range=[round(v, 5) for v in t_public[1:3]],
               kernel_ms=round(t_kernel[0], 5), kernel_ms_range=[round(v, 5) for v in t_kernel[1:3]],
               torch_ops_ms=round(t_torch[0], 4), torch_ops_ms_range=[round(v, 4) for v in t_torch[1:3]],
               two_transforms_and_a_blend_ms=round(t_hand[0], 4), two_transforms_and_a_blend_ms_range=[round(v, 4) for v in t_hand[1:3]],
               compulsory_bytes=compulsory, requested_bytes=requested, kernel_gbps_compulsory=round(compulsory / t_kernel[0] / 1e6, 1),
               max_amplitude_difference=float(((amp(alone) - amp(want)) * same_f0).abs().max()) / scale,
               max_noise_difference=float((alone[3] - want[3]).abs().max()),
               same_as_public_call=bool(torch.equal(got["c"], alone[2]) and torch.equal(got["H"], alone[3])))
    if args.large_batch:
        Bl = args.large_batch
        big_a, big_b = inputs(Bl, T_a, H, F, 2), inputs(Bl, T_b, H, F, 3)
        la, lb = prepared(big_a, big_b, T_out)
        wl = ramp[None].expand(Bl, -1).contiguous()
        t_large = timed(lambda: analysis._morph_device(la, lb, wl, wl, wl, sr, H, True), 3, 50, args.repeats)
        big = moved_bytes(Bl, T_a, T_b, T_out, H, F)
        # the copy rate of the same device and run: a device-to-device copy of as many bytes as the kernel must move (read + write)
        buf = torch.empty(big[0] // 8, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(buf)
        t_copy = timed(lambda: dst.copy_(buf), 3, 50, args.repeats)
        out["large"] = dict(batch=Bl, kernel_ms=round(t_large[0], 4), kernel_ms_range=[round(v, 4) for v in t_large[1:3]],
                            compulsory_bytes=big[0], requested_bytes=big[1], kernel_gbps_compulsory=round(big[0] / t_large[0] / 1e6, 1),
                            kernel_gbps_requested=round(big[1] / t_large[0] / 1e6, 1), copy_gbps=round(8 * buf.numel() / t_copy[0] / 1e6, 1),
                            fraction_of_copy_rate=round((big[0] / t_large[0]) / (8 * buf.numel() / t_copy[0]), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
