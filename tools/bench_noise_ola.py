#!/usr/bin/env python
"""Times the overlap-add filtered noise (noise_forward / noise_backward with overlap_add=True) next to the truncated forms the
same calls take without the flag, at the two headline shapes: 512 x 500 frames of hop 128 / 65 bands and 512 x 375 frames of
hop 512 / 195 bands, in-kernel draws, workspace allocation included (as the Python layer pays it).  Device events on the stream
bracket back-to-back calls after warm-up; every figure is taken `--repeats` times and printed as median and (max - min) / median.
For the first shape the synthesis step of bench.py (oscillator bank, 100 harmonics, + noise accumulated into its buffer) is timed
with either form, which gives the mode's share of that step.  Prints one JSON line.  There is no threshold: DESIGN.md section 5a
records the times.

    python tools/bench_noise_ola.py [--iters 200] [--repeats 5] [--batch 512]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402

SHAPES = [(500, 128, 65, 16000, 100), (375, 512, 195, 44100, 100)]      # frames, hop, bands, sample rate, harmonics


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def figure(fn, iters, repeats):
    ms = [timed(fn, 10, iters) for _ in range(repeats)]
    med = statistics.median(ms)
    return dict(ms=round(med, 4), spread=round((max(ms) - min(ms)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise_ola.py measures on the GPU; none is visible")
    B = args.batch
    gen = torch.Generator("cuda").manual_seed(0)
    out = []
    for T, hop, F, rate, harmonics in SHAPES:
        H = torch.rand(B, T, F, device="cuda", generator=gen)
        g = torch.randn(B, T * hop, device="cuda", generator=gen)
        y = torch.zeros(B, T * hop, device="cuda")
        row = dict(shape=dict(batch=B, frames=T, hop=hop, n_filters=F))
        for name, flag in (("overlap_add", True), ("truncated", False)):
            row[name] = dict(
                forward=figure(lambda: ddsp.noise_forward(H, hop, seed=1, out=y, overlap_add=flag), args.iters, args.repeats),
                backward=figure(lambda: ddsp.noise_backward(g, hop, F, seed=1, overlap_add=flag), args.iters, args.repeats))
        row["forward_ratio"] = round(row["overlap_add"]["forward"]["ms"] / row["truncated"]["forward"]["ms"], 2)
        row["backward_ratio"] = round(row["overlap_add"]["backward"]["ms"] / row["truncated"]["backward"]["ms"], 2)
        if hop == 128:
            f0 = 100.0 + 60.0 * torch.rand(B, T, 1, device="cuda", generator=gen)
            c = torch.rand(B, T, harmonics, device="cuda", generator=gen) / harmonics
            a = torch.rand(B, T, 1, device="cuda", generator=gen)

            def step(flag):
                dry = ddsp.osc_forward(f0, c, a, hop, rate)[0]
                ddsp.noise_forward(H, hop, seed=1, out=dry, accumulate=True, overlap_add=flag)

            row["synthesis_step"] = dict(overlap_add=figure(lambda: step(True), args.iters, args.repeats),
                                         truncated=figure(lambda: step(False), args.iters, args.repeats))
            row["share_of_step"] = round(row["overlap_add"]["forward"]["ms"] / row["synthesis_step"]["overlap_add"]["ms"], 3)
        out.append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
