#!/usr/bin/env python
"""Times the MFCC front end of the timbre encoder (encoder.mfcc) at 16 x 2 s and 512 x 2 s of audio at
44.1 kHz, n_fft 2048, hop 512, 128 bands, 30 coefficients: the one-launch kernel (ddsp_mfcc) beside the same definition as torch
operations on the same device (encoder.mfcc_torch: a framing view times the window, the library FFT, magnitude, two matmuls and
a log).  Device events on the stream around back-to-back calls after a warm-up, `--repeats` repetitions of every timing and the
whole measurement twice (`--runs`): the median, the smallest and the largest of each run are printed in one JSON line, with the
largest difference between the two forms.  There is no threshold: DESIGN.md section 10h records the figures.

    python tools/bench_mfcc.py [--shapes 16x88200,512x88200] [--iters 200] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd import encoder as enc        # noqa: E402
from bench_align import timed                      # noqa: E402

RATE, N_FFT, HOP, N_MELS, N_MFCC = 44100, 2048, 512, 128, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x88200,512x88200")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mfcc.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    tables = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in enc.mfcc_tables(N_FFT, RATE, N_MELS, N_MFCC).items()}
    results = []
    for shape in args.shapes.split(","):
        B, L = (int(x) for x in shape.split("x"))
        iters = max(args.iters * 16 // max(B, 16), 10)
        x = torch.rand((B, L), device=dev, generator=torch.Generator(device="cuda").manual_seed(B)) * 2 - 1
        kernel = lambda: ddsp.mfcc(x, N_FFT, HOP, RATE, n_mels=N_MELS, n_mfcc=N_MFCC)              # noqa: E731
        stock = lambda: enc.mfcc_torch(x, tables, N_FFT, HOP)[0]                                   # noqa: E731
        runs = []
        for _ in range(args.runs):
            t = dict(kernel=timed(kernel, 5, iters, args.repeats), torch_ops=timed(stock, 5, iters, args.repeats))
            runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
        med = lambda key: statistics.median(r[key][0] for r in runs)                              # noqa: E731
        ours, theirs = kernel(), stock()
        frames = ours.shape[0] * ours.shape[1]
        results.append(dict(shape=dict(rows=B, samples=L, frames=ours.shape[1]), iters=iters, median_smallest_largest_per_run=runs,
                            kernel_frames_per_us=round(frames / med("kernel_ms") / 1e3, 1),
                            kernel_input_gb_per_s=round(B * L * 4 / med("kernel_ms") / 1e6, 1),
                            torch_ops_over_one_launch=round(med("torch_ops_ms") / med("kernel_ms"), 1),
                            max_abs_difference=float((ours - theirs).abs().max())))
    print(json.dumps(dict(results=results)))


if __name__ == "__main__":
    main()
