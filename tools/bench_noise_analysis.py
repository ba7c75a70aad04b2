#!/usr/bin/env python
"""Times the noise analysis (analysis.noise_analysis) at the reference's dataset shape -- the residuals of 16 clips x 172 frames
at hop 512, 195 bands, 16 iterations -- on the HIP kernels against the package's own torch-op path on the same device (the path
CPU tensors and out-of-range shapes take).  Device events on the stream bracket back-to-back calls after warm-up; the share of
the fixed point's iterations is measured by calls that stop early (iterations 0) and that do more (2 x iterations).  Prints one
JSON line.  There is no threshold: DESIGN.md section 15 records the times.

    python tools/bench_noise_analysis.py [--batch 16] [--frames 172] [--iters 200] [--torch-iters 5] [--average 1] [--iterations 16]

--overlap-add times the analysis of the overlap-add noise model (8 iterations unless --iterations says
otherwise) on the overlap-add noise of the same H, alternating in one process with the truncated analysis at 8 and at 16
iterations, with a call that stops before the first iteration and with the model's torch-op path: --rounds (5) rounds of every
leg in turn, the median over the rounds and the spread (max - min) / median of each.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd import analysis              # noqa: E402


def inputs(batch, frames, hop, F, seed=0, overlap_add=False):
    """FilteredNoise (in-kernel draw) of a smooth, slowly moving H: what a residual looks like to the analysis."""
    gen = torch.Generator().manual_seed(seed)
    b = torch.linspace(0, 1, F)[None, None, :]
    t = torch.linspace(0, 1, frames)[None, :, None]
    centre = 0.3 + 0.25 * torch.sin(2 * torch.pi * (t + torch.rand(batch, 1, 1, generator=gen)))
    H = 0.02 + 0.15 * (1 - b) + 0.8 * torch.exp(-0.5 * ((b - centre) / 0.08) ** 2)
    conf = type("Conf", (), dict(hop_length=hop))
    noise = ddsp.FilteredNoise(conf, rng="device", seed=seed, overlap_add=overlap_add).cuda()
    return noise({"H": H.float().cuda().contiguous()}).contiguous()


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


def overlap_add_legs(args, hop, F):
    """The overlap-add analysis beside the truncated one: every leg once per round, in turn."""
    x = inputs(args.batch, args.frames, hop, F, overlap_add=True)
    iterations = args.iterations if args.iterations is not None else analysis.NOISE_OLA_ITERATIONS

    def call(overlap_add, its):
        return lambda: ddsp.noise_analysis(x, hop, F, average=args.average, iterations=its, overlap_add=overlap_add)

    legs = {"overlap_add_ms": (call(True, iterations), args.iters),
            "truncated_8_ms": (call(False, 8), args.iters),
            "truncated_16_ms": (call(False, 16), args.iters),
            "overlap_add_without_iterations_ms": (call(True, 0), args.iters),
            "overlap_add_double_iterations_ms": (call(True, 2 * iterations), args.iters),
            "overlap_add_torch_ops_ms": (lambda: analysis._noise_ola_torch(x, hop, F, args.average, iterations)[0], args.torch_iters)}
    times = {name: [] for name in legs}
    outs = {}
    for _ in range(args.rounds):
        for name, (fn, iters) in legs.items():
            ms, outs[name] = timed(fn, 1 if "torch" in name else 3, iters)
            times[name].append(ms)
    median = {name: statistics.median(v) for name, v in times.items()}
    got, want = outs["overlap_add_ms"], outs["overlap_add_torch_ops_ms"]
    # a band whose model spectrum is below fp32's rounding of its own sum can take the update's floor in one path and not in the
    # other: such frames are counted, and the two paths compared on the rest
    finite = torch.isfinite(got).all(-1) & torch.isfinite(want).all(-1)
    non_finite = dict(kernels=int((~torch.isfinite(got).all(-1)).sum()), torch_ops=int((~torch.isfinite(want).all(-1)).sum()))
    got, want = got[finite], want[finite]
    scale = want.max(dim=-1, keepdim=True).values.clamp(min=1e-30)
    out = dict(shape=dict(batch=args.batch, frames=args.frames, hop=hop, n_filters=F, average=args.average, iterations=iterations),
               rounds=args.rounds, calls_per_round=args.iters,
               **{name: round(median[name], 4) for name in legs},
               spread={name: round((max(v) - min(v)) / median[name], 4) for name, v in times.items()},
               per_iteration_ms=round((median["overlap_add_double_iterations_ms"] - median["overlap_add_ms"]) / max(1, iterations), 5),
               over_truncated_8=round(median["overlap_add_ms"] / median["truncated_8_ms"], 3),
               over_truncated_16=round(median["overlap_add_ms"] / median["truncated_16_ms"], 3),
               speedup_over_torch_ops=round(median["overlap_add_torch_ops_ms"] / median["overlap_add_ms"], 1),
               non_finite_frames=non_finite, max_difference_over_max_H=float(((got - want).abs() / scale).max()))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=172)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--average", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=None, help="16 for the truncated model, 8 with --overlap-add")
    ap.add_argument("--overlap-add", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise_analysis.py measures on the GPU; none is visible")
    hop, F = 512, 195
    if args.overlap_add:
        return overlap_add_legs(args, hop, F)
    if args.iterations is None:
        args.iterations = analysis.NOISE_ITERATIONS
    x = inputs(args.batch, args.frames, hop, F)

    def kernels(iterations=args.iterations):
        return ddsp.noise_analysis(x, hop, F, average=args.average, iterations=iterations)

    def torch_ops():
        return analysis._noise_torch(x, hop, F, args.average, args.iterations)[0]

    ms_kernel, got = timed(kernels, 3, args.iters)
    ms_zero, _ = timed(lambda: kernels(0), 3, args.iters)        # tables, measurement, rbar, p and H^0
    ms_double, _ = timed(lambda: kernels(2 * args.iterations), 3, args.iters)
    ms_torch, want = timed(torch_ops, 1, args.torch_iters)
    per_iteration = (ms_double - ms_kernel) / max(1, args.iterations)
    scale = want.max(dim=-1, keepdim=True).values.clamp(min=1e-30)
    out = dict(shape=dict(batch=args.batch, frames=args.frames, hop=hop, n_filters=F, average=args.average, iterations=args.iterations),
               kernel_ms=round(ms_kernel, 4), torch_ops_ms=round(ms_torch, 3), speedup=round(ms_torch / ms_kernel, 1),
               without_iterations_ms=round(ms_zero, 4), per_iteration_ms=round(per_iteration, 5),
               max_difference_over_max_H=float(((got - want).abs() / scale).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
