#!/usr/bin/env python
"""Times the conditioning statistics and the auto-adjust (conditioning.py) at the reference's dataset
shape -- `conditioning_statistics` pooled over 8192 examples of 172 frames (2 s at 44.1 kHz, hop 512), and `fit_conditioning`
of a batch of 16 x 172 in both forms: with the source given (the live use, one launch) and measured per row on the way (the
offline use, three launches) -- beside the same arithmetic written with torch operations on the same device (torch.histc of the
selected frames, cumsum and searchsorted for the tables; searchsorted and gathers for the map).  Device events on the stream,
warm-up first, `--repeats` repetitions of every timing and the whole measurement twice (`--runs`): the median, the smallest and
the largest of each run are printed in one JSON line.  There is no threshold: DESIGN.md section 10d records the figures.

    python tools/bench_condition.py [--examples 8192] [--batch 16] [--iters 200] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from bench_align import timed                      # noqa: E402

LO, HI, BINS, Q = -4.0, 2.0, 4096, 64


def features(rows, frames, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    walk = torch.randn((rows, frames, 1), device="cuda", generator=g).mul_(0.15).cumsum(1)
    return dict(f0=torch.rand((rows, frames, 1), device="cuda", generator=g) * 400 + 80,
                normalized_cents=(0.5 + 0.1 * walk).clamp_(0, 1), loudness=(-1.5 + walk).clamp_(-3.9, 1.9),
                harmonicity=torch.rand((rows, frames, 1), device="cuda", generator=g))


def torch_statistics(z, confidence=0.0):
    """pooled: the table of Q + 1 quantiles, the mean pitch, the count (fp32 histogram, fp64 tables)"""
    l, n, h = z["loudness"], z["normalized_cents"], z["harmonicity"]
    on = torch.isfinite(l) & torch.isfinite(n) & (h >= confidence)
    counts = torch.histc(l[on], bins=BINS, min=LO, max=HI).double()
    cum = counts.cumsum(0)
    N = cum[-1]
    need = (torch.arange(Q + 1, device=l.device, dtype=torch.float64) * N / Q).clamp_(min=0.5)
    b = torch.searchsorted(cum, need).clamp_(max=BINS - 1)
    c = counts[b].clamp_(min=1.0)
    f = ((need - (cum[b] - counts[b])) / c).clamp_(0, 1)
    table = (LO + (b + f) * ((HI - LO) / BINS)).float()
    return table, n[on].double().mean(), N


def torch_fit(z, S, T, shift):
    """S, T [Q + 1]: the quantile map of the loudness and a pitch shift by `shift` octaves"""
    l = z["loudness"]
    k = (torch.searchsorted(S, l.reshape(-1).contiguous(), right=True) - 1).clamp_(0, Q - 1).reshape(l.shape)
    d = S[k + 1] - S[k]
    w = torch.where(d > 0, (l - S[k]) / d, torch.full_like(l, 0.5))
    mapped = T[k] + w * (T[k + 1] - T[k])
    mapped = torch.where(l < S[0], l + (T[0] - S[0]), torch.where(l >= S[Q], l + (T[Q] - S[Q]), mapped))
    return torch.ldexp(z["f0"], shift), z["normalized_cents"] + float(shift) * (1200.0 / 7180.0), mapped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--examples", type=int, default=8192)
    ap.add_argument("--frames", type=int, default=172)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_condition.py measures on the GPU; none is visible")
    data, clip = features(args.examples, args.frames, 0), features(args.batch, args.frames, 1)
    clip["loudness"] = clip["loudness"] - 1.0
    target = ddsp.conditioning_statistics(data)
    source = ddsp.conditioning_statistics(clip)
    S, T = source.loudness_quantiles[0].contiguous(), target.loudness_quantiles[0].contiguous()
    shift = torch.tensor(1, device="cuda", dtype=torch.int32)

    runs = []
    for _ in range(args.runs):
        t = dict(statistics=timed(lambda: ddsp.conditioning_statistics(data), 5, args.iters, args.repeats),
                 statistics_per_row=timed(lambda: ddsp.conditioning_statistics(data, per_row=True), 5, args.iters // 4, args.repeats),
                 statistics_torch_ops=timed(lambda: torch_statistics(data), 5, args.iters // 4, args.repeats),
                 fit_source_given=timed(lambda: ddsp.fit_conditioning(clip, target, source=source), 5, args.iters, args.repeats),
                 fit_measured=timed(lambda: ddsp.fit_conditioning(clip, target), 5, args.iters, args.repeats),
                 fit_torch_ops=timed(lambda: torch_fit(clip, S, T, shift), 5, args.iters, args.repeats))
        runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
    med = lambda key: statistics.median(r[key][0] for r in runs)                                  # noqa: E731
    frames = args.examples * args.frames
    table_distance = float((torch_statistics(data)[0] - target.loudness_quantiles[0]).abs().max())
    out = dict(shape=dict(examples=args.examples, frames=args.frames, batch=args.batch, bins=BINS, quantiles=Q),
               median_smallest_largest_per_run=runs,
               statistics_frames_per_us=round(frames / med("statistics_ms") / 1e3, 1),
               statistics_input_gb_per_s=round(12.0 * frames / med("statistics_ms") / 1e6, 1),
               statistics_torch_ops_over_kernels=round(med("statistics_torch_ops_ms") / med("statistics_ms"), 1),
               fit_torch_ops_over_one_launch=round(med("fit_torch_ops_ms") / med("fit_source_given_ms"), 1),
               largest_table_distance_to_torch_ops=table_distance, pooled_frames=int(target.frames))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
