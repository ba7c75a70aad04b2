#!/usr/bin/env python
"""Times the tuning statistics and the pitch snap (tuning.py) at the reference's dataset shape --
`tuning_statistics` pooled over 8192 examples of 172 frames (2 s at 44.1 kHz, hop 512), and `tune_pitch` of a batch of 16 x 172
in both forms: with the statistics given (one launch) and measured per row on the way (three launches) -- beside the same
arithmetic written with torch operations on the same device (int64 positions, bincount, a matrix product for the 100 costs;
for the snap the nearest allowed note, note boundaries by comparison with the neighbour, segment sums by index_add).  The
torch form of the snap has no hysteresis -- the recurrence has no torch operation -- so the kernel is timed at hysteresis 0 as
well, where both compute the same notes.  Device events on the stream, warm-up first, `--repeats` repetitions of every timing
and the whole measurement twice (`--runs`): the median, the smallest and the largest of each run are printed in one JSON line.
There is no threshold: DESIGN.md section 10e records the figures.

    python tools/bench_tuning.py [--examples 8192] [--batch 16] [--iters 200] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd.tuning import OCTAVE, ORIGIN, SEMITONE  # noqa: E402
from bench_align import timed                      # noqa: E402

MASK = 0xAB5


def features(rows, frames, seed):
    """melodies: a random walk over semitones, 23 cents sharp, with vibrato and jitter"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    steps = (torch.rand((rows, frames, 1), device="cuda", generator=g) < 0.08) * torch.randint(-3, 4, (rows, frames, 1), device="cuda", generator=g)
    t = torch.arange(frames, device="cuda", dtype=torch.float32)[None, :, None]
    cents = (57.0 + steps.cumsum(1)) * 100.0 + 23.0 + 15.0 * torch.sin(0.7 * t) + 4.0 * torch.randn((rows, frames, 1), device="cuda", generator=g)
    n = ((cents - ORIGIN) / 7180.0).float()
    return dict(normalized_cents=n, f0=(10.0 * torch.exp2((7180.0 * n.double() + 1997.3794084376191) / 1200.0)).float(),
                harmonicity=torch.rand((rows, frames, 1), device="cuda", generator=g))


def positions(n):
    return torch.round((7180.0 * n.double() + ORIGIN) * 65536.0).long()


def torch_statistics(z, tables, confidence=0.0):
    """pooled: offset, root, profile, count"""
    deviation, allowed = tables
    n, h = z["normalized_cents"], z["harmonicity"]
    on = (n.abs() <= 4.0) & (h >= confidence)
    cell = torch.div(torch.remainder(positions(n[on]) + 32768, OCTAVE), 65536, rounding_mode="floor")
    H = torch.bincount(cell, minlength=1200)
    offset = torch.argmin(deviation @ H.view(12, 100).sum(0)) - 50
    cells = torch.remainder(100 * torch.arange(12, device=n.device)[:, None] + offset + torch.arange(-50, 50, device=n.device)[None], 1200)
    profile = H[cells].sum(1)
    return offset, torch.argmax(allowed @ profile), profile, H.sum()


def torch_snap(z, offset, root, steps):
    """hysteresis 0, vibrato kept, no glide: every note's mean onto its pitch"""
    down, up = steps
    n, f0 = z["normalized_cents"][..., 0], z["f0"][..., 0]
    B, T = n.shape
    v = positions(n) - 65536 * offset
    c = torch.div(v, SEMITONE, rounding_mode="floor")
    rel = torch.remainder(c - root, 12)
    lo, hi = c - down[rel], c + 1 + up[rel]
    note = torch.where(v - lo * SEMITONE <= hi * SEMITONE - v, lo, hi)
    start = torch.ones_like(note, dtype=torch.bool)
    start[:, 1:] = note[:, 1:] != note[:, :-1]
    ident = start.reshape(-1).long().cumsum(0) - 1
    count = torch.zeros(B * T, device=n.device, dtype=torch.int64).index_add_(0, ident, torch.ones_like(ident))
    total = torch.zeros(B * T, device=n.device, dtype=torch.int64).index_add_(0, ident, v.reshape(-1))
    L = count[ident].view(B, T)
    d = torch.div(2 * (note * SEMITONE * L - total[ident].view(B, T)) + L, 2 * L, rounding_mode="floor")
    return (f0.double() * torch.exp2(d.double() / (65536.0 * 1200.0))).float(), n + (d.double() / (65536.0 * 7180.0)).float(), note


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
        raise SystemExit("bench_tuning.py measures on the GPU; none is visible")
    data, clip = features(args.examples, args.frames, 0), features(args.batch, args.frames, 1)
    dev = torch.device("cuda")
    o = torch.arange(-50, 50, device=dev)[:, None]
    d = torch.arange(100, device=dev)[None]
    deviation = torch.minimum(torch.remainder(d - o, 100), torch.remainder(o - d, 100))
    r, p = torch.arange(12, device=dev)[:, None], torch.arange(12, device=dev)[None]
    allowed = (MASK >> torch.remainder(p - r, 12)) & 1
    down = torch.tensor([next(k for k in range(12) if (MASK >> ((c - k) % 12)) & 1) for c in range(12)], device=dev)
    up = torch.tensor([next(k for k in range(12) if (MASK >> ((c + 1 + k) % 12)) & 1) for c in range(12)], device=dev)
    tuning = ddsp.tuning_statistics(data)
    off, root = tuning.offset[0].long(), tuning.root[0].long()

    runs = []
    for _ in range(args.runs):
        t = dict(statistics=timed(lambda: ddsp.tuning_statistics(data), 5, args.iters, args.repeats),
                 statistics_per_row=timed(lambda: ddsp.tuning_statistics(data, per_row=True), 5, args.iters // 4, args.repeats),
                 statistics_torch_ops=timed(lambda: torch_statistics(data, (deviation, allowed)), 5, args.iters // 4, args.repeats),
                 snap_given=timed(lambda: ddsp.tune_pitch(clip, tuning), 5, args.iters, args.repeats),
                 snap_given_no_hysteresis=timed(lambda: ddsp.tune_pitch(clip, tuning, hysteresis=0.0), 5, args.iters, args.repeats),
                 snap_measured=timed(lambda: ddsp.tune_pitch(clip), 5, args.iters, args.repeats),
                 snap_torch_ops=timed(lambda: torch_snap(clip, off, root, (down, up)), 5, args.iters, args.repeats))
        runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
    med = lambda key: statistics.median(r[key][0] for r in runs)                                  # noqa: E731
    frames = args.examples * args.frames
    theirs = torch_statistics(data, (deviation, allowed))
    ours, info = ddsp.tune_pitch(clip, tuning, hysteresis=0.0, return_info=True)
    f0_t, n_t, note_t = torch_snap(clip, off, root, (down, up))
    out = dict(shape=dict(examples=args.examples, frames=args.frames, batch=args.batch),
               median_smallest_largest_per_run=runs,
               statistics_frames_per_us=round(frames / med("statistics_ms") / 1e3, 1),
               statistics_input_gb_per_s=round(8.0 * frames / med("statistics_ms") / 1e6, 1),
               statistics_torch_ops_over_kernels=round(med("statistics_torch_ops_ms") / med("statistics_ms"), 1),
               snap_torch_ops_over_one_launch=round(med("snap_torch_ops_ms") / med("snap_given_no_hysteresis_ms"), 1),
               offset=int(tuning.offset[0]), root=int(tuning.root[0]), pooled_frames=int(tuning.frames[0]),
               torch_ops_agree=dict(offset=int(theirs[0]) == int(tuning.offset[0]), root=int(theirs[1]) == int(tuning.root[0]),
                                    profile=bool(torch.equal(theirs[2], tuning.profile[0])),
                                    notes=bool(torch.equal(note_t.int(), info["notes"])),
                                    cents=bool(torch.equal(n_t, ours["normalized_cents"][..., 0]))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
