#!/usr/bin/env python
"""Times the note extraction and the note render (notes.py) at a batch of 16 x 172 frames and at the
reference's dataset shape, 8192 x 172 (2 s at 44.1 kHz, hop 512): `extract_notes` with the tuning given (one launch; also at
hysteresis 0) and `render_notes` (one launch; plain, and with glide, attack, release and vibrato), beside the same arithmetic
written with torch operations on the same device -- for the extraction the nearest allowed note, note boundaries by comparison
with the neighbour, segment sums by index_add_ and the level by scatter_reduce_, the records scattered to their slots; for the
render a searchsorted per frame and gathers.  The torch form of the extraction has no hysteresis -- the recurrence has no torch
operation -- so the kernel is timed at hysteresis 0 as well, where both find the same notes.  Device events on the stream,
warm-up first, `--repeats` repetitions of every timing and the whole measurement twice (`--runs`): the median, the smallest and
the largest of each run are printed in one JSON line, and whether the two forms agree.  There is no threshold: DESIGN.md section
10f records the figures.

    python tools/bench_notes.py [--shapes 16x172,8192x172] [--iters 200] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd.notes import HOLD, NO_PITCH  # noqa: E402
from ddsp_pytorch_amd.tuning import ORIGIN, SEMITONE  # noqa: E402
from bench_align import timed                      # noqa: E402
from bench_tuning import MASK, features, positions  # noqa: E402

RATE, HOP = 44100, 512


def torch_extract(z, offset, root, steps, N):
    """hysteresis 0, no minimum length, every frame on -> onset, frames, pitch, detune, level [B, N] and count [B]"""
    down, up = steps
    n, loud = z["normalized_cents"][..., 0], z["loudness"][..., 0]
    B, T = n.shape
    dev = n.device
    v = positions(n) - 65536 * offset
    c = torch.div(v, SEMITONE, rounding_mode="floor")
    rel = torch.remainder(c - root, 12)
    lo, hi = c - down[rel], c + 1 + up[rel]
    note = torch.where(v - lo * SEMITONE <= hi * SEMITONE - v, lo, hi)
    start = torch.ones_like(note, dtype=torch.bool)
    start[:, 1:] = note[:, 1:] != note[:, :-1]
    ident = start.reshape(-1).long().cumsum(0) - 1
    L = torch.zeros(B * T, device=dev, dtype=torch.int64).index_add_(0, ident, torch.ones_like(ident))
    total = torch.zeros(B * T, device=dev, dtype=torch.int64).index_add_(0, ident, v.reshape(-1))
    level = torch.full((B * T,), float("-inf"), device=dev).scatter_reduce_(0, ident, loud.reshape(-1), "amax")
    slot = (start.long().cumsum(1) - 1)[start] + (torch.arange(B, device=dev)[:, None] * N).expand(B, T)[start]
    first = ident[start.reshape(-1)]
    pitch = note[start]
    out = [torch.full((B * N,), fill, device=dev, dtype=torch.int32) for fill in (-1, 0, NO_PITCH, 0)]
    out[0][slot] = torch.arange(T, device=dev, dtype=torch.int32).expand(B, T)[start]
    out[1][slot] = L[first].int()
    out[2][slot] = pitch.int()
    out[3][slot] = (-torch.div(2 * (pitch * SEMITONE * L[first] - total[first]) + L[first], 2 * L[first], rounding_mode="floor")).int()
    lv = torch.full((B * N,), float("nan"), device=dev)
    lv[slot] = level[first]
    return [o.view(B, N) for o in out] + [lv.view(B, N), start.sum(1).int()]


def torch_render(notes, T, floor=0.0, default_level=1.0):
    """detune kept, the notes' own grid, no glide, envelope or vibrato -> position, owner, normalized_cents, f0, loudness"""
    B, N = notes.onset.shape
    dev = notes.onset.device
    used = torch.arange(N, device=dev)[None] < notes.count[:, None]
    onset = torch.where(used, notes.onset.long(), torch.full_like(notes.onset, 1 << 40, dtype=torch.int64))
    t = torch.arange(T, device=dev)[None].expand(B, T).contiguous()
    star = torch.searchsorted(onset, t, right=True) - 1
    i = star.clamp(min=0)
    frames, pitch, detune = notes.frames.long(), notes.pitch.long(), notes.detune.long()
    valid = (frames >= 1) & (pitch >= 0) & (pitch <= 127) & (detune.abs() <= 1 << 30) & used
    centre = pitch * SEMITONE + detune + 65536 * notes.offset.long()[:, None]
    has = (star >= 0) & valid.gather(1, i)
    pos = torch.where(has, centre.gather(1, i), torch.where((star < 0) & valid[:, :1], centre[:, :1], torch.full_like(t, HOLD)))
    on = has & (t - onset.gather(1, i) < frames.gather(1, i))
    c = pos.double() / 65536.0
    lv = notes.level.gather(1, i).double()
    lv = torch.where(lv.isnan(), torch.full_like(lv, default_level), lv)
    loud = torch.where(on, floor + (lv - floor), torch.full_like(lv, floor)).float()
    return pos, torch.where(on, star, torch.full_like(star, -1)).int(), ((c - ORIGIN) / 7180.0).float(), \
        (440.0 * torch.exp2((c - 6900.0) / 1200.0)).float(), loud


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x172,8192x172")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_notes.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    down = torch.tensor([next(k for k in range(12) if (MASK >> ((c - k) % 12)) & 1) for c in range(12)], device=dev)
    up = torch.tensor([next(k for k in range(12) if (MASK >> ((c + 1 + k) % 12)) & 1) for c in range(12)], device=dev)
    full = dict(glide=3, attack=2, release=4, vibrato_cents=25.0, vibrato_delay=4, vibrato_ramp=8)
    results = []
    for shape in args.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        iters = max(args.iters * 16 // max(B, 16), 10)
        z = features(B, T, B)
        z["loudness"] = torch.randn((B, T, 1), device=dev, generator=torch.Generator(device="cuda").manual_seed(B + 1))
        tuning = ddsp.tuning_statistics(z)
        off, root = tuning.offset[0].long(), tuning.root[0].long()
        notes = ddsp.extract_notes(z, tuning, hysteresis=0.0)
        runs = []
        for _ in range(args.runs):
            t = dict(extract=timed(lambda: ddsp.extract_notes(z, tuning), 5, iters, args.repeats),
                     extract_no_hysteresis=timed(lambda: ddsp.extract_notes(z, tuning, hysteresis=0.0), 5, iters, args.repeats),
                     extract_torch_ops=timed(lambda: torch_extract(z, off, root, (down, up), T), 5, iters, args.repeats),
                     render=timed(lambda: ddsp.render_notes(notes, T, RATE, HOP), 5, iters, args.repeats),
                     render_full=timed(lambda: ddsp.render_notes(notes, T, RATE, HOP, **full), 5, iters, args.repeats),
                     render_torch_ops=timed(lambda: torch_render(notes, T), 5, iters, args.repeats))
            runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
        med = lambda key: statistics.median(r[key][0] for r in runs)                              # noqa: E731
        theirs = torch_extract(z, off, root, (down, up), T)
        ours = [notes.onset, notes.frames, notes.pitch, notes.detune, notes.level, notes.count]
        out = ddsp.render_notes(notes, T, RATE, HOP, return_info=True)
        pos, owner, cents, f0, loud = torch_render(notes, T)
        results.append(dict(shape=dict(rows=B, frames=T), iters=iters, median_smallest_largest_per_run=runs,
                            notes=int(notes.count.sum()),
                            extract_frames_per_us=round(B * T / med("extract_ms") / 1e3, 1),
                            render_frames_per_us=round(B * T / med("render_ms") / 1e3, 1),
                            extract_torch_ops_over_one_launch=round(med("extract_torch_ops_ms") / med("extract_no_hysteresis_ms"), 1),
                            render_torch_ops_over_one_launch=round(med("render_torch_ops_ms") / med("render_ms"), 1),
                            torch_ops_agree=dict(records=all(bool(torch.equal(a, b)) for a, b in zip(theirs[:4] + theirs[5:], ours[:4] + ours[5:])),
                                                 level=bool(torch.equal(theirs[4].nan_to_num(9.0), ours[4].nan_to_num(9.0))),
                                                 position=bool(torch.equal(pos, out["position"])), owner=bool(torch.equal(owner, out["owner"])),
                                                 cents=bool(torch.equal(cents, out["normalized_cents"][..., 0])),
                                                 loudness=bool(torch.equal(loud, out["loudness"][..., 0])))))
    print(json.dumps(dict(results=results)))


if __name__ == "__main__":
    main()
