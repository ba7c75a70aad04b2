#!/usr/bin/env python
"""Times the note expression and the expressive render (notes.py) at a batch of 16 x 172 frames and at the
reference's dataset shape, 8192 x 172 (2 s at 44.1 kHz, hop 512): `note_expression` (one launch) and
`render_notes(..., expression=e)` (one launch; of the notes as found, and of the notes transposed and played 1.5 times as long with
the ends kept), beside the plain render and beside the same arithmetic written with torch operations on the same device -- a
searchsorted per frame and gathers, the time map in int64 tensor operations.  The protocol of tools/bench_notes.py: device events
on the stream, warm-up first, `--repeats` repetitions of every timing and the whole measurement twice (`--runs`); the median, the
smallest and the largest of each run are printed in one JSON line, and whether the two forms agree.  There is no threshold:
DESIGN.md section 10g records the figures.

    python tools/bench_expression.py [--shapes 16x172,8192x172] [--iters 200] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd.tuning import SEMITONE       # noqa: E402
from bench_align import timed                      # noqa: E402
from bench_notes import torch_render               # noqa: E402
from bench_tuning import features, positions       # noqa: E402

RATE, HOP = 44100, 512


def owners(notes, T):
    """-> (i* clamped to 0, whether i* exists and is valid, k = t - onset, the onsets with the unused slots pushed away)"""
    B, N = notes.onset.shape
    dev = notes.onset.device
    used = torch.arange(N, device=dev)[None] < notes.count[:, None]
    onset = torch.where(used, notes.onset.long(), torch.full_like(notes.onset, 1 << 40, dtype=torch.int64))
    t = torch.arange(T, device=dev)[None].expand(B, T).contiguous()
    star = torch.searchsorted(onset, t, right=True) - 1
    i = star.clamp(min=0)
    frames, pitch, detune = notes.frames.long(), notes.pitch.long(), notes.detune.long()
    valid = (frames >= 1) & (pitch >= 0) & (pitch <= 127) & (detune.abs() <= 1 << 30) & used
    return i, star, (star >= 0) & valid.gather(1, i), t - onset.gather(1, i), onset


def torch_expression(z, notes):
    """-> bend int32 [B, T], owner int32 [B, T]"""
    n = z["normalized_cents"][..., 0]
    i, star, has, k, _ = owners(notes, n.shape[1])
    own = has & (k < notes.frames.long().gather(1, i)) & (n.abs() <= 4.0)
    centre = notes.pitch.long() * SEMITONE + notes.detune.long() + 65536 * notes.offset.long()[:, None]
    bend = (positions(n) - centre.gather(1, i)).clamp(-(1 << 31), (1 << 31) - 1)
    return torch.where(own, bend, torch.zeros_like(bend)).int(), torch.where(own, star, torch.full_like(star, -1)).int()


def torch_render_expr(notes, e, T, keep_attack=0, keep_release=0):
    """the plain render of bench_notes.torch_render, then the source's curves (source = None, both amounts 1)
    -> position, owner, normalized_cents, loudness"""
    pos, owner, _, _, loud = torch_render(notes, T)
    i, _, _, k, onset = owners(notes, T)
    B, N = notes.onset.shape
    Ts, Ns = e.bend.shape[1], e.onset.shape[1]
    frames = notes.frames.long().gather(1, i)
    nxt = onset.gather(1, (i + 1).clamp(max=N - 1))
    length = torch.where(i + 1 < notes.count.long().clamp(0, N)[:, None], torch.minimum(frames, nxt - onset.gather(1, i)), frames)
    j = i.clamp(max=max(Ns - 1, 0))
    Ls, so = e.frames.long().gather(1, j), e.onset.long().gather(1, j)
    ok = (owner >= 0) & (k < length) & (i < e.count.long().clamp(0, Ns)[:, None]) & (Ls >= 1) & (so >= 0) & (so + Ls <= Ts)
    Ls, so, k, length = (torch.where(ok, x, torch.full_like(x, fill)) for x, fill in ((Ls, 1), (so, 0), (k, 0), (length, 1)))
    a = torch.minimum(torch.minimum(torch.full_like(Ls, keep_attack), Ls), length)
    r = torch.minimum(torch.minimum(torch.full_like(Ls, keep_release), Ls - a), length - a)
    middle = (k >= a) & (k < length - r)
    D = torch.where(middle, length - a - r + 1, torch.ones_like(Ls))
    x = torch.where(middle, (k - a + 1) * (Ls - a - r + 1), torch.zeros_like(Ls))
    q = torch.where(k < a, k, torch.where(middle, a - 1 + torch.div(x, D, rounding_mode="floor"), Ls - (length - k)))
    f = torch.div(torch.remainder(x, D) << 16, D, rounding_mode="floor")
    f = torch.where((q < 0) | (q >= Ls - 1), torch.zeros_like(f), f)
    q = torch.minimum(q.clamp(min=0), Ls - 1)
    at = so + q
    nxt = (at + 1).clamp(max=Ts - 1)
    b0 = e.bend.long().gather(1, at)
    bend = b0 + torch.where(f > 0, ((e.bend.long().gather(1, nxt) - b0) * f + 32768) >> 16, torch.zeros_like(b0))
    pos = pos + torch.where(ok, bend, torch.zeros_like(bend))
    sl = e.level.gather(1, j).double()
    l0 = e.loudness.gather(1, at).double()
    l = torch.where(f > 0, l0 + (e.loudness.gather(1, nxt).double() - l0) * (f.double() / 65536.0), l0)
    loud = torch.where(ok & ~sl.isnan(), (loud.double() + (l - sl)).float(), loud)
    c = pos.double() / 65536.0
    return pos, owner, ((c - ddsp.tuning.ORIGIN) / 7180.0).float(), loud


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x172,8192x172")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_expression.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    results = []
    for shape in args.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        iters = max(args.iters * 16 // max(B, 16), 10)
        z = features(B, T, B)
        z["loudness"] = torch.randn((B, T, 1), device=dev, generator=torch.Generator(device="cuda").manual_seed(B + 1))
        tuning = ddsp.tuning_statistics(z)
        notes = ddsp.extract_notes(z, tuning)
        e = ddsp.note_expression(z, notes, return_owner=True)
        # an edit: up a third, every note 1.5 times as long (a later note still cuts an earlier one), the ends kept
        edited = notes.transpose(4)._with(frames=torch.where(notes._used(), notes.frames + notes.frames // 2, notes.frames))
        keep = dict(keep_attack=2, keep_release=2)
        runs = []
        for _ in range(args.runs):
            t = dict(expression=timed(lambda: ddsp.note_expression(z, notes), 5, iters, args.repeats),
                     expression_torch_ops=timed(lambda: torch_expression(z, notes), 5, iters, args.repeats),
                     render_plain=timed(lambda: ddsp.render_notes(notes, T, RATE, HOP), 5, iters, args.repeats),
                     render_expression=timed(lambda: ddsp.render_notes(notes, T, RATE, HOP, expression=e), 5, iters, args.repeats),
                     render_expression_edited=timed(lambda: ddsp.render_notes(edited, T, RATE, HOP, expression=e, **keep), 5, iters, args.repeats),
                     render_expression_torch_ops=timed(lambda: torch_render_expr(edited, e, T, 2, 2), 5, iters, args.repeats))
            runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
        med = lambda key: statistics.median(r[key][0] for r in runs)                              # noqa: E731
        bend, owner = torch_expression(z, notes)
        agree = dict(bend=bool(torch.equal(bend, e.bend)), owner=bool(torch.equal(owner, e.owner)))
        for name, played, kw in (("as_found", notes, dict()), ("edited", edited, keep)):
            out = ddsp.render_notes(played, T, RATE, HOP, expression=e, return_info=True, **kw)
            pos, own, cents, loud = torch_render_expr(played, e, T, kw.get("keep_attack", 0), kw.get("keep_release", 0))
            agree[name] = dict(position=bool(torch.equal(pos, out["position"])), owner=bool(torch.equal(own, out["owner"])),
                               cents=bool(torch.equal(cents, out["normalized_cents"][..., 0])),
                               loudness_max_abs=float((loud - out["loudness"][..., 0]).abs().max()))
        results.append(dict(shape=dict(rows=B, frames=T), iters=iters, median_smallest_largest_per_run=runs, notes=int(notes.count.sum()),
                            expression_frames_per_us=round(B * T / med("expression_ms") / 1e3, 1),
                            render_expression_frames_per_us=round(B * T / med("render_expression_ms") / 1e3, 1),
                            expression_torch_ops_over_one_launch=round(med("expression_torch_ops_ms") / med("expression_ms"), 1),
                            render_torch_ops_over_one_launch=round(med("render_expression_torch_ops_ms") / med("render_expression_edited_ms"), 1),
                            torch_ops_agree=agree))
    print(json.dumps(dict(results=results)))


if __name__ == "__main__":
    main()
