#!/usr/bin/env python
"""Times the voice allocation and the mixdown (voices.py): `allocate_voices` at the reference's dataset
shape, 8192 scores of 64 notes on 8 voices (one launch, one wavefront per score), and `mix_voices` at 16 scores x 8 voices x 2 s
at 44.1 kHz (one launch; plain, with a gate, and gated with a pan), beside the same mix written with torch operations on the same
device -- `view(B, V, L) * g` then `.sum(1)`, the gate's per-sample gains prepared outside the timed part.  The mix moves
(B V + B C) L 4 bytes, the least it can; the tool reports that over the median time as GB/s.  Device events on the stream,
warm-up first, `--repeats` repetitions of every timing and the whole measurement twice (`--runs`): the median, the smallest and
the largest of each run are printed in one JSON line, and whether the two forms of the mix agree within the mix's bound.  There
is no threshold: DESIGN.md section 10i records the figures.

    python tools/bench_voices.py [--scores 8192] [--notes 64] [--voices 8] [--batch 16] [--seconds 2.0] [--iters 200] [--repeats 5] [--runs 2]
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

RATE, HOP = 44100, 512


def score(B, N, device, seed=0):
    """B scores of N notes whose onsets are in order and whose notes overlap: about four sound at once"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    onset = torch.randint(0, 4, (B, N), generator=g).cumsum(1).int()
    frames = torch.randint(2, 12, (B, N), generator=g).int()
    pitch = torch.randint(40, 90, (B, N), generator=g).int()
    return ddsp.Notes(onset, frames, pitch, level=torch.rand((B, N), generator=g)).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scores", type=int, default=8192)
    ap.add_argument("--notes", type=int, default=64)
    ap.add_argument("--voices", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voices.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    V, B = args.voices, args.batch
    notes = score(args.scores, args.notes, dev)
    T = int(args.seconds * RATE) // HOP
    L = T * HOP
    g = torch.Generator(device="cuda").manual_seed(1)
    audio = torch.randn((B * V, L), device=dev, generator=g)
    rows = ddsp.allocate_voices(score(B, 24, dev, seed=2), V)
    active = ddsp.render_notes(rows, T, RATE, HOP)["voiced"]
    gain = torch.rand((B, V), device=dev, generator=g, dtype=torch.float64)
    pan = torch.rand((B, V), device=dev, generator=g, dtype=torch.float64) * 2 - 1
    out1, out2 = torch.empty((B, L), device=dev), torch.empty((B, 2, L), device=dev)
    gate = dict(active=active, hop_length=HOP, hold=2, fade=6)
    # the torch form's per-sample gains: the gated mix of a constant 1 per voice
    ones = torch.ones((B * V, L), device=dev)
    eye = torch.eye(V, device=dev, dtype=torch.float64)
    g_plain = gain.float()[:, :, None]
    g_gated = torch.stack([ddsp.mix_voices(ones, V, gain=(gain * eye[v]), **gate) for v in range(V)], dim=1)
    torch_mix = lambda table: (audio.view(B, V, L) * table).sum(1)             # noqa: E731
    runs = []
    for _ in range(args.runs):
        t = dict(allocate=timed(lambda: ddsp.allocate_voices(notes, V), 5, max(args.iters // 10, 10), args.repeats),
                 allocate_with_info=timed(lambda: ddsp.allocate_voices(notes, V, steal="quietest", return_info=True), 5,
                                          max(args.iters // 10, 10), args.repeats),
                 mix=timed(lambda: ddsp.mix_voices(audio, V, gain=gain, out=out1), 5, args.iters, args.repeats),
                 mix_gated=timed(lambda: ddsp.mix_voices(audio, V, gain=gain, out=out1, **gate), 5, args.iters, args.repeats),
                 mix_gated_pan=timed(lambda: ddsp.mix_voices(audio, V, gain=gain, pan=pan, out=out2, **gate), 5, args.iters, args.repeats),
                 mix_torch_ops=timed(lambda: torch_mix(g_plain), 5, args.iters, args.repeats),
                 mix_gated_torch_ops=timed(lambda: torch_mix(g_gated), 5, args.iters, args.repeats))
        runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
    med = lambda key: statistics.median(r[key][0] for r in runs)                # noqa: E731
    gbs = lambda C, key: round((B * V + B * C) * L * 4 / med(key) / 1e6, 1)     # noqa: E731
    found, info = ddsp.allocate_voices(notes, V, return_info=True)
    bound = (V + 6) * 2.0 ** -24
    agree = {}
    for name, ours, table in (("plain", ddsp.mix_voices(audio, V, gain=gain), g_plain),
                              ("gated", ddsp.mix_voices(audio, V, gain=gain, **gate), g_gated)):
        magnitude = (audio.view(B, V, L) * table).abs().sum(1)
        agree[name] = bool(((ours - torch_mix(table)).abs() <= 2 * bound * magnitude).all())      # (both sides round)
    print(json.dumps(dict(results=dict(
        allocate=dict(scores=args.scores, notes=args.notes, voices=V, stolen=int(info["stolen"].sum()), placed=int((info["voice"] >= 0).sum()),
                      notes_per_us=round(args.scores * args.notes / med("allocate_ms") / 1e3, 1)),
        mix=dict(scores=B, voices=V, samples=L, frames=T, active_share=round(float(active.float().mean()), 3),
                 mix_GBps=gbs(1, "mix_ms"), mix_gated_GBps=gbs(1, "mix_gated_ms"), mix_gated_pan_GBps=gbs(2, "mix_gated_pan_ms"),
                 torch_ops_over_one_launch=round(med("mix_torch_ops_ms") / med("mix_ms"), 1),
                 gated_torch_ops_over_one_launch=round(med("mix_gated_torch_ops_ms") / med("mix_gated_ms"), 1),
                 torch_ops_agree=agree),
        iters=args.iters, median_smallest_largest_per_run=runs))))


if __name__ == "__main__":
    main()
