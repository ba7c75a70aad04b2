#!/usr/bin/env python
"""Times the overlap-add filtered noise (noise_forward / noise_backward with overlap_add=True) next to the truncated forms the
same calls take without the flag, at the two headline shapes: 512 x 500 frames of hop 128 / 65 bands and 512 x 375 frames of
hop 512 / 195 bands, in-kernel draws, workspace allocation included (as the Python layer pays it).  Device events on the stream
bracket back-to-back calls after warm-up; every figure is taken `--repeats` times and printed as median and (max - min) / median.
For the first shape the synthesis step of bench.py (oscillator bank, 100 harmonics, + noise accumulated into its buffer) is timed
with either form, which gives the mode's share of that step.  Prints one JSON line.  There is no threshold: DESIGN.md section 5a
records the times.

`--live` times the real-time callback instead (GraphedLiveDecoder.run: host arrays in, one hipGraph replay, host audio out; 4 frames
per call, 512-wide MLPs and GRU as bench.py's live_callback_ms) with the truncated noise against the overlap-add stream
(`delayed=True`), at hop 128 / 65 bands / 16 kHz and at the reference's default hop 512 / 195 bands / 44.1 kHz.  Both decoders live
in one process and alternate: each repeat times `--calls` callbacks of one, then of the other; median of the repeats' medians and
their spread, next to the callback's deadline frames * hop / sample rate.

    python tools/bench_noise_ola.py [--iters 200] [--repeats 5] [--batch 512]
    python tools/bench_noise_ola.py --live [--calls 100] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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


LIVE_SHAPES = [(128, 65, 16000, 100), (512, 195, 44100, 180)]            # hop, bands, sample rate, harmonics
LIVE_FRAMES = 4


def live(calls, repeats):
    out = []
    rng = np.random.default_rng(3)
    z = {"normalized_cents": rng.uniform(0, 1, (1, LIVE_FRAMES, 1)).astype(np.float32),
         "loudness": rng.uniform(-1, 1, (1, LIVE_FRAMES, 1)).astype(np.float32),
         "f0": rng.uniform(200, 400, (1, LIVE_FRAMES, 1)).astype(np.float32)}
    for hop, F, rate, harmonics in LIVE_SHAPES:
        conf = type("LiveConf", (), dict(n_harmonics=harmonics, n_noise_filters=F, sample_rate=rate, hop_length=hop, decoder_mlp_units=512,
                                         decoder_mlp_layers=3, decoder_gru_units=512, decoder_gru_layers=1))
        torch.manual_seed(0)
        forms = {"truncated": ddsp.GraphedLiveDecoder(ddsp.Decoder(conf, noise_rng="device").cuda().eval(), LIVE_FRAMES),
                 "overlap_add_delayed": ddsp.GraphedLiveDecoder(ddsp.Decoder(conf, noise_rng="device", noise_overlap_add=True).cuda().eval(),
                                                                LIVE_FRAMES, delayed=True)}
        medians = {name: [] for name in forms}
        for rep in range(repeats + 1):                            # (the first round warms both up and is dropped)
            for name, dec in forms.items():
                lat = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    audio = dec.run(z)
                    lat.append(1e3 * (time.perf_counter() - t0))
                assert audio.shape == (LIVE_FRAMES * hop,) and np.isfinite(audio).all()
                if rep:
                    medians[name].append(statistics.median(lat))
        row = dict(shape=dict(frames=LIVE_FRAMES, hop=hop, n_filters=F, sample_rate=rate, n_harmonics=harmonics),
                   deadline_ms=round(1e3 * LIVE_FRAMES * hop / rate, 3), delay_samples=forms["overlap_add_delayed"].delay,
                   delay_ms=round(1e3 * forms["overlap_add_delayed"].delay / rate, 3))
        for name, ms in medians.items():
            med = statistics.median(ms)
            row[name] = dict(ms=round(med, 4), spread=round((max(ms) - min(ms)) / med, 4))
        row["ratio"] = round(row["overlap_add_delayed"]["ms"] / row["truncated"]["ms"], 3)
        out.append(row)
        del forms
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--live", action="store_true", help="time the real-time callback, truncated against delayed overlap-add")
    ap.add_argument("--calls", type=int, default=100, help="--live: callbacks per repeat and form")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise_ola.py measures on the GPU; none is visible")
    if args.live:
        return live(args.calls, args.repeats)
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
