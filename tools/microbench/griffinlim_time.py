#!/usr/bin/env python3
"""Griffin-Lim time per iteration on one MI355X: the HIP path (three launches per iteration) against the stock loop
(torchaudio 0.8.1's istft / stft / element-wise formulation, spectral._stock_loop) on the same device, at the reference's
shape (style_transfer.py: 30 s at 44.1 kHz, n_fft 2048, hop 256, 1 x 1025 x 5168) and on film_ui's grid (n_fft 512 / 1024 /
2048 x hop = n_fft / 2 .. n_fft / 16, a 10 s clip).  Optionally one end-to-end style_transfer at the reference's settings on a
30 s clip, split into LBFGS and Griffin-Lim time.

Per iteration = (time of n_iter = K + k0) - (time of n_iter = k0), over K, so the fixed cost of a call (checks, envelope,
transposes, final istft) cancels; each timing is the median of `--reps` calls after `--warmup` calls of the same shape, with
a device synchronise on both sides (torch.cuda.Event pairs).  Bytes per iteration are the HIP design's, from the
shapes, against the 6.3 TB/s copy bandwidth measured on this part.

    python tools/microbench/griffinlim_time.py [--out profiles/gl_time.json] [--quick] [--style]
(--quick: the reference's shape only, a few iterations: the run rocprofv3 --kernel-trace --stats profiles)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import spectral  # noqa: E402

COPY_BW = 6.3e12


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def hip_bytes(B, T, n_fft, hop):
    """HBM-level bytes of one HIP iteration: synthesis reads S (4 B / bin) and R, R_prev (8 + 8 B / bin) and writes the frames
    (4 B / sample); the overlap-add reads the frames and writes y; the analysis reads y (n_fft / hop times, absorbed by the
    caches: counted once) and writes R (8 B / bin)."""
    F = n_fft // 2 + 1
    bins, samples, L = B * T * F, B * T * n_fft, B * hop * (T - 1)
    return bins * (4 + 16) + samples * 4 + samples * 4 + L * 4 + L * 4 + bins * 8


def per_iter(spec, w, n_fft, hop, hip, k0, K, warmup, reps):
    B, F, T = spec.shape
    if hip:
        def run(n):
            return lambda: ddsp.griffinlim(spec, w, n_fft, hop, n_fft, 1.0, n, 0.99, None, False)
    else:
        S = spec.pow(1.0)
        ang = torch.stack([torch.ones_like(S), torch.zeros_like(S)], dim=-1)

        def run(n):
            return lambda: spectral._stock_loop(S, ang, w, n_fft, hop, n_fft, n, 0.99, None)
    t0 = timed(run(k0), warmup, reps)
    t1 = timed(run(k0 + K), warmup, reps)
    return (t1 - t0) / K, t0


def measure(B, T, n_fft, hop, K, warmup, reps):
    gen = torch.Generator().manual_seed(T + n_fft)
    spec = torch.rand(B, n_fft // 2 + 1, T, generator=gen).cuda()
    w = torch.hann_window(n_fft, device="cuda")
    hip_ms, hip_fixed = per_iter(spec, w, n_fft, hop, True, 2, K, warmup, reps)
    stock_ms, stock_fixed = per_iter(spec, w, n_fft, hop, False, 2, max(2, K // 4), max(1, warmup // 2), max(3, reps // 2))
    nbytes = hip_bytes(B, T, n_fft, hop)
    return {"B": B, "T": T, "n_fft": n_fft, "hop": hop, "hip_ms_per_iter": hip_ms, "stock_ms_per_iter": stock_ms,
            "speedup": stock_ms / hip_ms, "hip_call_ms_at_2_iters": hip_fixed, "stock_call_ms_at_2_iters": stock_fixed,
            "hip_bytes_per_iter": nbytes, "hip_GBps": nbytes / (hip_ms * 1e-3) / 1e9,
            "hip_frac_of_copy_bw": nbytes / (hip_ms * 1e-3) / COPY_BW}


def style_run(seconds):
    """style_transfer at the reference's settings (4096 features, LBFGS max_iter 1000, 5000 Griffin-Lim iterations) on a
    seeded harmonic content clip and a noisy style clip twice as long."""
    sr = 44100
    rng = np.random.default_rng(1)
    t = np.arange(int(seconds * sr)) / sr
    content = sum(0.3 / h * np.sin(2 * np.pi * 220 * h * t) for h in range(1, 10)) + 0.01 * rng.standard_normal(t.size)
    ts = np.arange(2 * t.size) / sr
    style = rng.standard_normal(ts.size) * np.exp(-(ts % 0.25) * 12) + 0.3 * np.sin(2 * np.pi * 523.25 * ts)
    stats = {}
    torch.manual_seed(0)
    y = ddsp.style_transfer(content.astype(np.float32), style.astype(np.float32), sample_rate=sr, device="cuda", stats=stats)
    return {"seconds": seconds, "out_len": int(y.shape[-1]), "closure_evals": len(stats["losses"]),
            "final_loss": stats["losses"][-1], "lbfgs_s": stats["lbfgs_s"], "griffinlim_s": stats["griffinlim_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gl_time.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--style", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ref_T = 1 + (30 * 44100) // 256
    if args.quick:
        spec = torch.rand(1, 1025, ref_T).cuda()
        w = torch.hann_window(2048, device="cuda")
        ddsp.griffinlim(spec, w, 2048, 256, 2048, 1.0, 10, 0.99, None, False)
        torch.cuda.synchronize()
        print("quick done")
        return
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "reps": args.reps,
           "timing": "median of torch.cuda.Event pairs around whole calls, per iteration = (t[n=2+K] - t[n=2]) / K",
           "clock": "not pinned: the default power management of a shared box (DESIGN §12)"}
    t0 = time.time()
    out["reference_shape"] = measure(1, ref_T, 2048, 256, 40, args.warmup, args.reps)
    print(json.dumps(out["reference_shape"]), flush=True)
    grid = []
    T10 = lambda hop: 1 + (10 * 44100) // hop  # noqa: E731
    for n_fft in (512, 1024, 2048):
        for factor in (2, 4, 8, 16):
            hop = n_fft // factor
            r = measure(1, T10(hop), n_fft, hop, 20, 2, 3)
            grid.append(r)
            print(json.dumps(r), flush=True)
    out["film_ui_grid_10s"] = grid
    if args.style:
        out["style_transfer_30s"] = style_run(30.0)
        print(json.dumps(out["style_transfer_30s"]), flush=True)
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
