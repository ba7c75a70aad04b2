#!/usr/bin/env python
"""Times the time alignment (analysis.dtw_align / align_controls) at the reference's dataset shape -- 16 clips of 172 frames (2 s
at 44.1 kHz, hop 512) aligned with 16 clips of 215 frames, 180 harmonics, 195 noise bands, so D = 32 + 8 + 2 = 42 features -- four
ways on the same device: the HIP launch alone (outputs and workspace allocated once), the public dtw_align on prepared features,
align_controls (features of both dicts, then dtw_align), and the package's own torch-op path (one anti-diagonal at a time; what
CPU tensors and out-of-range shapes take).  Device events on the stream, warm-up first, `--repeats` repetitions of every timing,
and the whole measurement twice (`--runs`): the median, the smallest and the largest of each run are printed in one JSON line.
There is no threshold: DESIGN.md section 14d records the figures.

    python tools/bench_align.py [--batch 16] [--iters 200] [--torch-iters 2] [--repeats 5] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp                    # noqa: E402
from ddsp_pytorch_amd import analysis, _lib        # noqa: E402
from bench_morph import inputs                     # noqa: E402


def timed(fn, warmup, iters, repeats):
    """-> (median ms per call over `repeats` timings of `iters` calls, their smallest and largest, the last result)."""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            out = fn()
        stop.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(stop) / iters)
    return statistics.median(ms), min(ms), max(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py measures on the GPU; none is visible")
    sr, H, F, T_a, T_b, B, penalty = 44100, 180, 195, 172, 215, args.batch, 0.01
    ctrl_a, ctrl_b = inputs(B, T_a, H, F, 0), inputs(B, T_b, H, F, 1)
    x_a, x_b = ddsp.control_features(ctrl_a, sr).contiguous(), ddsp.control_features(ctrl_b, sr).contiguous()
    D = x_a.shape[-1]
    L = _lib.lib()
    nbytes = L.ddsp_dtw_workspace_bytes(B, T_a, T_b)
    pos_a, pos_b = torch.empty((B, T_a), device="cuda"), torch.empty((B, T_a), device="cuda")
    path = torch.empty((B, T_a + T_b - 1, 2), dtype=torch.int32, device="cuda")
    length, cost = torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), device="cuda")
    work = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(L.ddsp_dtw_align(x_a.data_ptr(), x_b.data_ptr(), pos_a.data_ptr(), pos_b.data_ptr(), path.data_ptr(), length.data_ptr(),
                                    cost.data_ptr(), work.data_ptr(), nbytes, B, T_a, T_b, D, T_a, 0, penalty, 0.0, stream), "ddsp_dtw_align")
        return path

    def public():
        return ddsp.dtw_align(x_a, x_b, penalty=penalty, return_path=True)

    def controls():
        return ddsp.align_controls(ctrl_a, ctrl_b, sr, penalty=penalty, return_path=True)

    def features():
        return ddsp.control_features(ctrl_a, sr), ddsp.control_features(ctrl_b, sr)

    def torch_ops():
        return analysis._dtw_torch(x_a, x_b, None, penalty)

    runs = []
    for _ in range(args.runs):
        t = dict(launch=timed(launch, 5, args.iters, args.repeats), dtw_align=timed(public, 5, args.iters, args.repeats),
                 align_controls=timed(controls, 5, args.iters // 4, args.repeats), control_features=timed(features, 5, args.iters // 4, args.repeats),
                 torch_ops=timed(torch_ops, 1, args.torch_iters, args.repeats))
        runs.append({k + "_ms": [round(v, 4) for v in t[k][:3]] for k in t})
        want = t["torch_ops"][3]
        same = bool(torch.equal(t["dtw_align"][3][2], want[0]) and torch.equal(t["dtw_align"][3][4], want[2]) and torch.equal(path, want[0]))
    med = lambda key: statistics.median(r[key][0] for r in runs)                                  # noqa: E731
    out = dict(shape=dict(batch=B, frames_a=T_a, frames_b=T_b, features=D, n_harmonics=H, n_noise_filters=F, sample_rate=sr, penalty=penalty),
               median_smallest_largest_per_run=runs, cells_per_us_launch=round(B * T_a * T_b / med("launch_ms") / 1e3, 1),
               torch_ops_over_launch=round(med("torch_ops_ms") / med("launch_ms"), 1),
               outside_the_launch_share_of_align_controls=round(1.0 - med("launch_ms") / med("align_controls_ms"), 3),
               features_share_of_align_controls=round(med("control_features_ms") / med("align_controls_ms"), 3),
               kernel_and_torch_ops_agree=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
