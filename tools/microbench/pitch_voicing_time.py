#!/usr/bin/env python3
"""Time of `pitch_voicing` on one MI355X: the launch alone (ddsp_pitch_voicing through ctypes on preallocated buffers) and
the whole Python call (output allocation and checks included), for fill 'hold' and 'interpolate', at the training shape
(B 16, T 172) and on one long row (B 1, T 51 680: ten minutes at 44.1 kHz, hop 512).

Each figure is the median of `--reps` torch.cuda.Event pairs after `--warmup` calls, with its 10th and 90th percentiles.
The inputs are seeded: a periodicity that walks through both thresholds, a quantised pitch, a loudness around the gate.

    python tools/microbench/pitch_voicing_time.py [--out profiles/pitch_voicing_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd.encoder import VOICING_FILLS  # noqa: E402

SHAPES = (("training batch", 16, 172), ("one long row", 1, 51680))
SILENCE = 0.4


def inputs(B, T, seed=0):
    rng = np.random.default_rng(seed)

    def reflected_walk(step):                                  # a random walk folded into [0, 1]
        return np.abs((np.cumsum(rng.normal(0, step, (B, T)), axis=1) + 0.25) % 2.0 - 1.0)

    p = reflected_walk(0.07)
    n = np.round((0.3 + 0.4 * reflected_walk(0.03)) * 20) / 20
    f0 = 100.0 + 400.0 * n + rng.random((B, T))
    loud = SILENCE + 0.2 * np.sin(np.cumsum(rng.normal(0, 0.05, (B, T)), axis=1))
    return [torch.from_numpy(x.astype(np.float32))[..., None].cuda() for x in (f0, p, n, loud)]


def event_ms(fn, warmup, reps):
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
    return {"median_ms": float(np.median(ts)), "p10_ms": float(np.percentile(ts, 10)), "p90_ms": float(np.percentile(ts, 90))}


def measure(B, T, fill, warmup, reps):
    f0, p, n, loud = inputs(B, T)
    L = ddsp._lib.lib()
    out = torch.empty((3, B, T), device="cuda")
    voiced = torch.empty((B, T), device="cuda", dtype=torch.uint8)
    state = torch.empty((B, 3), device="cuda")
    nbytes = L.ddsp_pitch_voicing_workspace_bytes(B, T)
    work = torch.empty(max(nbytes, 4), device="cuda", dtype=torch.uint8)
    code = VOICING_FILLS.index(fill)

    def launch():
        rc = L.ddsp_pitch_voicing(f0.data_ptr(), n.data_ptr(), p.data_ptr(), loud.data_ptr(), None, out[0].data_ptr(),
                                  out[1].data_ptr(), voiced.data_ptr(), out[2].data_ptr(), state.data_ptr(), work.data_ptr(),
                                  B, T, 3, 3, 0.31, 0.19, SILENCE, code, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def call():
        return ddsp.pitch_voicing(f0, p, n, loud, silence=SILENCE, fill=fill, return_state=True)

    res = {"B": B, "T": T, "fill": fill, "workspace_bytes": int(nbytes), "launch": event_ms(launch, warmup, reps),
           "python_call": event_ms(call, warmup, reps)}
    got = call()
    res["voiced_share"] = float(got[1].float().mean())
    res["frames_changed"] = float((got[0] != f0).float().mean())
    res["launch_ns_per_frame_of_a_row"] = res["launch"]["median_ms"] * 1e6 / T
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_voicing_time.json"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"what": "ddsp_pitch_voicing: the launch alone and the whole pitch_voicing call; windows 3 and 3, thresholds 0.31 / 0.19, "
                   "loudness gate on",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "reps": args.reps,
           "timing": "torch.cuda.Event pairs around single calls: median, 10th and 90th percentile",
           "clock": "not pinned: the default power management of a shared box", "results": []}
    for name, B, T in SHAPES:
        for fill in ("hold", "interpolate"):
            r = measure(B, T, fill, args.warmup, args.reps)
            r["shape"] = name
            out["results"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
