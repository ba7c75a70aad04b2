#!/usr/bin/env python3
"""Time of the YIN pitch front end on one MI355X, at two shapes:

  training set   16 rows of 88 064 samples at 44.1 kHz, n_fft 2048, hop 512   (a PLHDataset encode batch)
  live           one 4096-sample window, trimmed by a hop as AutoEncoder.forward_live trims it

  * `ddsp_yin_salience` alone: the launch through ctypes on the resampled audio and preallocated buffers;
  * the whole `F0Encoder.forward` with tracker 'yin' against tracker 'crepe' ('tiny' and 'full', the seeded weights of
    tests/crepe_seeded.py: the time does not depend on the values), same input, same process, the three taken in turn
    inside every repetition so that a drift of the clock meets all of them.

Every sample is ONE torch.cuda.Event pair around `inner` back-to-back calls, divided by `inner`; `--reps` samples after
`--warmup` untimed calls; median with 10th and 90th percentiles.  The ratios are formed per repetition (crepe / yin of the
same turn) and summarised the same way.  The input is seeded noise plus a tone: the time does not depend on it.

    python tools/microbench/yin_time.py [--out profiles/yin_salience.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd.encoder import _yin_table_on, YIN_OCTAVE_COST  # noqa: E402
from crepe_seeded import crepe_shapes, seeded_crepe_state  # noqa: E402


class Conf:
    sample_rate, n_fft, hop_length = 44100, 2048, 512

    def __init__(self, capacity="tiny"):
        self.crepe_capacity = capacity


SHAPES = (("training set", 16, 88064, 200, 10), ("live", 1, 4096 - 512, 200, 50))     # name, B, L, inner (kernel), inner (encoder)


def audio(B, L, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / 44100.0
    x = np.sin(2 * np.pi * 220.0 * t)[None] + 0.1 * rng.standard_normal((B, L))
    return torch.from_numpy(x.astype(np.float32)).cuda()


def sample_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summary(ts):
    return {"median": float(np.median(ts)), "p10": float(np.percentile(ts, 10)), "p90": float(np.percentile(ts, 90))}


def measure(name, B, L, inner_kernel, inner_encoder, warmup, reps):
    x = audio(B, L)
    encoders = {"yin": ddsp.F0Encoder(Conf(), tracker="yin").cuda()}
    for capacity in ("tiny", "full"):
        weights = seeded_crepe_state(crepe_shapes(ddsp.Crepe(capacity)), 1)
        encoders["crepe_" + capacity] = ddsp.F0Encoder(Conf(capacity), weights=weights).cuda()
    yin = encoders["yin"]
    y = yin.rs(x).contiguous()
    Lr = y.shape[1]
    hop = yin.resampled_hop(L, Lr)
    T = 1 + (Lr - 1024) // hop
    probs = torch.empty((B, T, 360), device="cuda")
    table = _yin_table_on(y.device, YIN_OCTAVE_COST)
    lib = ddsp._lib.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        rc = lib.ddsp_yin_salience(y.data_ptr(), table.data_ptr(), probs.data_ptr(), B, Lr, hop, T, stream)
        assert rc == 0, rc

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    kernel = [sample_ms(launch, inner_kernel) for _ in range(reps)]

    calls = {k: (lambda e=e: e(x)) for k, e in encoders.items()}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    turns = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            turns[k].append(sample_ms(fn, inner_encoder))
    res = {"shape": name, "B": B, "samples_44k": L, "samples_16k": int(Lr), "hop_16k": int(hop), "frames": int(T),
           "inner_kernel": inner_kernel, "inner_encoder": inner_encoder,
           "ddsp_yin_salience_ms": summary(kernel),
           "ddsp_yin_salience_us_per_frame": float(np.median(kernel)) * 1e3 / (B * T),
           "f0_encoder_forward_ms": {k: summary(v) for k, v in turns.items()}}
    for k in ("crepe_tiny", "crepe_full"):
        res[f"ratio_{k}_over_yin"] = summary(np.asarray(turns[k]) / np.asarray(turns["yin"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yin_salience.json"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"what": "ddsp_yin_salience alone, and F0Encoder.forward with tracker 'yin' against 'crepe' (tiny, full; seeded weights), "
                   "decoder 'argmax', on the same input in the same process",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": args.warmup, "reps": args.reps,
           "timing": "each sample: one torch.cuda.Event pair around `inner` back-to-back calls, divided by `inner`; "
                     "median, 10th and 90th percentile over the samples; ratios formed per repetition",
           "clock": "not pinned: the default power management of a shared box", "results": []}
    for shape in SHAPES:
        r = measure(*shape, args.warmup, args.reps)
        out["results"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
