#!/usr/bin/env python3
"""Pitch decode timings on one GPU: ddsp_pitch_viterbi + ddsp_pitch_centered against the same recurrence written in stock
torch ops on the same device.  Device events after warm-up, medians with their spread (10th .. 90th percentile), the two
versions alternating call by call; one JSON document on stdout (and --out).

  training  B 16, T 172: the probabilities of one training batch (16 clips x 2 s at 44.1 kHz, hop 512)
  live      B 1, T 4: the frames of one 4096-sample live window (AutoEncoder.live_window: 3584 samples -> 4 CREPE frames)
  share     the decode's part of one F0Encoder forward (decoder='viterbi') at the training batch, CREPE 'tiny' and 'full'

    python tools/microbench/pitch_decode_time.py [--quick] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ddsp_pytorch_amd as ddsp  # noqa: E402
from crepe_seeded import seeded_crepe_state, crepe_shapes  # noqa: E402
from pitch_decode_reference import track  # noqa: E402

BAND = 11


class Cfg:
    sample_rate, n_fft, hop_length = 44100, 2048, 512

    def __init__(self, capacity):
        self.crepe_capacity = capacity


def stock_viterbi(p, log_a):
    """The recurrence of ddsp_pitch_viterbi in stock torch ops on p's device: a handful of launches per frame, then a
    dependent gather per frame for the walk back."""
    T = p.shape[1]
    e = torch.log(torch.clamp_min(p, 1e-30))
    v = e[:, 0]
    back = []
    for t in range(1, T):
        cand = F.pad(v, (BAND, BAND), value=float("-inf")).unfold(1, 2 * BAND + 1, 1) + log_a
        best, arg = cand.max(dim=-1)
        back.append(arg)
        v = best + e[:, t]
        if t % 8 == 0:
            v = v - v.max(dim=-1, keepdim=True).values
    s = v.argmax(dim=-1)
    path = [s]
    for arg in reversed(back):
        s = s + arg.gather(1, s[:, None])[:, 0] - BAND
        path.append(s)
    return torch.stack(path[::-1], dim=1).unsqueeze(-1)


def stock_centered(center, p):
    idx = center + torch.arange(-4, 5, device=p.device)
    w = p.gather(-1, idx.clamp(0, 359)) * ((idx >= 0) & (idx < 360))
    off = 20 * (w * torch.arange(-4, 5, device=p.device)).sum(-1, keepdim=True) / w.sum(-1, keepdim=True)
    base = (center * 20).float()
    cents = base + 1997.3794084376191 + off
    return 10 * 2 ** (cents / 1200), p.gather(-1, center), (base + off) / 7180.


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": len(ms)}


def compare(B, T, rounds):
    p = torch.from_numpy(np.stack([track(100 + r, T)[0] for r in range(B)])).cuda()
    log_a = ddsp.encoder.viterbi_log_transition().cuda()

    def hip():
        return ddsp.pitch_centered(ddsp.pitch_viterbi(p), p)

    def stock():
        return stock_centered(stock_viterbi(p, log_a), p)

    for _ in range(3):
        hip(), stock()
    torch.cuda.synchronize()
    same = float((ddsp.pitch_viterbi(p) == stock_viterbi(p, log_a)).float().mean())
    t_hip, t_stock = [], []
    for r in range(rounds):                                  # alternate, and swap the order every round
        for which in (("hip", "stock") if r % 2 == 0 else ("stock", "hip")):
            (t_hip if which == "hip" else t_stock).append(event_ms(hip if which == "hip" else stock))
    out = {"B": B, "T": T, "hip": summary(t_hip), "stock": summary(t_stock), "paths_equal_share": same}
    out["speedup_of_medians"] = out["stock"]["median_ms"] / out["hip"]["median_ms"]
    out["hip_faster_beyond_both_spreads"] = bool(out["hip"]["p90_ms"] < out["stock"]["p10_ms"])
    # the kernels alone, without the Python wrapper's allocations and casts
    L = ddsp._lib.lib()
    bins = torch.empty((B, T), device="cuda", dtype=torch.int32)
    o = torch.empty((3, B, T), device="cuda")

    def kernels():
        L.ddsp_pitch_viterbi(p.data_ptr(), log_a.data_ptr(), None, None, bins.data_ptr(), None, B, T, None)
        L.ddsp_pitch_centered(p.data_ptr(), bins.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None, B * T, None)

    kernels()
    out["hip_kernels_only"] = summary([event_ms(kernels) for _ in range(rounds)])
    return out


def share(capacity, rounds):
    w = seeded_crepe_state(crepe_shapes(ddsp.Crepe(capacity)), 0)
    x = 0.3 * torch.randn(16, 88200 + 1536, device="cuda")
    res = {}
    probs = None
    for decoder in ("argmax", "viterbi"):
        enc = ddsp.F0Encoder(Cfg(capacity), weights=w, decoder=decoder).cuda()
        for _ in range(3):
            probs = enc(x)[2]
        res[f"forward_{decoder}"] = summary([event_ms(lambda: enc(x)) for _ in range(rounds)])
    res["decode"] = summary([event_ms(lambda: ddsp.pitch_centered(ddsp.pitch_viterbi(probs), probs)) for _ in range(rounds)])
    res["frames"] = [int(probs.shape[0]), int(probs.shape[1])]
    res["decode_share_of_forward"] = res["decode"]["median_ms"] / res["forward_viterbi"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="few rounds (for a profiler run)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    rounds = 10 if a.quick else 60
    res = {"what": "ddsp_pitch_viterbi + ddsp_pitch_centered (hip) against the same recurrence in stock torch ops (stock), "
                   "tools/microbench/pitch_decode_time.py",
           "device": torch.cuda.get_device_name(0), "unit": "milliseconds per call, device events",
           "training": compare(16, 172, rounds), "live": compare(1, 4, rounds * 4),
           "share_tiny": share("tiny", rounds), "share_full": share("full", max(rounds // 3, 5))}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
