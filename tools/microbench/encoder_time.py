#!/usr/bin/env python3
"""Encoder timings on one GPU (device events, warm-up, >= 0.5 s windows); one JSON document on stdout (and --out).

  offline   Encoder.forward at the reference's training batch: 16 clips x 2 s at 44.1 kHz plus the AutoEncoder padding
            (89 736 samples, 172 frames each), CREPE 'tiny' and 'full' (seeded weights: speed does not depend on them)
  live      AutoEncoder.forward_live with the default Config (180 harmonics, 195 bands, hop 512, CREPE 'full' and 'tiny'):
            median / p99 over >= 200 callbacks against the 2048 / 44100 s = 46.4 ms deadline (rt/synth.py:53-55)
  ab        the encoder's stock-torch composition on the GPU vs the HIP kernels: pad / ReLU / BN / pool vs the fused epilogue
            (every CREPE layer of the offline batch), torch.stft + log + mean vs ddsp_loudness, conv1d resampling vs ddsp_resample
  roofline  loudness and resampler: compulsory HBM bytes (input read once, output written once) / time against 8 TB/s

    python tools/microbench/encoder_time.py [--quick] [--out FILE]
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

HBM_BYTES_PER_S = 8.0e12
DEADLINE_MS = 2048 / 44100 * 1e3


class Cfg:
    sample_rate, n_fft, hop_length = 44100, 2048, 512
    n_harmonics, n_noise_filters = 180, 195
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 512, 3, 512, 1

    def __init__(self, capacity):
        self.crepe_capacity = capacity


def weights(capacity):
    return seeded_crepe_state(crepe_shapes(ddsp.Crepe(capacity)), 0)


def time_ms(fn, min_s=0.5, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < min_s * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        n += 1
    return total / n


def offline(capacity, min_s):
    enc = ddsp.Encoder(Cfg(capacity), weights=weights(capacity)).cuda()
    x = 0.3 * torch.randn(16, 88200 + 1536, device="cuda")
    ms = time_ms(lambda: enc(x), min_s)
    frames = enc(x)["f0"].shape[1] * 16
    return {"ms": ms, "frames": frames, "frames_per_s": frames / ms * 1e3}


def live(capacity, n_calls):
    ae = ddsp.AutoEncoder(Cfg(capacity), weights=weights(capacity)).cuda().eval()
    hidden = torch.randn(1, 1, 512, device="cuda")
    buf = (0.3 * np.random.default_rng(0).standard_normal(4096)).astype(np.float32)
    for _ in range(10):
        ae.forward_live(buf, hidden)
    t = []
    for _ in range(n_calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ae.forward_live(buf, hidden)                       # ends in a D2H copy: synchronous
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(t)), "p99_ms": float(np.percentile(t, 99)), "calls": n_calls, "deadline_ms": DEADLINE_MS}


def ab(min_s):
    out = {}
    L = ddsp._lib.lib()
    # epilogue: every layer of 'full' and 'tiny' at the offline batch (16 x 172 frames)
    for cap in ("tiny", "full"):
        m = ddsp.Crepe(cap).cuda().eval()
        N = 16 * 172
        Lc = 256
        stock, fused = 0.0, 0.0
        for i, (conv, bn) in enumerate(m.layers()):
            C = conv.out_channels
            y = torch.randn(N, C, Lc, device="cuda")
            last = i == 5
            o = torch.empty((N, (Lc // 2) * C) if last else (N, C, Lc // 2 + 63), device="cuda")

            def hip():
                L.ddsp_crepe_epilogue(y.data_ptr(), conv.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                      bn.weight.data_ptr(), bn.bias.data_ptr(), o.data_ptr(), N, C, Lc, int(last), None)

            def torch_path():
                z = F.max_pool2d(bn(F.relu(y[..., None] + conv.bias[None, :, None, None])), (2, 1), (2, 1))
                if last:
                    return z.permute(0, 2, 1, 3).reshape(N, -1)
                return F.pad(z, (0, 0, 31, 32))

            with torch.no_grad():
                stock += time_ms(torch_path, min_s / 6)
                fused += time_ms(hip, min_s / 6)
            Lc //= 2
        out[f"epilogue_{cap}"] = {"stock_ms": stock, "hip_ms": fused}
    # loudness at the offline batch
    enc = ddsp.LoudnessEncoder(Cfg("tiny")).cuda()
    x = 0.3 * torch.randn(16, 88200 + 1536, device="cuda")

    def stock_loud():
        s = torch.stft(x, 2048, 512, center=False, return_complex=True, window=torch.ones(2048, device="cuda")).permute(0, 2, 1)
        d = torch.log10(torch.abs(s) + 1e-20) * 20
        d += enc.a_weight
        return torch.mean(d / 90 + 1, dim=-1, keepdim=True)

    lh = time_ms(lambda: enc(x), min_s)
    out["loudness"] = {"stock_ms": time_ms(stock_loud, min_s), "hip_ms": lh,
                       "bytes": x.numel() * 4 + 16 * 172 * 4}
    out["loudness"]["hbm_fraction"] = out["loudness"]["bytes"] / (lh * 1e-3) / HBM_BYTES_PER_S
    # ... and through the pair kernel (two frames per transform, equalised): every size at hop n_fft / 4 on the same batch;
    # 1024 / 256 is the 16 kHz 'full' configuration
    out["loudness_pair"] = {}
    for n_fft in (64, 128, 256, 512, 1024):
        class CfgN:
            sample_rate, hop_length = 16000, n_fft // 4
        CfgN.n_fft = n_fft
        encn = ddsp.LoudnessEncoder(CfgN).cuda()
        ones = torch.ones(n_fft, device="cuda")

        def stock_loudn():
            s = torch.stft(x, n_fft, n_fft // 4, center=False, return_complex=True, window=ones).permute(0, 2, 1)
            d = torch.log10(torch.abs(s) + 1e-20) * 20
            d += encn.a_weight
            return torch.mean(d / 90 + 1, dim=-1, keepdim=True)

        out["loudness_pair"][str(n_fft)] = {"stock_ms": time_ms(stock_loudn, min_s / 2), "hip_ms": time_ms(lambda: encn(x), min_s / 2),
                                            "frames": 16 * (1 + (x.shape[1] - n_fft) // (n_fft // 4))}
    # resampler
    rs = ddsp.encoder.Resample(44100, 16000).cuda()
    yr = rs(x)

    def stock_rs():
        xp = F.pad(x, (rs.width, rs.width + rs.orig))
        return F.conv1d(xp[:, None], rs.kernel, stride=rs.orig).transpose(1, 2).reshape(16, -1)[..., :yr.shape[1]]

    rh = time_ms(lambda: rs(x), min_s)
    out["resample"] = {"stock_ms": time_ms(stock_rs, min_s), "hip_ms": rh, "bytes": x.numel() * 4 + yr.numel() * 4,
                       "taps_per_output": rs.ntaps}
    out["resample"]["hbm_fraction"] = out["resample"]["bytes"] / (rh * 1e-3) / HBM_BYTES_PER_S
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="short windows (for a profiler run)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    min_s = 0.1 if a.quick else 0.5
    calls = 20 if a.quick else 200
    res = {"device": torch.cuda.get_device_name(0)}
    for cap in ("tiny", "full"):
        res[f"offline_{cap}"] = offline(cap, min_s)
        res[f"live_{cap}"] = live(cap, calls)
    res["ab"] = ab(min_s)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
