#!/usr/bin/env python3
"""Training-set build rate on one GPU: PLHDataset over a seeded 10-minute corpus, CREPE tiny and full.

Corpus: 10 files of 60 s (six 44.1 kHz, four 48 kHz; stereo int16), written to a temporary folder.  Default Config geometry
(44.1 kHz, n_fft 2048, hop 512, 2 s examples every 0.5 s, batch 16) with seeded CREPE weights.  Reports:
  * end to end: PLHDataset(conf, clear=True) wall time -> examples/s and CREPE frames/s (pinned outputs, D2H and both cache
    files written, as in use);
  * the stages on their own, each synchronised: host decode (load_audio), H2D of the raw PCM, assembly (pcm_to_mono, resample,
    concatenation, make_examples per encoder batch) and the encoder;
  * the reference's flow as stock ops on the device (float32 upload, mean, pad + strided conv1d resampler, pad, unfold, cat,
    pad per batch) against the HIP assembly, with the same Encoder after it; its examples/s counts host decode, assembly
    (which includes its float32 upload) and encoder, to be read against `stages_examples_per_s`.

    python tools/microbench/dataset_time.py [--out profiles/dataset_build_time.json] [--minutes 10]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from scipy.io import wavfile  # noqa: E402

import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import dataset  # noqa: E402
from crepe_seeded import seeded_crepe_state, crepe_shapes  # noqa: E402


class Conf:
    example_duration, example_overlap, sample_rate, n_fft, hop_length, batch_size = 2, 0.5, 44100, 2048, 512, 16

    def __init__(self, data_dir, capacity):
        self.data_dir, self.crepe_capacity = data_dir, capacity
        self.crepe_weights = seeded_crepe_state(crepe_shapes(ddsp.Crepe(capacity)), 7)


def write_corpus(d, minutes):
    rng = np.random.default_rng(2026)
    n_files = max(1, int(minutes))
    for i in range(n_files):
        sr = 44100 if i % 5 < 3 else 48000
        t = np.arange(60 * sr) / sr
        f0 = 110.0 * 2 ** (rng.uniform(0, 3) + 0.2 * np.sin(2 * np.pi * 0.1 * t))
        phase = 2 * np.pi * np.cumsum(f0) / sr
        x = sum(0.3 / k * np.sin(k * phase) for k in range(1, 6)) + 0.01 * rng.standard_normal(t.shape)
        pcm = np.round(np.stack([x, 0.9 * x], 1) * 32767).astype(np.int16)
        os.makedirs(os.path.join(d, f"take{i // 4}"), exist_ok=True)
        wavfile.write(os.path.join(d, f"take{i // 4}", f"f{i:02d}.wav"), sr, pcm)


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def stages(conf, encoder, dev):
    """The device build's stages one at a time (same work as PLHDataset, synchronised between stages)."""
    files = dataset.find_audio_files(conf.data_dir)
    t0 = time.perf_counter()
    pcms = [dataset.load_audio(f) for f in files]
    t1 = sync()
    xs = [(torch.from_numpy(p).to(dev), sr) for p, sr in pcms]
    t2 = sync()
    duration, step = dataset.example_geometry(conf)
    parts, table, start, n = [], [], 0, 0
    rs = {}
    for (x, sr), f in zip(xs, files):
        mono = dataset.pcm_to_mono(x)
        if sr != conf.sample_rate:
            rs.setdefault(sr, ddsp.encoder.Resample(sr, conf.sample_rate).to(dev))
            mono = rs[sr](mono[None])[0]
        parts.append(mono)
        table.append((start, len(mono), dataset.hop_pad(len(mono), conf.hop_length)[0], n))
        start += len(mono)
        n += dataset.count_examples(f, len(mono), conf)
    y = torch.cat(parts)
    files_t = torch.tensor(table, dtype=torch.int64).to(dev)
    p = conf.n_fft - conf.hop_length
    chunks = []
    for e0 in range(0, n, conf.batch_size):
        E = min(conf.batch_size, n - e0)
        enc_in = torch.empty((E, duration + p), device=dev)
        dataset.make_examples(y, files_t, e0, E, duration, step, p, enc_in=enc_in)
        chunks.append(enc_in)
    t3 = sync()
    frames = 0
    with torch.no_grad():
        for enc_in in chunks:
            frames += encoder(enc_in)["f0"].shape[:2].numel()
    t4 = sync()
    pcm_bytes = sum(p.nbytes for p, _ in pcms)
    return dict(examples=n, crepe_frames=frames, host_decode_ms=1e3 * (t1 - t0), h2d_ms=1e3 * (t2 - t1), h2d_bytes=pcm_bytes,
                assembly_ms=1e3 * (t3 - t2), encoder_ms=1e3 * (t4 - t3)), pcms


def stock_assembly(conf, pcms, dev):
    """audio_dataset.py:28-59 and :86-90 as stock torch ops on the device (float32 [C, L] uploaded, as torchaudio.load returns)."""
    duration, step = dataset.example_geometry(conf)
    p = conf.n_fft - conf.hop_length
    floats = [(dataset.pcm_to_float(pc), sr) for pc, sr in pcms]          # (host scaling, untimed: torchaudio does it on load)
    t0 = sync()
    audios = []
    for y, sr in floats:
        y = y.to(dev)
        y = y[0] if y.shape[0] == 1 else y.mean(dim=0)
        if sr != conf.sample_rate:
            kernel, width, o, nw = ddsp.encoder.sinc_resample_kernel(sr, conf.sample_rate)
            L = y.shape[0]
            z = F.conv1d(F.pad(y[None], (width, width + o))[:, None], kernel.to(dev), stride=o)
            y = z.transpose(1, 2).reshape(-1)[:ddsp.encoder.resampled_length(L, sr, conf.sample_rate)]
        pad = len(y) % conf.hop_length
        audios.append(F.pad(y, (pad // 2, pad - pad // 2)).unfold(0, duration, step))
    audios = torch.cat(audios)
    chunks = [F.pad(audios[e0:e0 + conf.batch_size], (p // 2, p - p // 2)) for e0 in range(0, len(audios), conf.batch_size)]
    t1 = sync()
    return 1e3 * (t1 - t0), audios, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_build_time.json"))
    ap.add_argument("--minutes", type=float, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "corpus_minutes": args.minutes,
              "geometry": "44.1 kHz, n_fft 2048, hop 512, 2 s examples every 0.5 s, batch 16"}
    with tempfile.TemporaryDirectory() as d:
        write_corpus(d, args.minutes)
        for capacity in ("tiny", "full"):
            conf = Conf(d, capacity)
            encoder = ddsp.Encoder(conf).to(dev).eval()
            stages(conf, encoder, dev)                                     # warm-up: MIOpen's algorithm search, allocator
            st, pcms = stages(conf, encoder, dev)
            t0 = sync()
            plh = ddsp.PLHDataset(conf, clear=True)
            t1 = sync()
            wall = t1 - t0
            frames = plh.final["f0"].shape[0] * plh.final["f0"].shape[1]
            stock_assembly(conf, pcms, dev)                                # warm-up
            stock_ms, audios, chunks = stock_assembly(conf, pcms, dev)
            assert audios.shape[0] == len(plh)
            t2 = sync()
            with torch.no_grad():
                for c in chunks:
                    encoder(c)
            t3 = sync()
            result[capacity] = dict(
                end_to_end_s=wall, examples=len(plh), crepe_frames=frames, examples_per_s=len(plh) / wall,
                crepe_frames_per_s=frames / wall, stages=st,
                stage_share={k: st[k] / sum(st[j] for j in ("host_decode_ms", "h2d_ms", "assembly_ms", "encoder_ms"))
                             for k in ("host_decode_ms", "h2d_ms", "assembly_ms", "encoder_ms")},
                encoder_frames_per_s=1e3 * st["crepe_frames"] / st["encoder_ms"],
                # the stages alone (no pinned allocation, D2H or cache writes): the like-for-like figure for the stock flow's
                stages_examples_per_s=1e3 * len(plh) / sum(st[k] for k in ("host_decode_ms", "h2d_ms", "assembly_ms", "encoder_ms")),
                # (its assembly includes the float32 upload: twice the bytes of the int16 PCM)
                reference_flow_stock=dict(assembly_ms=stock_ms, encoder_ms=1e3 * (t3 - t2),
                                          examples_per_s=len(plh) / (1e-3 * (st["host_decode_ms"] + stock_ms) + (t3 - t2))))
            print(capacity, json.dumps(result[capacity]))
            del plh, encoder
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
