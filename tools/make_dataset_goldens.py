#!/usr/bin/env python3
"""Generate the training-set fixtures tests/golden/g26_* by running the REFERENCE's own dataset/audio_dataset.py on the CPU.

Needs a checkout of the reference (read-only): $DDSP_REFERENCE, default ../reference next to this repository.  The stubs of
tools/make_encoder_goldens.py are reused as they are (librosa.A_weighting, torchaudio.transforms.Resample, the seeded CREPE
weights behind the reference's torch.load); the resampler stub is widened to the 1-D input AudioData hands it, as torchaudio's
resample accepts any leading shape.  Four more patches, each a RESTATEMENT or a harness setting:
  * torchaudio.load(path)   -> scipy.io.wavfile's samples, scaled as normalize=True scales them (int16 / 32768, int32 / 2^31,
                               float32 as is), channels first [C, L] (ddsp_pytorch_amd.dataset.load_audio + pcm_to_float)
  * glob.glob               -> sorted paths (the reference's order is the file system's)
  * DataLoader              -> num_workers = 0
  * Tensor.cuda / Module.cuda -> the identity (the CPU capture of audio_dataset.py:83, 87)
and tqdm is the identity.  Everything else -- mono, hop-pad, geometry, unfold, the encoder padding and batching, the Encoder,
the concatenation and both cache files -- is the reference's code running.

The inputs are deterministic synthetic WAVs: their PCM arrays, rates and relative paths are stored in the fixtures, and the
tests write them out again.  Each fixture also records `spread64`, the largest |fp32 - fp64| of the CREPE probabilities over
its frames (the fp64 run is the reference's CREPE in double on the same frames).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_dataset_goldens.py
"""
import os
import sys
import tempfile
import types

import torch  # noqa: E402

_torch_load = torch.load                   # (make_encoder_goldens replaces it with the seeded CREPE loader)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_encoder_goldens as meg  # noqa: E402  (stubs, seeded CREPE loader, sys.path, MKL / mkldnn settings)

import glob  # noqa: E402

import numpy as np  # noqa: E402
from scipy.io import wavfile  # noqa: E402

from ddsp_pytorch_amd import dataset as ddsp_dataset  # noqa: E402
from crepe_seeded import top1_margin  # noqa: E402


class _Resample1d(meg._StubResample):
    def forward(self, waveform):
        shape = waveform.shape
        return super().forward(waveform.reshape(-1, shape[-1])).reshape(*shape[:-1], -1)


def _torchaudio_load(path):
    pcm, sr = ddsp_dataset.load_audio(path)
    return ddsp_dataset.pcm_to_float(pcm), sr


meg.torchaudio.load = _torchaudio_load
meg.torchaudio.transforms.Resample = _Resample1d
tqdm = types.ModuleType("tqdm")
tqdm.tqdm = lambda it, *a, **k: it
sys.modules["tqdm"] = tqdm
_glob = glob.glob
glob.glob = lambda pattern, *a, **k: sorted(_glob(pattern, *a, **k))

from dataset import audio_dataset as ref_dataset  # noqa: E402

_DataLoader = ref_dataset.DataLoader
ref_dataset.DataLoader = lambda *a, **k: _DataLoader(*a, **{**k, "num_workers": 0})
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self


class Conf:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def pcm(x, fmt):
    """float signal in (-1, 1) -> the stored sample format."""
    if fmt == "int16":
        return np.round(x * 32767).astype(np.int16)
    if fmt == "int32":
        return (np.round(x * 8388607).astype(np.int32) << 8)          # a 24-bit file as scipy returns it (left-justified)
    return x.astype(np.float32)


def signal(n, sr, channels, rng, f0):
    """channels x n: a harmonic tone per channel (slightly detuned) with a little noise."""
    return np.stack([meg.tone(n, sr, [f0 * (1 + 0.01 * c) * k for k in range(1, 5)], [0.3 / k for k in range(1, 5)], rng,
                              noise=0.01) for c in range(channels)], 1)


def capture(conf, files):
    """Write the WAVs, run the reference's PLHDataset (which runs AudioData), return its caches and the CREPE fp64 spread."""
    with tempfile.TemporaryDirectory() as d:
        for rel, sr, data in files:
            os.makedirs(os.path.dirname(os.path.join(d, rel)), exist_ok=True)
            wavfile.write(os.path.join(d, rel), sr, data)
        conf.data_dir = d
        frames = []
        hook = torch.nn.modules.module.register_module_forward_pre_hook(
            lambda m, a: frames.append((m, a[0].clone())) if type(m).__name__ == "Crepe" else None)
        try:
            plh = ref_dataset.PLHDataset(conf, clear=True)
        finally:
            hook.remove()
        audios = _torch_load(os.path.join(d, "audio_dataset.pth"), weights_only=True)
        cached = _torch_load(os.path.join(d, "plh_dataset.pth"), weights_only=True)
        assert all(torch.equal(cached[k], v) for k, v in plh.final.items())
        p32 = plh.final["probabilities"].reshape(-1, 360).numpy()
        p64 = np.concatenate([meg.ref_crepe_double(m)(x.double()).numpy() for m, x in frames])
        ok = ~np.isnan(p32)
        spread = float(np.max(np.abs(p32[ok] - p64[ok])))
    return plh.final, audios, spread


def save_case(name, conf, files):
    final, audios, spread = capture(conf, files)
    assert torch.equal(final["audio"], audios)
    m = top1_margin(final["probabilities"].numpy())
    decisive = float(np.mean(m > 40 * spread))
    print(f"  {name}: {len(audios)} examples of {audios.shape[1]} samples, {final['f0'].shape[1]} frames, spread64 {spread:.2e}, "
          f"decisive (> 40 x spread) {decisive:.3f}")
    assert decisive >= 0.9
    out = {"conf": np.array([conf.sample_rate, conf.n_fft, conf.hop_length, conf.batch_size]),
           "durations": np.array([conf.example_duration, conf.example_overlap]), "crepe_seed": np.int64(conf.seed),
           "n_files": np.int64(len(files)), "spread64": np.float64(spread)}
    for i, (rel, sr, data) in enumerate(files):
        out.update({f"file{i}_path": np.array(rel), f"file{i}_rate": np.int64(sr), f"file{i}_pcm": data})
    out.update({f"out_{k}": v.numpy() for k, v in final.items()})
    out["out_keys"] = np.array(list(final.keys()))
    meg.save(name, **out)


def g26_mix():
    """22.05 kHz conf (n_fft 1024, hop 256, 0.25 s examples every 0.1 s), batch 4: rates equal, above and below, 1-3 channels,
    int16 / int32 / float32, len % hop zero, odd and even, one file that yields exactly one example, and two decoys the
    reference's one-level glob does not match."""
    rng = np.random.default_rng(2626)
    conf = Conf(example_duration=0.25, example_overlap=0.1, sample_rate=22050, n_fft=1024, hop_length=256,
                crepe_capacity="tiny", batch_size=4, seed=26)
    meg.seed_crepe("tiny", conf.seed)
    hop = conf.hop_length
    files = [("a/equal_mono_i16.wav", 22050, pcm(signal(40 * hop, 22050, 1, rng, 196.0)[:, 0], "int16")),   # len % hop = 0
             ("a/one_example_stereo_i16.wav", 22050, pcm(signal(6001, 22050, 2, rng, 330.0), "int16")),
             ("b/above_stereo_i32.wav", 44100, pcm(signal(2 * 7039 - 1, 44100, 2, rng, 262.0), "int32")),
             ("b/below_3ch_f32.wav", 16000, pcm(signal(6578, 16000, 3, rng, 440.0), "float32")),
             ("top_level_decoy.wav", 22050, pcm(signal(100, 22050, 1, rng, 220.0)[:, 0], "int16")),
             ("a/b/too_deep_decoy.wav", 22050, pcm(signal(100, 22050, 1, rng, 220.0)[:, 0], "int16"))]
    # the conf-rate lengths: 10240 (pad 0), 6001 (pad 113, odd), 7039 (pad 127, odd), ceil(6578 * 441 / 320) = 9066 (pad 106, even)
    lens = [ddsp_dataset.resampled_length(d.shape[0], sr, 22050) for _, sr, d in files[:4]]
    assert [n % hop for n in lens] == [0, 113, 127, 106], lens
    save_case("g26_dataset_mix", conf, files)


def g26_default():
    """The default Config's geometry (44.1 kHz, n_fft 2048, hop 512, 2 s examples every 0.5 s) with tiny CREPE: one 48 kHz mono
    int16 file that yields exactly one example."""
    rng = np.random.default_rng(2627)
    conf = Conf(example_duration=2, example_overlap=0.5, sample_rate=44100, n_fft=2048, hop_length=512, crepe_capacity="tiny",
                batch_size=16, seed=27)
    meg.seed_crepe("tiny", conf.seed)
    files = [("voice/default_48k_mono_i16.wav", 48000, pcm(signal(100000, 48000, 1, rng, 247.0)[:, 0], "int16"))]
    save_case("g26_dataset_default", conf, files)


if __name__ == "__main__":
    for fn in sys.argv[1:] or ("g26_mix", "g26_default"):
        globals()[fn]()
