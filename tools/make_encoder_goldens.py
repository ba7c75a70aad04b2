#!/usr/bin/env python3
"""Generate the encoder fixtures tests/golden/g19_* .. g25_* by running the REFERENCE's own encoder / autoencoder on the CPU.

Needs a checkout of the reference (read-only): $DDSP_REFERENCE, default ../reference next to this repository.  The reference's
model/autoencoder/encoder.py imports librosa and torchaudio, which this environment does not have, so two small stubs go
into sys.modules first -- both RESTATEMENTS, whose parity with the real libraries cannot be pinned here:
  * librosa.A_weighting                  -> ddsp_pytorch_amd.encoder.a_weighting (the published formula, min_db = -80)
  * torchaudio.transforms.Resample(o, n) -> the Hann-windowed sinc kernel of ddsp_pytorch_amd.encoder.sinc_resample_kernel
                                            applied as torchaudio applies it (pad (width, width + orig), strided conv1d,
                                            ceil(new L / orig) outputs); identity at equal rates
and, for model/autoencoder/autoencoder.py, `train.train` is a stub module exposing the reference's own
model.autoencoder.decoder.Decoder (what train/train.py:9 imports).  Everything else -- hop arithmetic, normalisation,
framing, CREPE, argmax, cents, the loudness pipeline, padding / trimming, the decoder -- is the reference's code running.

CREPE weights: the pretrained ones belong to their authors and stay out of the repository; the reference's torch.load of
crepe/pretrained/{capacity}.pth is patched to return the seeded weights of tests/crepe_seeded.py.  The live callbacks (G25)
patch torch.Tensor.cuda to the identity for the CPU capture (autoencoder.py:28 moves the window to the GPU).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_encoder_goldens.py
"""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DDSP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import math  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import ddsp_pytorch_amd as ddsp  # noqa: E402
from crepe_seeded import seeded_crepe_state, crepe_shapes, top1_margin  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)
# CPU convolutions on the native (im2col + BLAS) path rather than oneDNN's ISA-dependent kernels: the tests pin the same
torch.backends.mkldnn.enabled = False


# ---- stubs --------------------------------------------------------------------------------------------------------------
class _StubResample(torch.nn.Module):
    def __init__(self, orig_freq=16000, new_freq=16000):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if self.orig_freq != self.new_freq:
            kernel, self.width, self.o, self.n = ddsp.encoder.sinc_resample_kernel(orig_freq, new_freq)
            self.register_buffer("kernel", kernel, persistent=False)

    def forward(self, waveform):
        if self.orig_freq == self.new_freq:
            return waveform
        B, L = waveform.shape
        x = F.pad(waveform, (self.width, self.width + self.o))
        y = F.conv1d(x[:, None], self.kernel, stride=self.o).transpose(1, 2).reshape(B, -1)
        return y[..., :int(math.ceil(self.n * L / self.o))]


librosa = types.ModuleType("librosa")
librosa.A_weighting = lambda f, min_db=-80.0: ddsp.encoder.a_weighting(f, min_db)
torchaudio = types.ModuleType("torchaudio")
torchaudio.transforms = types.ModuleType("torchaudio.transforms")
torchaudio.transforms.Resample = _StubResample
sys.modules.update({"librosa": librosa, "torchaudio": torchaudio, "torchaudio.transforms": torchaudio.transforms})

from model.autoencoder import encoder as ref_encoder  # noqa: E402
from model.autoencoder.decoder import Decoder as RefDecoder  # noqa: E402

train_stub = types.ModuleType("train.train")
train_stub.Decoder = RefDecoder
sys.modules["train.train"] = train_stub
from model.autoencoder import autoencoder as ref_autoencoder  # noqa: E402

_SEEDED = {}


def _seeded_load(path, *a, **k):
    capacity = os.path.splitext(os.path.basename(str(path)))[0]
    return _SEEDED[capacity]


torch.load = _seeded_load


def seed_crepe(capacity, seed):
    """Install the seeded weights for the reference's torch.load; the fixture stores only the seed (the tests redraw them)."""
    _SEEDED[capacity] = seeded_crepe_state(crepe_shapes(ddsp.Crepe(capacity)), seed)
    return {"crepe_seed": np.int64(seed)}


class Conf:
    def __init__(self, sample_rate, n_fft, hop_length, crepe_capacity="tiny", **kw):
        self.sample_rate, self.n_fft, self.hop_length, self.crepe_capacity = sample_rate, n_fft, hop_length, crepe_capacity
        self.__dict__.update(kw)


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def tone(n, sr, f0s, amps, rng, noise=0.0, phase=True):
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + (rng.uniform(0, 2 * np.pi) if phase else 0.0)) for f, a in zip(f0s, amps))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


def loud_rows(n, sr, rng):
    return np.stack([0.3 * rng.standard_normal(n).astype(np.float32),                       # white noise
                     tone(n, sr, [220 * k for k in range(1, 9)], [0.5 / k for k in range(1, 9)], rng),   # harmonic tone
                     tone(n, sr, [440.0], [1e-4], rng),                                       # -80 dB tone
                     np.zeros(n, np.float32)])                                                # silence


def g19():
    rng = np.random.default_rng(1919)
    out = {}
    for tag, (sr, n_fft, hop, n) in {"a": (44100, 2048, 512, 8192), "b": (16000, 1024, 256, 5000)}.items():
        enc = ref_encoder.LoudnessEncoder(Conf(sr, n_fft, hop))
        x = loud_rows(n, sr, rng)
        loud = enc(torch.from_numpy(x)).numpy()
        loud64 = np.asarray(ref_encoder.LoudnessEncoder.forward(_Double(enc), torch.from_numpy(x).double()))
        out.update({f"{tag}_x": x, f"{tag}_loudness": loud, f"{tag}_a_weight": enc.a_weight.numpy(),
                    f"{tag}_spread64": np.float64(np.max(np.abs(loud - loud64))), f"{tag}_conf": np.array([sr, n_fft, hop])})
    save("g19_loudness", **out)


class _Double:
    """The reference LoudnessEncoder's attributes with a float64 a_weight (the fp64 yardstick of the fp32 fixture)."""

    def __init__(self, enc):
        self.n_fft, self.hop_length, self.a_weight = enc.n_fft, enc.hop_length, enc.a_weight.double()


def g20():
    rng = np.random.default_rng(2020)
    out = {}
    for tag, sr in {"a": 44100, "b": 48000}.items():
        x = rng.standard_normal((2, 9001)).astype(np.float32) * 0.3
        x[1] = tone(9001, sr, [300.0, 3000.0, 7000.0], [0.4, 0.2, 0.1], rng)
        y = _StubResample(sr, 16000)(torch.from_numpy(x)).numpy()
        out.update({f"{tag}_x": x, f"{tag}_y": y, f"{tag}_rate": np.int64(sr)})
    save("g20_resample", **out)


def f0_capture(enc, x):
    """Reference F0Encoder.forward on x, plus its CREPE input frames and the fp64 spread of the probabilities."""
    frames = []
    h = enc.model.register_forward_pre_hook(lambda m, a: frames.append(a[0].clone()))
    f, harm, p, c = enc(torch.from_numpy(x.copy()))      # (at equal rates the reference normalises its input in place)
    h.remove()
    m64 = ref_crepe_double(enc.model)
    p64 = m64(frames[0].double()).reshape(p.shape).numpy()
    ok = ~np.isnan(p.numpy())
    spread = float(np.max(np.abs(p.numpy()[ok] - p64[ok]))) if ok.any() else 0.0
    return dict(f0=f.numpy(), harmonicity=harm.numpy(), probabilities=p.numpy(), normalized_cents=c.numpy(), spread64=np.float64(spread))


def ref_crepe_double(model):
    import copy
    return copy.deepcopy(model).double()


def g21():
    w = seed_crepe("tiny", 21)
    conf = Conf(44100, 2048, 512)
    enc = ref_encoder.F0Encoder(conf)
    rng = np.random.default_rng(2121)
    clips = np.stack([tone(16384, 44100, [196.0 * k for k in range(1, 6)], [0.5 / k for k in range(1, 6)], rng, noise=0.01),
                      tone(16384, 44100, [523.25, 1046.5], [0.4, 0.1], rng, noise=0.02)])
    live = tone(3584, 44100, [330.0, 660.0], [0.5, 0.2], rng, noise=0.01)[None]
    silent = np.zeros((1, 3584), np.float32)
    out = dict(w)
    for tag, x in (("clips", clips), ("live", live), ("silent", silent)):
        r = f0_capture(enc, x)
        out.update({f"{tag}_x": x, **{f"{tag}_{k}": v for k, v in r.items()}})
        if tag != "silent":
            m = top1_margin(r["probabilities"])
            print(f"  g21 {tag}: min margin {m.min():.2e}, spread64 {r['spread64']:.2e}, "
                  f"decisive (> 40 x spread) {np.mean(m > 40 * r['spread64']):.3f}")
            assert np.mean(m > 40 * r["spread64"]) >= 0.9
    assert np.all(np.isnan(out["silent_probabilities"])) and np.all(out["silent_normalized_cents"] == 0)
    save("g21_f0_tiny", **out)


def g22():
    w = seed_crepe("full", 22)
    enc = ref_encoder.F0Encoder(Conf(16000, 1024, 256, "full"))
    rng = np.random.default_rng(2222)
    x = np.stack([tone(1280, 16000, [250.0, 500.0], [0.5, 0.2], rng, noise=0.01)])
    r = f0_capture(enc, x)
    assert r["probabilities"].shape == (1, 2, 360)
    save("g22_f0_full", **w, x=x, **r)


def g23():
    out = {}
    for cap in ("tiny", "full"):
        seed_crepe(cap, 23)
        enc = ref_encoder.Encoder(Conf(44100, 2048, 512, cap))
        sd = enc.state_dict()
        out[f"{cap}_keys"] = np.array(list(sd.keys()), dtype="<U64")
        out[f"{cap}_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()], dtype="<U32")
        print(f"  g23 {cap}: {len(sd)} entries")
    save("g23_encoder_state_keys", **out)


class AEConf:
    n_harmonics, n_noise_filters, sample_rate, hop_length, n_fft = 16, 9, 44100, 512, 2048
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1
    crepe_capacity = "tiny"


MARGIN = 1e-4     # every frame of G24 / G25: a flipped pitch bin would change the audio completely


def make_ae(seed_w, seed_torch):
    w = seed_crepe("tiny", seed_w)
    torch.manual_seed(seed_torch)
    ae = ref_autoencoder.AutoEncoder(AEConf)
    with torch.no_grad():
        ae.decoder.reverb.wet.fill_(0.5)
        ae.decoder.reverb.decay.fill_(3.0)
    dec = {f"dw__{k}": v.numpy().copy() for k, v in ae.decoder.state_dict().items()}
    return ae, w, dec


def g24():
    # the first CREPE seed (from 2400 on) whose every frame of these inputs has a decisive pitch bin
    rng = np.random.default_rng(2424)
    x = np.stack([tone(8192, 44100, [220.0 * k for k in range(1, 5)], [0.5 / k for k in range(1, 5)], rng, noise=0.005),
                  tone(8192, 44100, [392.0, 784.0], [0.4, 0.2], rng, noise=0.005)])
    for seed in range(2400, 2500):
        ae, w, dec = make_ae(seed, 2424)
        p = ae.padding
        z = ae.encoder(F.pad(torch.from_numpy(x), (p // 2, p - p // 2)))
        m = top1_margin(z["probabilities"].numpy())
        if m.min() > MARGIN:
            break
    print(f"  g24: seed {seed}, {z['f0'].shape[1]} frames, min margin {m.min():.2e}")
    assert m.min() > MARGIN
    torch.manual_seed(77)
    y = ae(torch.from_numpy(x))
    save("g24_autoencoder_forward", **w, **dec, x=x, y=y.numpy(), **{f"z_{k}": v.numpy() for k, v in z.items()})


def g25():
    for seed in range(2500, 2600):
        if live_calls(seed, dry=True):
            break
    live_calls(seed)


def live_calls(seed, dry=False):
    ae, w, dec = make_ae(seed, 2525)
    rng = np.random.default_rng(2525)
    hidden = torch.from_numpy(rng.standard_normal((1, 1, 12)).astype(np.float32))
    out = {"hidden": hidden.numpy().copy()}
    buf = np.zeros(4096, np.float32)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # the CPU capture of autoencoder.py:28
    try:
        for call in range(3):
            buf[:-2048] = buf[2048:]
            buf[-2048:] = tone(2048, 44100, [261.63 * (call + 1), 523.25 * (call + 1)], [0.4, 0.2], rng, noise=0.005)
            if call == 0:
                buf[:2048] = tone(2048, 44100, [200.0], [0.4], rng, noise=0.005)
            z = ae.encoder(torch.from_numpy(buf.copy()).unsqueeze(0)[:, 256:-256])
            m = top1_margin(z["probabilities"].numpy())
            if dry:
                if m.min() <= MARGIN:
                    return False
                continue
            assert m.min() > MARGIN, (call, m.min())
            torch.manual_seed(250 + call)
            audio, h_ret = ae.forward_live(buf.copy(), hidden)
            assert h_ret is hidden
            out[f"x_{call}"] = buf.copy()
            out[f"audio_{call}"] = np.asarray(audio, dtype=np.float32)
            out.update({f"z{call}_{k}": v.numpy() for k, v in z.items()})
            print(f"  g25 call {call}: min margin {m.min():.2e}")
    finally:
        torch.Tensor.cuda = cuda
    if dry:
        return True
    print(f"  g25: seed {seed}")
    save("g25_autoencoder_live", **w, **dec, **out, last_phases=ae.decoder.harmonics.last_phases.detach().numpy().astype(np.float32))


if __name__ == "__main__":
    for fn in sys.argv[1:] or ("g19", "g20", "g21", "g22", "g23", "g24", "g25"):
        globals()[fn]()
