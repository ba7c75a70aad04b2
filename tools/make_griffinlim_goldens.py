#!/usr/bin/env python3
"""Generate the Griffin-Lim fixtures tests/golden/g27_* (torchaudio 0.8.1's functional.griffinlim, requirements.txt:111).

torchaudio is not installed, so `griffinlim_081` below is a RESTATEMENT of 0.8.1's function on today's torch.stft /
torch.istft, labelled as such: the same steps in the same order -- pack the batch, pow(1 / power), the initial angles as a
real view [..., 2], `rebuilt = tensor(0.)`, per iteration istft(...).float(), stft(center=True, reflect, onesided), the
in-place `tprev.mul_(momentum / (1 + momentum))`, complex_norm as pow(2).sum(-1).pow(0.5), `.add(1e-16)` and the division,
then the final istft and the unpacking.  The one change is forced by today's torch: 0.8.1 handed istft the real view
[..., 2], today's istft takes complex input, so the product is viewed as complex first (same values).

Each case stores its inputs (magnitude spectrogram, window, fixed complex64 angles, parameters) and, for n_iter 0, 1, 4 and 16:
  y32_<n>     the restatement on the fp32 spectrogram
  y64_<n>     the restatement on the same spectrogram in fp64 (0.8.1's `.float()` of each intermediate inverse included)
  exact_<n>   the same loop in fp64 throughout (no `.float()`): the yardstick of the spread
  spread_<n>  max |y32_<n> - exact_<n>|, the fp32-vs-fp64 spread the device tests scale their tolerance by

    PYTHONDONTWRITEBYTECODE=1 python tools/make_griffinlim_goldens.py
"""
import math
import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")     # MKL's one reproducible FFT path (tests/conftest.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_ITERS = (0, 1, 4, 16)


def griffinlim_081(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum, length, rand_init, angles=None,
                   cast_inverse=True):
    """RESTATEMENT of torchaudio 0.8.1 functional.griffinlim (without its unused `normalized`); `angles` (complex, the
    spectrogram's shape) replaces the initial draw, `cast_inverse=False` drops the `.float()` (the fp64 yardstick only)."""
    assert momentum < 1, 'momentum={} > 1 can be unstable'.format(momentum)
    assert momentum >= 0, 'momentum={} < 0'.format(momentum)
    shape = specgram.size()
    specgram = specgram.reshape([-1] + list(shape[-2:]))
    specgram = specgram.pow(1 / power)
    batch, freq, frames = specgram.size()
    if angles is not None:
        ang = torch.view_as_real(angles.reshape(batch, freq, frames)).to(dtype=specgram.dtype, device=specgram.device)
    else:
        if rand_init:
            ang = 2 * math.pi * torch.rand(batch, freq, frames)
        else:
            ang = torch.zeros(batch, freq, frames)
        ang = torch.stack([ang.cos(), ang.sin()], dim=-1).to(dtype=specgram.dtype, device=specgram.device)
    specgram = specgram.unsqueeze(-1).expand_as(ang)
    rebuilt = torch.tensor(0.)
    for _ in range(n_iter):
        tprev = rebuilt
        inverse = torch.istft(torch.view_as_complex((specgram * ang).contiguous()), n_fft=n_fft, hop_length=hop_length,
                              win_length=win_length, window=window, length=length)
        if cast_inverse:
            inverse = inverse.float()
        rebuilt = torch.view_as_real(torch.stft(input=inverse, n_fft=n_fft, hop_length=hop_length, win_length=win_length,
                                                window=window, center=True, pad_mode='reflect', normalized=False, onesided=True,
                                                return_complex=True))
        ang = rebuilt
        if momentum:
            ang = ang - tprev.mul_(momentum / (1 + momentum))
        ang = ang.div(ang.pow(2.).sum(-1).pow(0.5).add(1e-16).unsqueeze(-1).expand_as(ang))
    waveform = torch.istft(torch.view_as_complex((specgram * ang).contiguous()), n_fft=n_fft, hop_length=hop_length,
                           win_length=win_length, window=window, length=length)
    return waveform.reshape(shape[:-2] + waveform.shape[-1:])


def test_signal(rng, lead, samples, sr=16000):
    """Harmonic tones plus a little noise, one per leading row."""
    t = np.arange(samples) / sr
    rows = []
    for _ in range(int(np.prod(lead))):
        f0 = rng.uniform(110, 440)
        x = sum(rng.uniform(0.1, 0.5) / h * np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) for h in range(1, 9))
        rows.append(x + 0.02 * rng.standard_normal(samples))
    return np.asarray(rows).reshape(tuple(lead) + (samples,))


# name, n_fft, hop, win_length, power, momentum, length ('none', 'long', 'exact'), leading dims, frames
CASES = [
    ("n2048_h256", 2048, 256, 2048, 1.0, 0.99, "none", (1,), 28),
    ("n1024_h128_p2", 1024, 128, 1024, 2.0, 0.0, "long", (2,), 25),
    ("n512_h64", 512, 64, 512, 1.0, 0.99, "exact", (2, 1), 33),
    ("n512_w400_h100", 512, 100, 400, 1.0, 0.5, "none", (2,), 27),
]


def make_case(name, n_fft, hop, win_length, power, momentum, length_kind, lead, frames, seed):
    rng = np.random.default_rng(seed)
    natural = hop * (frames - 1)
    length = {"none": None, "long": natural + hop // 2, "exact": natural}[length_kind]
    window = torch.hann_window(win_length, True)
    x = torch.from_numpy(test_signal(rng, lead, natural).astype(np.float32))
    spec = torch.stft(x.reshape(-1, natural), n_fft, hop, win_length, window, center=True, pad_mode='reflect',
                      return_complex=True).abs().pow(power)
    spec = spec.reshape(tuple(lead) + spec.shape[-2:]).contiguous()
    assert spec.shape[-1] == frames
    phase = torch.from_numpy(rng.uniform(0, 2 * np.pi, spec.shape).astype(np.float32))
    angles = torch.polar(torch.ones_like(phase), phase)
    out = {"spec": spec.numpy(), "window": window.numpy(), "angles": angles.numpy(),
           "params": np.array([n_fft, hop, win_length, -1 if length is None else length], dtype=np.int64),
           "power": np.float64(power), "momentum": np.float64(momentum)}
    for n in N_ITERS:
        kw = dict(n_fft=n_fft, hop_length=hop, win_length=win_length, power=power, n_iter=n, momentum=momentum, length=length,
                  rand_init=False, angles=angles)
        y32 = griffinlim_081(spec, window, **kw)
        y64 = griffinlim_081(spec.double(), window.double(), **kw)
        exact = griffinlim_081(spec.double(), window.double(), cast_inverse=False, **kw)
        out[f"y32_{n}"] = y32.numpy()
        out[f"y64_{n}"] = y64.numpy()
        out[f"exact_{n}"] = exact.numpy()
        out[f"spread_{n}"] = np.float64((y32.double() - exact).abs().max())
    return out


def main():
    torch.set_num_threads(1)
    os.makedirs(GOLDEN, exist_ok=True)
    for i, case in enumerate(CASES):
        arrays = make_case(*case, seed=2700 + i)
        path = os.path.join(GOLDEN, f"g27_{case[0]}.npz")
        np.savez_compressed(path, **arrays)
        print(path, {k: float(arrays[k]) for k in arrays if k.startswith("spread")})


if __name__ == "__main__":
    sys.exit(main())
