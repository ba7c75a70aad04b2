"""Griffin-Lim phase reconstruction: `torchaudio.functional.griffinlim` (torchaudio 0.8.1, requirements.txt:111) as the
reference's spectral tools call it (style_transfer.py:149-156, helper.py:105-112), with the iteration on the device.

On CUDA fp32 with n_fft a power of two in [64, 2048] every iteration is three HIP launches (csrc/ddsp_griffinlim.hip, DESIGN
§12) and the call does not synchronise with the host after its checks.  CPU tensors run the stock loop below; every other
CUDA case (another n_fft, fp64) runs the same stock loop on the device, as LoudnessEncoder does for n_fft.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib

__all__ = ["griffinlim", "griffinlim_uses_hip", "window_envelope"]


def _padded_window(window: torch.Tensor, n_fft: int, win_length: int) -> torch.Tensor:
    """The window zero-padded and centred to n_fft, as torch.stft / torch.istft pad a win_length window."""
    if window.dim() != 1 or window.shape[0] != win_length:
        raise ValueError(f"window must be 1-D of win_length = {win_length} samples, got shape {tuple(window.shape)}")
    if not 0 < win_length <= n_fft:
        raise ValueError(f"win_length = {win_length} must be in [1, n_fft = {n_fft}]")
    left = (n_fft - win_length) // 2
    return torch.nn.functional.pad(window, (left, n_fft - win_length - left))


def window_envelope(window: torch.Tensor, n_fft: int, hop_length: int, n_frames: int, length: Optional[int]) -> torch.Tensor:
    """istft's window envelope over the retained samples: sum of window^2 over the frames covering sample n_fft/2 + j, for
    j < min(L, n_fft/2 + hop (T - 1)), L = length or hop (T - 1).  `window` is already padded to n_fft."""
    full = n_fft + hop_length * (n_frames - 1)
    sq = window.pow(2).reshape(1, n_fft, 1).expand(1, n_fft, n_frames)
    env = torch.nn.functional.fold(sq, output_size=(1, full), kernel_size=(1, n_fft), stride=(1, hop_length)).reshape(full)
    L = length if length is not None else hop_length * (n_frames - 1)
    return env[n_fft // 2:n_fft // 2 + L]


def griffinlim_uses_hip(device: torch.device, dtype: torch.dtype, n_fft: int, win_length: int) -> bool:
    """Whether griffinlim takes the HIP path for these arguments (CUDA fp32, n_fft a power of two in [64, 2048],
    win_length <= n_fft); every other case runs the stock loop on the tensor's device."""
    if torch.device(device).type != "cuda" or dtype != torch.float32 or not 0 < win_length <= n_fft:
        return False
    return bool(_lib.lib().ddsp_griffinlim_supported(int(n_fft)))


def _initial_angles(batch: int, freq: int, frames: int, rand_init: bool, generator, angles, shape, dtype, device):
    """torchaudio 0.8.1's start, as a real view [batch, F, T, 2]: unit modulus with phase 2 pi rand (drawn on the CPU from
    `generator`) or all 1; an explicit complex `angles` [..., F, T] overrides both."""
    if angles is not None:
        if not torch.is_complex(angles) or tuple(angles.shape) != tuple(shape):
            raise ValueError(f"angles must be a complex tensor of the spectrogram's shape {tuple(shape)}, got "
                             f"{angles.dtype} {tuple(angles.shape)}")
        a = torch.view_as_real(angles.reshape(batch, freq, frames).resolve_conj())
        return a.to(dtype=dtype, device=device)
    if rand_init:
        phase = 2 * math.pi * torch.rand(batch, freq, frames, generator=generator)
    else:
        phase = torch.zeros(batch, freq, frames)
    return torch.stack([phase.cos(), phase.sin()], dim=-1).to(dtype=dtype, device=device)


def _stock_loop(spec, ang, window, n_fft, hop_length, win_length, n_iter, momentum, length):
    """torchaudio 0.8.1's iteration on torch.stft / torch.istft (real-view angles, complex_norm as pow / sum / pow, the
    `.float()` of every intermediate inverse, the in-place momentum product of the previous rebuild)."""
    specgram = spec.unsqueeze(-1).expand_as(ang)
    rebuilt = torch.tensor(0.)
    for _ in range(n_iter):
        tprev = rebuilt
        inverse = torch.istft(torch.view_as_complex((specgram * ang).contiguous()), n_fft=n_fft, hop_length=hop_length,
                              win_length=win_length, window=window, length=length).float()
        rebuilt = torch.view_as_real(torch.stft(inverse, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window,
                                                center=True, pad_mode='reflect', normalized=False, onesided=True,
                                                return_complex=True))
        ang = rebuilt
        if momentum:
            ang = ang - tprev.mul_(momentum / (1 + momentum))
        ang = ang.div(ang.pow(2.).sum(-1).pow(0.5).add(1e-16).unsqueeze(-1).expand_as(ang))
    return torch.istft(torch.view_as_complex((specgram * ang).contiguous()), n_fft=n_fft, hop_length=hop_length,
                       win_length=win_length, window=window, length=length)


def griffinlim(specgram: torch.Tensor, window: torch.Tensor, n_fft: int, hop_length: int, win_length: int, power: float,
               n_iter: int, momentum: float, length: Optional[int], rand_init: bool, *, generator: Optional[torch.Generator] = None,
               angles: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Waveform [..., L] from a magnitude spectrogram [..., n_fft // 2 + 1, T] by Griffin-Lim with momentum (fast Griffin-Lim),
    L = `length` or hop_length * (T - 1).  The semantics of torchaudio 0.8.1's `functional.griffinlim`; the keywords are the
    reference's.  0.8.1's `normalized` argument is left out: it was unused there (a deprecation warning only) and the
    reference never passes it.

    `rand_init` draws the initial phases as 0.8.1 does, `2 pi torch.rand(batch, F, T)` on the CPU, from `generator` (default:
    torch's global generator), so the same seed gives the same start; without it every angle is 1.  An explicit complex
    `angles` of the spectrogram's shape overrides both.

    Raises before any work: ValueError for momentum outside [0, 1), for a `length` with 1 + length // hop_length != T (the
    stock loop would die on a broadcast in its second iteration), for a signal too short for reflect padding
    (L <= n_fft // 2) and for a bad shape; RuntimeError (torch's "window overlap add min" message) when the window envelope is
    below 1e-11 anywhere in the retained range (checked once per call) and for an input that requires grad (there is no
    backward).
    """
    if not 0 <= momentum < 1:
        raise ValueError(f"momentum={momentum} must be in [0, 1) (torchaudio asserts momentum < 1 and momentum >= 0)")
    for name, t in (("specgram", specgram), ("window", window), ("angles", angles)):
        if t is not None and t.requires_grad:
            raise RuntimeError(f"griffinlim has no backward: {name} must not require grad")
    if n_iter < 0 or hop_length <= 0:
        raise ValueError(f"n_iter = {n_iter} and hop_length = {hop_length} must be >= 0 and > 0")
    shape = specgram.shape
    freq = n_fft // 2 + 1
    if specgram.dim() < 2 or shape[-2] != freq or shape[-1] < 1:
        raise ValueError(f"specgram must be [..., n_fft // 2 + 1 = {freq}, T >= 1], got {tuple(shape)}")
    spec = specgram.reshape([-1] + list(shape[-2:]))
    batch, _, frames = spec.shape
    if length is not None and 1 + length // hop_length != frames:
        raise ValueError(f"length = {length} gives 1 + length // hop_length = {1 + length // hop_length} frames, the "
                         f"spectrogram has {frames}")
    L = length if length is not None else hop_length * (frames - 1)
    if L <= n_fft // 2:
        raise ValueError(f"a signal of {L} samples is too short for the reflect padding of n_fft // 2 = {n_fft // 2}")
    wpad = _padded_window(window, n_fft, win_length)
    env = window_envelope(wpad.to(spec.device), n_fft, hop_length, frames, length)
    natural = n_fft // 2 + hop_length * (frames - 1)
    lowest = float(env[:min(L, natural)].abs().min())
    if lowest < 1e-11:
        raise RuntimeError(f"griffinlim: window overlap add min: {lowest:g} (the window does not satisfy NOLA for "
                           f"n_fft = {n_fft}, hop_length = {hop_length}, win_length = {win_length})")

    spec = spec.pow(1 / power)
    if griffinlim_uses_hip(spec.device, spec.dtype, n_fft, win_length) and batch <= 65535:
        y = _griffinlim_hip(spec, wpad, env, n_fft, hop_length, L, n_iter, momentum, rand_init, generator, angles, shape)
    else:
        ang = _initial_angles(batch, freq, frames, rand_init, generator, angles, shape, spec.dtype, spec.device)
        with torch.no_grad():
            y = _stock_loop(spec, ang, window, n_fft, hop_length, win_length, n_iter, momentum, length)
    return y.reshape(shape[:-2] + y.shape[-1:])


def _griffinlim_hip(spec, wpad, env, n_fft, hop_length, L, n_iter, momentum, rand_init, generator, angles, shape):
    batch, freq, frames = spec.shape
    dev = spec.device
    mag = spec.contiguous()
    ang = None
    if angles is not None or rand_init:
        ang = _initial_angles(batch, freq, frames, rand_init, generator, angles, shape, torch.float32, dev).contiguous()
    win = wpad.to(device=dev, dtype=torch.float32).contiguous()
    envd = torch.ones(L, device=dev, dtype=torch.float32)
    envd[:env.shape[0]] = env.to(torch.float32)
    c = float(torch.tensor(momentum / (1 + momentum), dtype=torch.float32)) if momentum else 0.0
    lib = _lib.lib()
    y = torch.empty((batch, L), device=dev, dtype=torch.float32)
    nbytes = lib.ddsp_griffinlim_workspace_bytes(batch, frames, n_fft, int(ang is not None))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        rc = lib.ddsp_griffinlim(mag.data_ptr(), ang.data_ptr() if ang is not None else None, win.data_ptr(), envd.data_ptr(),
                                 y.data_ptr(), ws.data_ptr(), nbytes, batch, frames, n_fft, hop_length, L, n_iter, c,
                                 torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_griffinlim")
    return y
