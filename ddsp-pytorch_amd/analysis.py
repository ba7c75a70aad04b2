"""Harmonic analysis: the inverse of `OscillatorBank` (include/ddsp_hip.h: ddsp_harm_*).

Given audio [B, N] and its pitch track f0 [B, T, 1] (N = T hop), the per-frame complex amplitudes C [B, T, H] of the harmonics
along the oscillator's own phase track, the bank's controls a = sum_k |C| and c = |C| / a, the harmonic part of the audio and
the residual the harmonics do not explain:

  harmonic_analysis(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False) -> dict(f0, a, c[, C])
  harmonic_resynthesis(C, f0, hop, sample_rate) -> harm [B, T hop]
  harmonic_residual(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False)
                                                                        -> (harm, resid, the dict of harmonic_analysis)
  HarmonicAnalyzer(conf)  nn.Module without parameters over conf.n_harmonics / sample_rate / hop_length / n_fft (the window)

The returned `f0` is the track the analysis demodulated with: the input with frames that are not finite or <= 0 set to 0, so
that `OscillatorBank` on the dict runs the same phases.  CUDA fp32 tensors with an even win_length <= 4096 and n_harmonics <= 256
take the HIP kernels (csrc/ddsp_harm.hip); CPU tensors, and CUDA calls outside that range or in fp64, run the same definition as
stock torch ops in the input's dtype (fp64 in, fp64 out), frames and samples in chunks that bound the memory.  No backward.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib
from .encoder import _refuse_grad

KERNEL_MAX_WINDOW = 4096
KERNEL_MAX_HARMONICS = 256
PHASE_READY = 1                          # include/ddsp_hip.h: DDSP_HARM_PHASE_READY
_CHUNK_ELEMENTS = 1 << 24                # the torch path's largest intermediate, in elements


def _check(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced, what):
    if f0.dim() != 3 or f0.shape[-1] != 1:
        raise ValueError(f"{what}: f0 must be [B, T, 1], got {tuple(f0.shape)}")
    B, T = f0.shape[:2]
    hop, sample_rate, n_harmonics = int(hop), int(sample_rate), int(n_harmonics)
    if hop < 1 or sample_rate < 1 or n_harmonics < 1 or T < 1:
        raise ValueError(f"{what}: hop, sample_rate, n_harmonics and the number of frames must be positive")
    if win_length is not None and (int(win_length) < 2 or int(win_length) % 2):
        raise ValueError(f"{what}: win_length must be even and at least 2, got {win_length}")
    if audio is not None:
        if audio.dim() != 2 or audio.shape[0] != B:
            raise ValueError(f"{what}: audio must be [B, N] with f0's batch, got {tuple(audio.shape)} and f0 {tuple(f0.shape)}")
        if audio.shape[1] != T * hop:
            raise ValueError(f"{what}: audio has {audio.shape[1]} samples, f0 has {T} frames of hop {hop} = {T * hop}")
        if audio.device != f0.device:
            raise ValueError(f"{what}: audio and f0 are on different devices")
        _refuse_grad(audio, what)
    _refuse_grad(f0, what)
    if voiced is not None and tuple(voiced.shape) != (B, T, 1):
        raise ValueError(f"{what}: voiced must be [B, T, 1], got {tuple(voiced.shape)}")
    if voiced is not None and voiced.device != f0.device:        # (the kernel would read a host address)
        raise ValueError(f"{what}: voiced is on {voiced.device}, f0 on {f0.device}")
    return B, T, hop, sample_rate, n_harmonics


def _in_kernel_range(x: torch.Tensor, win_length, n_harmonics: int) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and n_harmonics <= KERNEL_MAX_HARMONICS
            and (win_length is None or win_length <= KERNEL_MAX_WINDOW))


def _clean_f0(f0: torch.Tensor) -> torch.Tensor:
    return torch.where(torch.isfinite(f0) & (f0 > 0), f0, torch.zeros((), dtype=f0.dtype, device=f0.device))


# ------------------------------------------------------------------------------------------------------------ torch-op path

def _up_index(n: torch.Tensor, T: int, hop: int):
    """Frames and weight of the bank's upsampling at the samples n (int64): (i0, i1, frac in fp64)."""
    pos = ((n.double() + 0.5) / hop - 0.5).clamp(0, T - 1)
    i0 = pos.floor().long()
    return i0, (i0 + 1).clamp(max=T - 1), pos - i0.double()


def _up(x: torch.Tensor, n: torch.Tensor, hop: int) -> torch.Tensor:
    """x [B, T, K] at the samples n -> [B, len(n), K]: x[i0] + (x[i1] - x[i0]) frac."""
    i0, i1, frac = _up_index(n, x.shape[1], hop)
    return x[:, i0] + (x[:, i1] - x[:, i0]) * frac.to(x.dtype)[None, :, None]


def _theta(f0: torch.Tensor, hop: int, sample_rate: int) -> torch.Tensor:
    """The phase track in turns, fp64 [B, N], whatever the dtype of f0."""
    B, T = f0.shape[:2]
    n = torch.arange(T * hop, device=f0.device)
    return torch.cumsum(_up(_clean_f0(f0).double(), n, hop)[..., 0] / sample_rate, dim=1)


def _harmonic_mask(f0: torch.Tensor, voiced, sample_rate: int, H: int) -> torch.Tensor:
    """[B, T, H] True where C is kept: the bank's Nyquist mask (product in f0's dtype), a usable f0, a voiced frame."""
    k = torch.arange(1, H + 1, device=f0.device).to(f0.dtype)
    keep = ~(k * f0 > sample_rate // 2) & torch.isfinite(f0) & (f0 > 0)
    if voiced is not None:
        keep = keep & voiced.bool()
    return keep


def _analysis_torch(audio, f0, voiced, hop, sample_rate, H, W):
    dt, dev = audio.dtype, audio.device
    B, N = audio.shape
    T = f0.shape[1]
    theta = _theta(f0, hop, sample_rate)
    j = torch.arange(W, device=dev)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * j.double() / W)
    k = torch.arange(1, H + 1, device=dev).double()
    lead = (W - hop) // 2
    C = torch.zeros((B, T, H), dtype=torch.complex128 if dt == torch.float64 else torch.complex64, device=dev)
    step = max(1, _CHUNK_ELEMENTS // max(1, B * W * H))
    zero = torch.zeros((), dtype=dt, device=dev)
    for t0 in range(0, T, step):
        t = torch.arange(t0, min(T, t0 + step), device=dev)
        idx = (t * hop - lead)[:, None] + j[None, :]                              # [Tc, W]
        inside = (idx >= 0) & (idx < N)
        at = idx.clamp(0, N - 1)
        wj = torch.where(inside, w[None, :], torch.zeros((), dtype=torch.float64, device=dev))
        norm = wj.sum(-1)                                                         # fp64 [Tc]
        wx = torch.where(inside[None], wj.to(dt)[None] * audio[:, at], zero)      # [B, Tc, W]
        turns = (theta[:, at][..., None] * k) % 1.0                               # [B, Tc, W, H] fp64
        ang = (2 * math.pi * turns).to(dt)
        re = torch.einsum('btw,btwh->bth', wx, torch.cos(ang))
        im = -torch.einsum('btw,btwh->bth', wx, torch.sin(ang))
        scale = (2.0 / norm).to(dt)[None, :, None]
        C[:, t0:t0 + step] = torch.complex(re * scale, im * scale)
    C = torch.where(_harmonic_mask(f0, voiced, sample_rate, H), C, torch.zeros((), dtype=C.dtype, device=dev))
    amp = C.abs()
    a = amp.sum(-1, keepdim=True)
    c = torch.where(a == 0, torch.full((), 1.0 / H, dtype=dt, device=dev), amp / a)
    return C, a, c


def _resynth_torch(C, f0, hop, sample_rate):
    B, T, H = C.shape
    dt = C.real.dtype
    theta = _theta(f0, hop, sample_rate)
    k = torch.arange(1, H + 1, device=C.device).double()
    parts = torch.view_as_real(C).reshape(B, T, 2 * H)                            # re, im interleaved per harmonic
    harm = torch.empty((B, T * hop), dtype=dt, device=C.device)
    step = max(1, _CHUNK_ELEMENTS // max(1, B * H))
    for n0 in range(0, T * hop, step):
        n = torch.arange(n0, min(T * hop, n0 + step), device=C.device)
        ang = (2 * math.pi * ((theta[:, n0:n0 + step, None] * k) % 1.0)).to(dt)   # [B, Nc, H]
        cu = _up(parts, n, hop).reshape(B, -1, H, 2)
        harm[:, n0:n0 + step] = (cu[..., 0] * torch.cos(ang) - cu[..., 1] * torch.sin(ang)).sum(-1)
    return harm


# -------------------------------------------------------------------------------------------------------------- device path

def _workspace(B, T, hop, device):
    return torch.empty(_lib.lib().ddsp_harm_workspace_bytes(B, T, hop), device=device, dtype=torch.uint8)


def _analysis_device(audio, f0, voiced, hop, sample_rate, H, W, workspace):
    B, T = f0.shape[:2]
    C = torch.empty((B, T, H, 2), device=audio.device, dtype=torch.float32)
    a = torch.empty((B, T, 1), device=audio.device, dtype=torch.float32)
    c = torch.empty((B, T, H), device=audio.device, dtype=torch.float32)
    v = None if voiced is None else voiced.detach().to(torch.uint8).contiguous()
    with torch.cuda.device(audio.device):
        rc = _lib.lib().ddsp_harm_analysis(audio.data_ptr(), f0.data_ptr(), None if v is None else v.data_ptr(), C.data_ptr(),
                                           a.data_ptr(), c.data_ptr(), workspace.data_ptr(), B, T, hop, W, H, sample_rate,
                                           torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_harm_analysis")
    return torch.view_as_complex(C), a, c


def _resynth_device(C, f0, audio, hop, sample_rate, workspace, phase_ready):
    B, T, H = C.shape
    Cr = torch.view_as_real(C).contiguous()
    harm = torch.empty((B, T * hop), device=C.device, dtype=torch.float32)
    resid = None if audio is None else torch.empty_like(harm)
    with torch.cuda.device(C.device):
        rc = _lib.lib().ddsp_harm_resynth(Cr.data_ptr(), f0.data_ptr(), None if audio is None else audio.data_ptr(), harm.data_ptr(),
                                          None if resid is None else resid.data_ptr(), workspace.data_ptr(), B, T, hop, H,
                                          sample_rate, PHASE_READY if phase_ready else 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_harm_resynth")
    return harm, resid


# ------------------------------------------------------------------------------------------------------------------- public

def _controls(f0, a, c, C, return_complex):
    out = dict(f0=_clean_f0(f0), a=a, c=c)
    if return_complex:
        out['C'] = C
    return out


def _empty(f0, T, hop, H, dt):
    dev = f0.device
    C = torch.zeros((0, T, H), dtype=torch.complex128 if dt == torch.float64 else torch.complex64, device=dev)
    return C, torch.zeros((0, T, 1), dtype=dt, device=dev), torch.zeros((0, T, H), dtype=dt, device=dev)


def _prepare(audio, f0, voiced):
    audio = audio.detach()
    if audio.dtype not in (torch.float32, torch.float64):        # integers and 16-bit floats: analysed in fp32
        audio = audio.float()
    return audio.contiguous(), f0.detach().to(audio.dtype).contiguous(), None if voiced is None else voiced.detach()


def harmonic_residual(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False):
    """-> (harm [B, N], resid = audio - harm, dict(f0, a, c[, C])): the harmonic part of `audio` along `f0` and what is left."""
    B, T, hop, sample_rate, H = _check(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced, "harmonic_residual")
    W = int(win_length)
    audio, f0, voiced = _prepare(audio, f0, voiced)
    if B == 0:
        C, a, c = _empty(f0, T, hop, H, audio.dtype)
        return torch.zeros_like(audio), torch.zeros_like(audio), _controls(f0, a, c, C, return_complex)
    if _in_kernel_range(audio, W, H):
        ws = _workspace(B, T, hop, audio.device)
        C, a, c = _analysis_device(audio, f0, voiced, hop, sample_rate, H, W, ws)
        harm, resid = _resynth_device(C, f0, audio, hop, sample_rate, ws, True)
    else:
        C, a, c = _analysis_torch(audio, f0, voiced, hop, sample_rate, H, W)
        harm = _resynth_torch(C, f0, hop, sample_rate)
        resid = audio - harm
    return harm, resid, _controls(f0, a, c, C, return_complex)


def harmonic_analysis(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False):
    """-> dict(f0 [B, T, 1], a [B, T, 1], c [B, T, H]) as `OscillatorBank` reads it, plus C (complex [B, T, H]) when asked."""
    B, T, hop, sample_rate, H = _check(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced, "harmonic_analysis")
    W = int(win_length)
    audio, f0, voiced = _prepare(audio, f0, voiced)
    if B == 0:
        C, a, c = _empty(f0, T, hop, H, audio.dtype)
    elif _in_kernel_range(audio, W, H):
        C, a, c = _analysis_device(audio, f0, voiced, hop, sample_rate, H, W, _workspace(B, T, hop, audio.device))
    else:
        C, a, c = _analysis_torch(audio, f0, voiced, hop, sample_rate, H, W)
    return _controls(f0, a, c, C, return_complex)


def harmonic_resynthesis(C, f0, hop, sample_rate):
    """C complex [B, T, H] (as harmonic_analysis returns it, or any other) along `f0` -> harm [B, T hop]."""
    if C.dim() != 3 or C.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"harmonic_resynthesis: C must be complex64 or complex128 [B, T, H], got {C.dtype} {tuple(C.shape)}")
    B, T, hop, sample_rate, H = _check(None, f0, hop, sample_rate, max(1, C.shape[-1]), None, None, "harmonic_resynthesis")
    if tuple(C.shape[:2]) != (B, T) or C.shape[-1] < 1 or C.device != f0.device:
        raise ValueError(f"harmonic_resynthesis: C {tuple(C.shape)} does not match f0 {tuple(f0.shape)}")
    _refuse_grad(C, "harmonic_resynthesis")
    C = C.detach().contiguous()
    f0 = f0.detach().to(C.real.dtype).contiguous()
    if B == 0:
        return torch.zeros((0, T * hop), dtype=C.real.dtype, device=C.device)
    if _in_kernel_range(C.real, None, H):
        return _resynth_device(C, f0, None, hop, sample_rate, _workspace(B, T, hop, C.device), False)[0]
    return _resynth_torch(C, f0, hop, sample_rate)


class HarmonicAnalyzer(nn.Module):
    """forward(audio [B, T hop], f0 [B, T, 1], voiced=None) -> dict(f0, a, c): `harmonic_analysis` at the configuration's
    n_harmonics, sample_rate, hop_length and n_fft (the window).  No parameters."""

    def __init__(self, conf):
        super().__init__()
        self.n_harmonics = conf.n_harmonics
        self.sample_rate = conf.sample_rate
        self.hop_length = conf.hop_length
        self.win_length = conf.n_fft

    def forward(self, audio, f0, voiced=None):
        return harmonic_analysis(audio, f0, self.hop_length, self.sample_rate, self.n_harmonics, self.win_length, voiced=voiced)
