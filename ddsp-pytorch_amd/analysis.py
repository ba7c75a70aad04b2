"""Harmonic analysis: the inverse of `OscillatorBank` (include/ddsp_hip.h: ddsp_harm_*).

Given audio [B, N] and its pitch track f0 [B, T, 1] (N = T hop), the per-frame complex amplitudes C [B, T, H] of the harmonics
along the oscillator's own phase track, the bank's controls a = sum_k |C| and c = |C| / a, the harmonic part of the audio and
the residual the harmonics do not explain:

  harmonic_analysis(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False, refine=0,
                    max_cents=50.0) -> dict(f0, a, c[, C])
  harmonic_resynthesis(C, f0, hop, sample_rate) -> harm [B, T hop]
  harmonic_residual(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False, refine=0,
                    max_cents=50.0)                                     -> (harm, resid, the dict of harmonic_analysis)
  refine_f0(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, iterations=2, max_cents=50.0) -> f0 [B, T, 1]
  HarmonicAnalyzer(conf, refine=0)  nn.Module without parameters over conf.n_harmonics / sample_rate / hop_length / n_fft (the window)

`refine_f0` reads the pitch back from the harmonics (ddsp_harm_refine): per step and per frame whose
window lies inside the clip, the |C_k|^2-weighted least-squares fit of the harmonics' reassigned frequency deviations replaces the
frame's f0 by the window mean of the track plus that deviation; every frame stays within `max_cents` of the track given.  A decoded
track is up to half a 20-cent bin off, which puts high harmonics outside their analysis window; `refine=N` in the analysis
functions runs N such steps first and demodulates with (and returns) the refined track.  refine=0 is the analysis as it was.

The returned `f0` is the track the analysis demodulated with: the input with frames that are not finite or <= 0 set to 0, so
that `OscillatorBank` on the dict runs the same phases.  CUDA fp32 tensors with an even win_length <= 4096 and n_harmonics <= 256
take the HIP kernels (csrc/ddsp_harm.hip); CPU tensors, and CUDA calls outside that range or in fp64, run the same definition as
stock torch ops in the input's dtype (fp64 in, fp64 out), frames and samples in chunks that bound the memory.  No backward.

Noise analysis: the inverse of `FilteredNoise` (include/ddsp_hip.h: ddsp_noise_analysis).  From a residual
x [B, T hop] the band magnitudes H [B, T, n_filters] whose FilteredNoise frames have, in expectation, the in-frame
autocorrelation measured on x (averaged over `average` frames), by `iterations` steps of a multiplicative fixed point:

  noise_analysis(x, hop, n_filters, average=1, iterations=None, return_power=False, overlap_add=False)
                                                                        -> H [B, T, F]  (or (H, p), p the target spectrum)
  NoiseAnalyzer(conf, overlap_add=None)   nn.Module without parameters over conf.n_noise_filters / hop_length

hop >= 2 (n_filters - 1) is required (below it the filter is cropped and H is not identifiable).  CUDA fp32 tensors with
n_filters <= 257 and hop <= 1024 take the HIP kernels (csrc/ddsp_noise_analysis.hip); everything else the same definition as
stock torch ops in the input's dtype.  No backward.

overlap_add=True inverts FilteredNoise's overlap-add mode instead (ddsp_noise_analysis_ola): that noise is
stationary, so the model is (hop / 3) times the autocorrelation of the frame's whole response, the measured products cross frame
boundaries and any hop >= 1 is analysable.  `iterations=None` is 16 for the truncated model and 8 for the overlap-add one.

Control transformation: what makes the analysed dict worth having (include/ddsp_hip.h:
ddsp_transform_controls).  Time stretch, transposition and formant shift of f0, a, c and the noise bands H between analysis and
synthesis, the spectral envelope resampled in harmonic coordinates so that a transposition does not carry the formants along:

  transform_controls(ctrl, sample_rate, stretch=1.0, transpose=0.0, formant=0.0, positions=None, n_harmonics=None) -> dict
  ControlTransform(conf)                  nn.Module without parameters over conf.sample_rate

CUDA fp32 controls with at most 256 harmonics (in and out) and 257 bands take the HIP kernel (csrc/ddsp_transform.hip), one
launch; everything else the same definition as stock torch ops in the controls' dtype.  No backward.

Control morph: the operation between two analysed sounds (include/ddsp_hip.h: ddsp_morph_controls).  A
sound whose pitch (in log frequency), spectral envelope (compared at equal frequency, or harmonic by harmonic) and noise bands
each lie between those of two control dicts, by weights that may move over time; the two sounds may differ in frames and in
harmonics, and `positions_a` / `positions_b` take any time alignment:

  morph_controls(ctrl_a, ctrl_b, sample_rate, mix=0.5, mix_f0=None, mix_harmonics=None, mix_noise=None, coordinates='hz',
                 frames=None, positions_a=None, positions_b=None, n_harmonics=None) -> dict
  ControlMorph(conf)                      nn.Module without parameters over conf.sample_rate

CUDA fp32 controls in the transformation's range take the HIP kernel (csrc/ddsp_morph.hip), one launch; everything else the same
definition as stock torch ops.  No backward.

Time alignment: which frame of one sound goes with which frame of the other (include/ddsp_hip.h:
ddsp_dtw_align).  Dynamic time warping over per-frame features, the path resampled onto an output timeline as the
`positions_a` / `positions_b` of `morph_controls`:

  dtw_align(x_a, x_b, radius=None, penalty=0.0, timing=0.0, frames=None, return_path=False) -> positions_a, positions_b[, path, length, cost]
  control_features(ctrl, sample_rate, n_bands=32, noise_groups=8, range_log2=10.0) -> [B, T, D]
  align_controls(ctrl_a, ctrl_b, sample_rate, radius=None, penalty=0.0, timing=0.0, frames=None, return_path=False, **features)
  ControlAlign(conf)                      nn.Module without parameters over conf.sample_rate

CUDA fp32 features with D <= 64 and at most 2048 frames a sound take the HIP kernel (csrc/ddsp_align.hip), one launch for the
recurrence, the walk back and the timeline; everything else the same definition as stock torch ops.  No backward.
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
NOISE_KERNEL_MAX_FILTERS = 257           # csrc/ddsp_noise_analysis.hip: kMaxF, kMaxHop, kMaxGrid
NOISE_KERNEL_MAX_HOP = 1024
NOISE_KERNEL_MAX_FRAMES = 2 ** 31 - 1
NOISE_OLA_KERNEL_MAX_SAMPLES = 2 ** 31 - 8192   # (exclusive) samples of one row of the overlap-add analysis
NOISE_ITERATIONS = 16                    # the defaults of `iterations`: the truncated model and the overlap-add one
NOISE_OLA_ITERATIONS = 8
TRANSFORM_KERNEL_MAX_FRAMES = 2 ** 47    # csrc/ddsp_transform.hip: rows x frames, in or out; kMaxBlocks and kWaves
TRANSFORM_KERNEL_MAX_BLOCKS = 8192
TRANSFORM_KERNEL_WAVES = 4
MORPH_KERNEL_MAX_FRAMES = 2 ** 47        # csrc/ddsp_morph.hip: rows x frames of either sound or of the output; kMaxBlocks, kWaves
MORPH_KERNEL_MAX_BLOCKS = 8192
MORPH_KERNEL_WAVES = 4
MORPH_COORDINATES = {'hz': 0, 'harmonic': 1}    # include/ddsp_hip.h: DDSP_MORPH_HZ, DDSP_MORPH_HARMONIC
DTW_KERNEL_MAX_FRAMES = 2048             # csrc/ddsp_align.hip: kMaxT, kMaxD
DTW_KERNEL_MAX_FEATURES = 64


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


def _refine_torch(audio, f0, anchor, voiced, hop, sample_rate, H, W, max_cents):
    """One refinement step as torch ops in f0's dtype (the phase track and the window mean in fp64): f0, anchor [B, T, 1] -> g."""
    dt, dev = audio.dtype, audio.device
    B, N = audio.shape
    T = f0.shape[1]
    lead = (W - hop) // 2
    alive = torch.isfinite(f0) & (f0 > 0)
    if voiced is not None:
        alive = alive & voiced.bool()
    inter = [t for t in range(T) if t * hop - lead >= 0 and t * hop - lead + W <= N]
    g = f0.clone()
    if inter:
        t_lo, t_hi = inter[0], inter[-1]
        theta = _theta(f0, hop, sample_rate)
        j = torch.arange(W, device=dev)
        w = 0.5 - 0.5 * torch.cos(2 * math.pi * j.double() / W)
        wd = (math.pi / W) * torch.sin(2 * math.pi * j.double() / W)
        k = torch.arange(1, H + 1, device=dev).double()
        keep = _harmonic_mask(f0, voiced, sample_rate, H)
        zero = torch.zeros((), dtype=dt, device=dev)
        step = max(1, _CHUNK_ELEMENTS // max(1, B * W * H))
        for t0 in range(t_lo, t_hi + 1, step):
            t = torch.arange(t0, min(t_hi + 1, t0 + step), device=dev)
            idx = (t * hop - lead)[:, None] + j[None, :]                              # [Tc, W], all inside the clip
            x = audio[:, idx]                                                         # [B, Tc, W]
            wx, wdx = w.to(dt) * x, wd.to(dt) * x
            ang = (2 * math.pi * ((theta[:, idx][..., None] * k) % 1.0)).to(dt)       # [B, Tc, W, H]
            cos, sin = torch.cos(ang), torch.sin(ang)
            kept = keep[:, t0:t0 + len(t)]
            cr, ci = (torch.where(kept, v, zero) for v in (torch.einsum('btw,btwh->bth', wx, cos), -torch.einsum('btw,btwh->bth', wx, sin)))
            dr, di = (torch.where(kept, v, zero) for v in (torch.einsum('btw,btwh->bth', wdx, cos), -torch.einsum('btw,btwh->bth', wdx, sin)))
            kk = k.to(dt)
            num = (kk * (di * cr - dr * ci)).sum(-1, keepdim=True)
            den = (kk * kk * (cr * cr + ci * ci)).sum(-1, keepdim=True)
            mean = ((w[None, None, :] * _up(_clean_f0(f0).double(), idx.reshape(-1), hop).reshape(B, len(t), W)).sum(-1, keepdim=True)
                    / w.sum()).to(dt)
            value = mean - (sample_rate / (2 * math.pi)) * num / den
            here = f0[:, t0:t0 + len(t)]
            g[:, t0:t0 + len(t)] = torch.where(alive[:, t0:t0 + len(t)] & (den != 0) & torch.isfinite(value), value, here)
        one = torch.ones((), dtype=dt, device=dev)
        for edge, frames in ((t_lo, slice(0, t_lo)), (t_hi, slice(t_hi + 1, T))):
            ratio = torch.where(alive[:, edge:edge + 1], g[:, edge:edge + 1] / f0[:, edge:edge + 1], one)
            g[:, frames] = torch.where(alive[:, frames], f0[:, frames] * ratio, f0[:, frames])
    clamped = torch.minimum(torch.maximum(g, anchor * 2.0 ** (-max_cents / 1200.0)), anchor * 2.0 ** (max_cents / 1200.0))
    return torch.where(alive, clamped, f0)


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


def _refine_device(audio, f0, voiced, hop, sample_rate, H, W, iterations, max_cents):
    """`iterations` steps of ddsp_harm_refine from f0 [B, T, 1], anchored at f0."""
    B, T = f0.shape[:2]
    v = None if voiced is None else voiced.detach().to(torch.uint8).contiguous()
    ws = torch.empty(_lib.lib().ddsp_harm_refine_workspace_bytes(B, T, hop), device=audio.device, dtype=torch.uint8)
    track = f0
    with torch.cuda.device(audio.device):
        for _ in range(iterations):
            out = torch.empty_like(f0)
            rc = _lib.lib().ddsp_harm_refine(audio.data_ptr(), track.data_ptr(), f0.data_ptr(), None if v is None else v.data_ptr(),
                                             out.data_ptr(), None, None, ws.data_ptr(), B, T, hop, W, H, sample_rate, max_cents, 0,
                                             torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "ddsp_harm_refine")
            track = out
    return track


# ------------------------------------------------------------------------------------------------------------------- public

def _refined(audio, f0, voiced, hop, sample_rate, H, W, iterations, max_cents):
    """f0 after `iterations` steps (prepared tensors, B > 0); iterations = 0 returns f0 itself and launches nothing."""
    if iterations == 0:
        return f0
    if _in_kernel_range(audio, W, H):
        return _refine_device(audio, f0, voiced, hop, sample_rate, H, W, iterations, max_cents)
    track = f0
    for _ in range(iterations):
        track = _refine_torch(audio, track, f0, voiced, hop, sample_rate, H, W, max_cents)
    return track


def _check_refine(iterations, max_cents, what):
    iterations, max_cents = int(iterations), float(max_cents)
    if iterations < 0:
        raise ValueError(f"{what}: the number of refinement steps must be at least 0, got {iterations}")
    if not 0 < max_cents < math.inf:
        raise ValueError(f"{what}: max_cents must be positive and finite, got {max_cents}")
    return iterations, max_cents


def refine_f0(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, iterations=2, max_cents=50.0):
    """-> f0 [B, T, 1] after `iterations` refinement steps, every frame within `max_cents` of the track given; frames that are
    not finite, not positive or not voiced come back as they are."""
    B, T, hop, sample_rate, H = _check(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced, "refine_f0")
    iterations, max_cents = _check_refine(iterations, max_cents, "refine_f0")
    audio, f0, voiced = _prepare(audio, f0, voiced)
    if B == 0 or iterations == 0:
        return f0.clone()
    return _refined(audio, f0, voiced, hop, sample_rate, H, int(win_length), iterations, max_cents)


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


def harmonic_residual(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False, refine=0,
                      max_cents=50.0):
    """-> (harm [B, N], resid = audio - harm, dict(f0, a, c[, C])): the harmonic part of `audio` along `f0` (after `refine` steps of
    `refine_f0`) and what is left."""
    B, T, hop, sample_rate, H = _check(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced, "harmonic_residual")
    refine, max_cents = _check_refine(refine, max_cents, "harmonic_residual")
    W = int(win_length)
    audio, f0, voiced = _prepare(audio, f0, voiced)
    if B == 0:
        C, a, c = _empty(f0, T, hop, H, audio.dtype)
        return torch.zeros_like(audio), torch.zeros_like(audio), _controls(f0, a, c, C, return_complex)
    f0 = _refined(audio, f0, voiced, hop, sample_rate, H, W, refine, max_cents)
    if _in_kernel_range(audio, W, H):
        ws = _workspace(B, T, hop, audio.device)
        C, a, c = _analysis_device(audio, f0, voiced, hop, sample_rate, H, W, ws)
        harm, resid = _resynth_device(C, f0, audio, hop, sample_rate, ws, True)
    else:
        C, a, c = _analysis_torch(audio, f0, voiced, hop, sample_rate, H, W)
        harm = _resynth_torch(C, f0, hop, sample_rate)
        resid = audio - harm
    return harm, resid, _controls(f0, a, c, C, return_complex)


def harmonic_analysis(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced=None, return_complex=False, refine=0,
                      max_cents=50.0):
    """-> dict(f0 [B, T, 1], a [B, T, 1], c [B, T, H]) as `OscillatorBank` reads it, plus C (complex [B, T, H]) when asked.
    refine: steps of `refine_f0` (each within `max_cents` of f0) before the analysis; the dict's f0 is then the refined track."""
    B, T, hop, sample_rate, H = _check(audio, f0, hop, sample_rate, n_harmonics, win_length, voiced, "harmonic_analysis")
    refine, max_cents = _check_refine(refine, max_cents, "harmonic_analysis")
    W = int(win_length)
    audio, f0, voiced = _prepare(audio, f0, voiced)
    if B == 0:
        C, a, c = _empty(f0, T, hop, H, audio.dtype)
        return _controls(f0, a, c, C, return_complex)
    f0 = _refined(audio, f0, voiced, hop, sample_rate, H, W, refine, max_cents)
    if _in_kernel_range(audio, W, H):
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
    n_harmonics, sample_rate, hop_length and n_fft (the window), after `refine` steps of `refine_f0`.  No parameters."""

    def __init__(self, conf, refine=0):
        super().__init__()
        self.refine = _check_refine(refine, 50.0, "HarmonicAnalyzer")[0]
        self.n_harmonics = conf.n_harmonics
        self.sample_rate = conf.sample_rate
        self.hop_length = conf.hop_length
        self.win_length = conf.n_fft

    def forward(self, audio, f0, voiced=None):
        return harmonic_analysis(audio, f0, self.hop_length, self.sample_rate, self.n_harmonics, self.win_length, voiced=voiced,
                                 refine=self.refine)


# ------------------------------------------------------------------------------------------------------------ noise analysis

def _noise_tables(F: int, hop: int, dt, dev):
    """(A [M, F], d [M], Cos [F, L]): the non-zero rows of the impulse-response map (offsets e = j below M / 2, j - M above; samples
    d = e or hop + e) and c_l g[l] cos(pi b l / L); evaluated in fp64, rounded once to dt."""
    L, M = F - 1, 2 * (F - 1)
    j = torch.arange(M, device=dev)
    e = torch.where(j < L, j, j - M)
    b = torch.arange(F, device=dev)
    cb = torch.where((b == 0) | (b == F - 1), 1.0, 2.0).double()
    A = ((0.5 + 0.5 * torch.cos(math.pi * e.double() / L))[:, None] * (cb / M)[None, :]
         * torch.cos(math.pi * torch.remainder(b[None, :] * e[:, None], M).double() / L))
    lag = torch.arange(L, device=dev)
    cl = torch.where(lag == 0, 1.0, 2.0).double() * (0.5 + 0.5 * torch.cos(math.pi * lag.double() / L))
    Cos = cl[None, :] * torch.cos(math.pi * torch.remainder(b[:, None] * lag[None, :], M).double() / L)
    return A.to(dt), torch.where(e >= 0, e, hop + e), Cos.to(dt)


def _lagged(a: torch.Tensor, k: torch.Tensor, L: int, weights=None) -> torch.Tensor:
    """a, k [n, hop] -> [n, L]: sum_{d < hop - l} w[l][d] a[d] k[d + l], w = 1 or the truncation weights hop - l - d."""
    hop = a.shape[-1]
    out = torch.empty((a.shape[0], L), dtype=a.dtype, device=a.device)
    for lag in range(L):
        prod = a[:, :hop - lag] * k[:, lag:]
        out[:, lag] = (prod if weights is None else prod * weights[lag:]).sum(-1)
    return out


def _noise_spectrum(r: torch.Tensor, Cos: torch.Tensor) -> torch.Tensor:
    q = r @ Cos.T
    ext = torch.cat([q[:, 1:2], q, q[:, -2:-1]], dim=-1)
    return 0.25 * ext[:, :-2] + 0.5 * ext[:, 1:-1] + 0.25 * ext[:, 2:]


def _frame_average(r: torch.Tensor, average: int) -> torch.Tensor:
    """r [B, T, L] -> the mean over t' in [t - s, t + s] inside [0, T), s = (average - 1) / 2."""
    T = r.shape[1]
    s = min((average - 1) // 2, T - 1)
    rbar = torch.zeros_like(r)
    for o in range(-s, s + 1):                                   # t' = t + o ascending; no prefix sums: a NaN stays in its window
        t0, t1 = max(0, -o), T - max(0, o)
        rbar[:, t0:t1] += r[:, t0 + o:t1 + o]
    t = torch.arange(T, device=r.device)
    return rbar / ((t + s).clamp(max=T - 1) - (t - s).clamp(min=0) + 1).to(r.dtype)[None, :, None]


def _noise_torch(x, hop, F, average, iterations):
    dt, dev = x.dtype, x.device
    B = x.shape[0]
    T, L = x.shape[1] // hop, F - 1
    A, d, Cos = _noise_tables(F, hop, dt, dev)
    weights = torch.arange(hop, 0, -1, device=dev).to(dt)        # weights[l + d] = hop - l - d
    frames = x.reshape(B * T, hop)
    step = max(1, _CHUNK_ELEMENTS // hop)
    r = torch.cat([_lagged(frames[i:i + step], frames[i:i + step], L) for i in range(0, B * T, step)]).reshape(B, T, L)
    rbar = _frame_average(r, average)
    p = _noise_spectrum(rbar.reshape(B * T, L), Cos).clamp(min=0)                # (clamp keeps a NaN)
    H = torch.sqrt(3.0 * p / hop)
    tiny = torch.finfo(dt).tiny
    for _ in range(iterations):
        for i in range(0, B * T, step):
            Hc, pc = H[i:i + step], p[i:i + step]
            k = torch.zeros((Hc.shape[0], hop), dtype=dt, device=dev)
            k[:, d] = Hc @ A.T
            R = _lagged(k, k, L, weights) / 3.0
            H[i:i + step] = Hc * torch.sqrt(pc / _noise_spectrum(R, Cos).clamp(min=tiny))
    return H.reshape(B, T, F), p.reshape(B, T, F)


def _noise_ola_tables(F: int, dt, dev):
    """(HT [P, F], Cos [F, L]): the half response hh[d] = h[+-d] of unit vector b, (1/2 + 1/2 cos(pi d / P)) (c_b / M)
    cos(2 pi b d / M), and c_l g[l] cos(pi b l / L); evaluated in fp64, rounded once to dt."""
    P, M = F - 1, 2 * (F - 1)
    d = torch.arange(P, device=dev)
    b = torch.arange(F, device=dev)
    cb = torch.where((b == 0) | (b == F - 1), 1.0, 2.0).double()
    HT = ((0.5 + 0.5 * torch.cos(math.pi * d.double() / P))[:, None] * (cb / M)[None, :]
          * torch.cos(math.pi * torch.remainder(b[None, :] * d[:, None], M).double() / P))
    return HT.to(dt), _noise_tables(F, M, dt, dev)[2]


def _noise_ola_measure(x: torch.Tensor, hop: int, L: int) -> torch.Tensor:
    """x [B, N] -> r [B, T, L]: r_t[l] = (hop / c) sum_{n < hop, t hop + n + l < N} x[t hop + n] x[t hop + n + l], c the count of terms."""
    B, N = x.shape
    T = N // hop
    r = torch.zeros((B, T, L), dtype=x.dtype, device=x.device)
    step = max(1, _CHUNK_ELEMENTS // N)
    for lag in range(min(L, N)):
        for i in range(0, B, step):
            prod = torch.nn.functional.pad(x[i:i + step, :N - lag] * x[i:i + step, lag:], (0, lag))
            r[i:i + step, :, lag] = prod.reshape(-1, T, hop).sum(-1)
    count = (N - torch.arange(T, device=x.device)[:, None] * hop - torch.arange(L, device=x.device)[None, :]).clamp(0, hop)
    scale = torch.where(count > 0, hop / count.clamp(min=1).to(x.dtype), torch.zeros((), dtype=x.dtype, device=x.device))
    return r * scale[None]


def _noise_ola_torch(x, hop, F, average, iterations):
    dt, dev = x.dtype, x.device
    B = x.shape[0]
    T, L = x.shape[1] // hop, F - 1
    HT, Cos = _noise_ola_tables(F, dt, dev)
    rbar = _frame_average(_noise_ola_measure(x, hop, L), average)
    p = _noise_spectrum(rbar.reshape(B * T, L), Cos).clamp(min=0)                # (clamp keeps a NaN)
    H = torch.sqrt(3.0 * p / hop)
    tiny = torch.finfo(dt).tiny
    step = max(1, _CHUNK_ELEMENTS // (2 * L + 1))
    for _ in range(iterations):
        for i in range(0, B * T, step):
            Hc, pc = H[i:i + step], p[i:i + step]
            hh = Hc @ HT.T                                                       # [n, P]: h[d], d >= 0
            h = torch.cat([hh[:, 1:].flip(-1), hh], dim=-1)                      # h[e] at e + P - 1
            R = _lagged(h, h, L) * (hop / 3.0)
            H[i:i + step] = Hc * torch.sqrt(pc / _noise_spectrum(R, Cos).clamp(min=tiny))
    return H.reshape(B, T, F), p.reshape(B, T, F)


def _noise_in_kernel_range(x: torch.Tensor, hop: int, F: int) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and F <= NOISE_KERNEL_MAX_FILTERS and hop <= NOISE_KERNEL_MAX_HOP
            and x.shape[0] * (x.shape[1] // hop) <= NOISE_KERNEL_MAX_FRAMES)


def _noise_ola_in_kernel_range(x: torch.Tensor, hop: int, F: int) -> bool:
    return _noise_in_kernel_range(x, hop, F) and x.shape[1] < NOISE_OLA_KERNEL_MAX_SAMPLES


def _noise_device(x, hop, F, average, iterations, return_power, overlap_add=False):
    B, T = x.shape[0], x.shape[1] // hop
    name = "ddsp_noise_analysis_ola" if overlap_add else "ddsp_noise_analysis"
    H = torch.empty((B, T, F), device=x.device, dtype=torch.float32)
    p = torch.empty_like(H) if return_power else None
    ws = torch.empty(getattr(_lib.lib(), name + "_workspace_bytes")(B, T, F, hop), device=x.device, dtype=torch.uint8)
    with torch.cuda.device(x.device):
        rc = getattr(_lib.lib(), name)(x.data_ptr(), H.data_ptr(), None if p is None else p.data_ptr(), ws.data_ptr(), B, T, F,
                                       hop, min(average, 2 * T + 1), iterations, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, name)
    return H, p


def noise_analysis(x, hop, n_filters, average=1, iterations=None, return_power=False, overlap_add=False):
    """x [B, T hop] -> H [B, T, n_filters] >= 0 as `FilteredNoise` reads it (with return_power: (H, p), p [B, T, n_filters] the
    smoothed, lag-windowed spectrum of the averaged autocorrelation that H reproduces in expectation).  overlap_add: the model of
    FilteredNoise's overlap-add mode (any hop >= 1) instead of the truncated one; iterations=None: 16 and 8 of them."""
    what = "noise_analysis"
    overlap_add = bool(overlap_add)
    if iterations is None:
        iterations = NOISE_OLA_ITERATIONS if overlap_add else NOISE_ITERATIONS
    hop, F, average, iterations = int(hop), int(n_filters), int(average), int(iterations)
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be [B, N], got {tuple(x.shape)}")
    if F < 2 or hop < 1:
        raise ValueError(f"{what}: n_filters must be at least 2 and hop positive, got {F} and {hop}")
    if hop < 2 * (F - 1) and not overlap_add:
        raise ValueError(f"{what}: hop {hop} < 2 (n_filters - 1) = {2 * (F - 1)}: FilteredNoise crops the impulse response there "
                         "and H is not identifiable (its overlap-add mode, overlap_add=True, has no such limit)")
    if average < 1 or average % 2 == 0:
        raise ValueError(f"{what}: average must be an odd count of frames, got {average}")
    if iterations < 0:
        raise ValueError(f"{what}: iterations must be at least 0, got {iterations}")
    if x.shape[1] == 0 or x.shape[1] % hop:
        raise ValueError(f"{what}: x has {x.shape[1]} samples, which is no positive number of whole frames of hop {hop}")
    _refuse_grad(x, what)
    x = x.detach()
    if x.dtype not in (torch.float32, torch.float64):            # integers and 16-bit floats: analysed in fp32
        x = x.float()
    x = x.contiguous()
    if x.shape[0] == 0:
        H = torch.zeros((0, x.shape[1] // hop, F), dtype=x.dtype, device=x.device)
        return (H, torch.zeros_like(H)) if return_power else H
    if overlap_add:
        if _noise_ola_in_kernel_range(x, hop, F):
            H, p = _noise_device(x, hop, F, average, iterations, return_power, overlap_add=True)
        else:
            H, p = _noise_ola_torch(x, hop, F, average, iterations)
    elif _noise_in_kernel_range(x, hop, F):
        H, p = _noise_device(x, hop, F, average, iterations, return_power)
    else:
        H, p = _noise_torch(x, hop, F, average, iterations)
    return (H, p) if return_power else H


class NoiseAnalyzer(nn.Module):
    """forward(x [B, T hop], average=1, iterations=None) -> H [B, T, n_noise_filters]: `noise_analysis` at the configuration's
    n_noise_filters and hop_length.  overlap_add: None reads conf.noise_overlap_add (off where there is none), as `FilteredNoise`
    does.  No parameters."""

    def __init__(self, conf, overlap_add=None):
        super().__init__()
        self.n_filters = conf.n_noise_filters
        self.hop_length = conf.hop_length
        self.overlap_add = bool(getattr(conf, 'noise_overlap_add', False) if overlap_add is None else overlap_add)

    def forward(self, x, average=1, iterations=None):
        return noise_analysis(x, self.hop_length, self.n_filters, average=average, iterations=iterations,
                              overlap_add=self.overlap_add)


# ------------------------------------------------------------------------------------------------------- control transformation

def _per_frame(value, B, T_out, device, what, name):
    """A tensor [T'], [B, T'] or [B, T', 1] -> fp64 [B, T'] on `device` (T_out None: taken from the tensor)."""
    if value.device != device:
        raise ValueError(f"{what}: {name} is on {value.device}, the controls on {device}")
    _refuse_grad(value, what)
    v = value.detach()
    if v.dim() == 3 and v.shape[-1] == 1:
        v = v[..., 0]
    if v.dim() == 1:
        v = v[None, :].expand(B, -1)
    if v.dim() != 2 or v.shape[0] != B or v.shape[1] < 1 or (T_out is not None and v.shape[1] != T_out):
        raise ValueError(f"{what}: {name} must be [T'], [B, T'] or [B, T', 1] with B = {B}"
                         + ("" if T_out is None else f" and T' = {T_out}") + f", got {tuple(value.shape)}")
    return v.double()


def _semitone_ratio(value, B, T_out, device, what, name):
    """Semitones (a float or a per-frame tensor) -> the ratio 2^(value / 12) as contiguous fp32 [B, T']."""
    if torch.is_tensor(value):
        return torch.exp2(_per_frame(value, B, T_out, device, what, name) / 12.0).float().contiguous()
    semitones = float(value)
    ratio = 2.0 ** (semitones / 12.0) if math.isfinite(semitones) and abs(semitones) < 12.0 * 1024 else math.nan
    ratio = float(torch.tensor(ratio, dtype=torch.float32))     # as the kernel will see it
    if not 0.0 < ratio < math.inf:
        raise ValueError(f"{what}: {name} = {value!r} semitones is no finite, positive fp32 ratio")
    return torch.full((B, T_out), ratio, dtype=torch.float32, device=device)


def _source_frames(f0, a, c, pos, sample_rate):
    """What the transformation and the morph read of one sound (rules 1 to 3): f0, a [B, T], c [B, T, H] in
    one dtype, pos fp32 [B, T'] -> the amplitudes A [B, T, H] the bank plays, the frame pair i0, i1 and its weight lambda (fp64)
    of every output frame, the fp32 pitch at the position (no glide from an unvoiced neighbour) and whether a neighbour is voiced."""
    dt, dev = c.dtype, c.device
    B, T, H = c.shape
    zero = torch.zeros((), dtype=dt, device=dev)
    f32 = f0.float()
    voiced = torch.isfinite(f32) & (f32 > 0)                                        # [B, T]
    cm = torch.where(_harmonic_mask(f32[..., None], None, sample_rate, H), c, zero)
    S = cm.sum(-1)
    gain = torch.where(S == 0, zero, torch.where(voiced, a, zero) / torch.where(S == 0, torch.ones((), dtype=dt, device=dev), S))
    A = cm * gain[..., None]                                                        # the amplitudes the bank plays
    p = torch.nan_to_num(pos.double(), nan=0.0, posinf=float(T - 1), neginf=0.0).clamp(0.0, float(T - 1))
    i0 = p.floor().long()
    i1 = (i0 + 1).clamp(max=T - 1)
    lam64 = p - i0.double()
    fa, fb = f32.gather(1, i0), f32.gather(1, i1)
    va, vb = voiced.gather(1, i0), voiced.gather(1, i1)
    f0s = torch.where(va & vb, ((1.0 - lam64) * fa.double() + lam64 * fb.double()).float(), torch.where(va, fa, fb))
    return A, i0, i1, lam64, f0s, va | vb


def _envelope_at(Ai, u, m, mu):
    """E(u) of the rows Ai [B, Tc, H] at u [B, Tc, H'] (fp64), m = floor(u) kept in [1, H - 1] and mu = u - m in Ai's dtype."""
    H = Ai.shape[-1]
    zero = torch.zeros((), dtype=Ai.dtype, device=Ai.device)
    between = (1 - mu) * Ai.gather(2, m - 1) + mu * Ai.gather(2, m.clamp(max=H - 1))
    return torch.where(u < 1, Ai[..., :1], torch.where(u < H, between, torch.where(u == H, Ai[..., H - 1:], zero)))


def _transform_torch(f0, a, c, noise, pos, r, q, sample_rate, H_out):
    """The definition as torch ops in c's dtype: f0, a [B, T], c [B, T, H], noise [B, T, F] or None; pos, r, q fp32 [B, T'].  The
    masks, f0' and the weights' inputs are fp32 whatever the dtype, as the definition has them; u and v are formed in fp64."""
    dt, dev = c.dtype, c.device
    B, T, H = c.shape
    T_out = pos.shape[1]
    zero = torch.zeros((), dtype=dt, device=dev)
    ok = torch.isfinite(r) & (r > 0) & torch.isfinite(q) & (q > 0)                  # [B, T']
    one32 = torch.ones((), dtype=torch.float32, device=dev)
    r, q = torch.where(ok, r, one32), torch.where(ok, q, one32)
    A, i0, i1, lam64, f0s, present = _source_frames(f0, a, c, pos, sample_rate)
    live = ok & present
    f0o = torch.where(live, f0s * r, torch.zeros((), dtype=torch.float32, device=dev))             # fp32 [B, T']
    rq = r.double() / q.double()
    k_out = torch.arange(1, H_out + 1, device=dev)
    F = 0 if noise is None else noise.shape[-1]
    a_out = torch.empty((B, T_out), dtype=dt, device=dev)
    c_out = torch.empty((B, T_out, H_out), dtype=dt, device=dev)
    n_out = None if noise is None else torch.empty((B, T_out, F), dtype=dt, device=dev)
    step = max(1, _CHUNK_ELEMENTS // max(1, B * max(H, H_out, F)))
    for t0 in range(0, T_out, step):
        sl = slice(t0, t0 + step)
        lam = lam64[:, sl].to(dt)[..., None]                                        # [B, Tc, 1]
        u = k_out.double() * rq[:, sl, None]                                        # [B, Tc, H']
        m = u.clamp(max=float(H)).floor().long().clamp(1, max(1, H - 1))
        mu = (u - m.double()).to(dt)
        env = [_envelope_at(A.gather(1, idx[..., None].expand(-1, -1, H)), u, m, mu) for idx in (i0[:, sl], i1[:, sl])]
        amp = (1 - lam) * env[0] + lam * env[1]
        masked = k_out.float() * f0o[:, sl, None] > sample_rate // 2
        amp = torch.where(live[:, sl, None] & ~masked, amp, zero)
        total = amp.sum(-1)
        a_out[:, sl] = total
        c_out[:, sl] = torch.where(total[..., None] == 0, torch.full((), 1.0 / H_out, dtype=dt, device=dev), amp / total[..., None])
        if noise is not None:
            v = torch.arange(F, device=dev).double() / q[:, sl, None].double()      # [B, Tc, F]
            n = v.clamp(max=float(F - 1)).floor().long()
            nu = (v - n.double()).to(dt)
            band = []
            for idx in (i0[:, sl], i1[:, sl]):
                Ni = noise.gather(1, idx[..., None].expand(-1, -1, F))
                band.append((1 - nu) * Ni.gather(2, n) + nu * Ni.gather(2, (n + 1).clamp(max=F - 1)))
            n_out[:, sl] = torch.where(ok[:, sl, None] & (v <= F - 1), (1 - lam) * band[0] + lam * band[1], zero)
    return f0o.to(dt), a_out, c_out, n_out


def _transform_in_kernel_range(c, noise, T_out, H_out) -> bool:
    B, T, H = c.shape
    return (c.is_cuda and c.dtype == torch.float32 and H <= KERNEL_MAX_HARMONICS and H_out <= KERNEL_MAX_HARMONICS
            and (noise is None or noise.shape[-1] <= NOISE_KERNEL_MAX_FILTERS)
            and B * max(T, T_out) <= TRANSFORM_KERNEL_MAX_FRAMES)


def _transform_device(f0, a, c, noise, pos, r, q, sample_rate, H_out):
    B, T, H = c.shape
    T_out = pos.shape[1]
    f0_out = torch.empty((B, T_out), device=c.device, dtype=torch.float32)
    a_out = torch.empty_like(f0_out)
    c_out = torch.empty((B, T_out, H_out), device=c.device, dtype=torch.float32)
    n_out = None if noise is None else torch.empty((B, T_out, noise.shape[-1]), device=c.device, dtype=torch.float32)
    with torch.cuda.device(c.device):
        rc = _lib.lib().ddsp_transform_controls(f0.data_ptr(), a.data_ptr(), c.data_ptr(), None if noise is None else noise.data_ptr(),
                                                pos.data_ptr(), r.data_ptr(), q.data_ptr(), f0_out.data_ptr(), a_out.data_ptr(),
                                                c_out.data_ptr(), None if n_out is None else n_out.data_ptr(), B, T, T_out, H, H_out,
                                                1 if noise is None else noise.shape[-1], sample_rate,
                                                torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_transform_controls")
    return f0_out, a_out, c_out, n_out


def _control_arrays(ctrl, what):
    """The checks of a control dict -> f0, a [B, T], c [B, T, H], the noise bands [B, T, F] or None: detached, contiguous, in c's
    dtype where that is fp32 or fp64 (else fp32)."""
    for key in ("f0", "a", "c"):
        if key not in ctrl:
            raise ValueError(f"{what}: the control dict has no '{key}'")
    f0, a, c, noise = ctrl["f0"], ctrl["a"], ctrl["c"], ctrl.get("H")
    if f0.dim() != 3 or f0.shape[-1] != 1:
        raise ValueError(f"{what}: f0 must be [B, T, 1], got {tuple(f0.shape)}")
    B, T = f0.shape[:2]
    if tuple(a.shape) != (B, T, 1) or c.dim() != 3 or tuple(c.shape[:2]) != (B, T) or c.shape[-1] < 1 or T < 1:
        raise ValueError(f"{what}: a must be [B, T, 1] and c [B, T, H] with f0's {B} x {T} >= 1 frames, got {tuple(a.shape)} and {tuple(c.shape)}")
    if noise is not None and (noise.dim() != 3 or tuple(noise.shape[:2]) != (B, T) or noise.shape[-1] < 1):
        raise ValueError(f"{what}: the noise bands H must be [B, T, F], got {tuple(noise.shape)}")
    dev = c.device
    for name, v in (("f0", f0), ("a", a), ("H", noise)):
        if v is not None and v.device != dev:
            raise ValueError(f"{what}: {name} is on {v.device}, c on {dev}")
    for v in (f0, a, c, noise):
        if v is not None:
            _refuse_grad(v, what)
    dt = c.dtype if c.dtype in (torch.float32, torch.float64) else torch.float32
    f0, a, c = (v.detach().to(dt).contiguous() for v in (f0[..., 0], a[..., 0], c))
    return f0, a, c, None if noise is None else noise.detach().to(dt).contiguous()


def transform_controls(ctrl, sample_rate, stretch=1.0, transpose=0.0, formant=0.0, positions=None, n_harmonics=None) -> dict:
    """The control dict of `harmonic_analysis` (f0 [B, T, 1], a [B, T, 1], c [B, T, H], optionally the noise bands H [B, T, F]; other
    keys are dropped) stretched in time, transposed and formant-shifted -> a dict of the same keys with
    T' frames and n_harmonics (None: H) harmonics, for `OscillatorBank` / `Decoder.synthesize`.

    transpose, formant: semitones, a float or a tensor [T'], [B, T'] or [B, T', 1]; the pitch moves by r = 2^(transpose / 12), the
    spectral envelope (and the noise bands) by q = 2^(formant / 12).  formant=0 keeps the formants where they are whatever the
    transposition; formant=None lets them follow the pitch (q = r, every harmonic keeps its amplitude).
    stretch > 0: T' = max(1, floor(T stretch + 1/2)) frames that read the input at pos[t'] = (t' + 1/2) T / T' - 1/2, clamped to
    [0, T - 1].  positions ([T'] or [B, T'], in input frames) replaces it by any time map (freeze, reverse, ...).
    A per-frame value that is not usable (a ratio that is not finite and positive) silences its frame; a position outside
    [0, T - 1] is clamped.  CUDA fp32 controls with H, n_harmonics <= 256 and F <= 257 take the HIP kernel
    (csrc/ddsp_transform.hip); CPU tensors, fp64 and larger sizes run the same definition as torch ops.  No backward."""
    what = "transform_controls"
    f0, a, c, noise = _control_arrays(ctrl, what)
    B, T, H = c.shape
    dt, dev = c.dtype, c.device
    H_out = H if n_harmonics is None else int(n_harmonics)
    sample_rate = int(sample_rate)
    if H_out < 1 or sample_rate < 1:
        raise ValueError(f"{what}: n_harmonics and sample_rate must be positive, got {n_harmonics} and {sample_rate}")

    if positions is not None:
        if not (isinstance(stretch, (int, float)) and float(stretch) == 1.0):
            raise ValueError(f"{what}: positions replaces stretch; give one of them")
        if not torch.is_tensor(positions) or positions.dim() not in (1, 2):
            raise ValueError(f"{what}: positions must be a tensor [T'] or [B, T']")
        pos = _per_frame(positions, B, None, dev, what, "positions").float().contiguous()
        T_out = pos.shape[1]
    else:
        if torch.is_tensor(stretch):
            raise ValueError(f"{what}: stretch is one factor; a time map goes into positions")
        stretch = float(stretch)
        if not 0.0 < stretch < math.inf:
            raise ValueError(f"{what}: stretch must be positive and finite, got {stretch}")
        T_out = max(1, int(math.floor(T * stretch + 0.5)))
        pos = ((torch.arange(T_out, dtype=torch.float64, device=dev) + 0.5) * T / T_out - 0.5).clamp(0.0, float(T - 1))
        pos = pos.float()[None, :].expand(B, -1).contiguous()
    r = _semitone_ratio(transpose, B, T_out, dev, what, "transpose")
    q = r if formant is None else _semitone_ratio(formant, B, T_out, dev, what, "formant")

    if B == 0:
        out = dict(f0=torch.zeros((0, T_out, 1), dtype=dt, device=dev), a=torch.zeros((0, T_out, 1), dtype=dt, device=dev),
                   c=torch.zeros((0, T_out, H_out), dtype=dt, device=dev))
        if noise is not None:
            out["H"] = torch.zeros((0, T_out, noise.shape[-1]), dtype=dt, device=dev)
        return out
    path = _transform_device if _transform_in_kernel_range(c, noise, T_out, H_out) else _transform_torch
    f0_out, a_out, c_out, n_out = path(f0, a, c, noise, pos, r, q, sample_rate, H_out)
    out = dict(f0=f0_out[..., None], a=a_out[..., None], c=c_out)
    if n_out is not None:
        out["H"] = n_out
    return out


class ControlTransform(nn.Module):
    """forward(ctrl, stretch=1.0, transpose=0.0, formant=0.0, positions=None, n_harmonics=None) -> dict: `transform_controls` at the
    configuration's sample_rate.  No parameters."""

    def __init__(self, conf):
        super().__init__()
        self.sample_rate = conf.sample_rate

    def forward(self, ctrl, **keywords):
        return transform_controls(ctrl, self.sample_rate, **keywords)


# -------------------------------------------------------------------------------------------------------------- control morph

def _morph_torch(src_a, src_b, wf, wh, wn, sample_rate, H_out, hz):
    """The definition of DESIGN.md section 14c as torch ops in the controls' dtype.  src_X = (f0, a [B, T_X], c [B, T_X, H_X], noise
    [B, T_X, F] or None, pos fp32 [B, T']); wf, wh, wn fp32 [B, T'].  f0', the masks and the weights are fp32 whatever the dtype,
    u_X, exp2 and log2 fp64, as the definition has them."""
    c_a, c_b = src_a[2], src_b[2]
    dt, dev = c_a.dtype, c_a.device
    B, T_out = wf.shape
    zero, zero32 = torch.zeros((), dtype=dt, device=dev), torch.zeros((), dtype=torch.float32, device=dev)
    sane = torch.isfinite(wf) & torch.isfinite(wh) & torch.isfinite(wn)            # [B, T']
    wf, wh, wn = (torch.where(sane, w, zero32).clamp(0.0, 1.0) for w in (wf, wh, wn))
    srcs = []
    for f0, a, c, noise, pos in (src_a, src_b):
        A, i0, i1, lam64, f, present = _source_frames(f0, a, c, pos, sample_rate)
        present = present & sane
        srcs.append(dict(A=A, i0=i0, i1=i1, lam64=lam64, present=present, noise=noise, H=c.shape[-1],
                         f=torch.where(present, f, torch.ones((), dtype=torch.float32, device=dev))))
    sa, sb = srcs
    fa, fb, pa, pb = sa["f"], sb["f"], sa["present"], sb["present"]
    w64 = wf.double()
    mean = torch.exp2((1.0 - w64) * torch.log2(fa.double()) + w64 * torch.log2(fb.double())).float()
    mean = torch.minimum(torch.maximum(mean, torch.minimum(fa, fb)), torch.maximum(fa, fb))
    f0o = torch.where(pa & pb, torch.where(wf == 0, fa, torch.where(wf == 1, fb, mean)), torch.where(pa, fa, torch.where(pb, fb, zero32)))
    live = pa | pb
    for s in srcs:
        s["scale"] = torch.where(s["present"], f0o.double() / s["f"].double(), torch.ones((), dtype=torch.float64, device=dev)) if hz \
            else torch.ones((B, T_out), dtype=torch.float64, device=dev)
    k_out = torch.arange(1, H_out + 1, device=dev)
    F = 0 if sa["noise"] is None else sa["noise"].shape[-1]
    a_out = torch.empty((B, T_out), dtype=dt, device=dev)
    c_out = torch.empty((B, T_out, H_out), dtype=dt, device=dev)
    n_out = None if sa["noise"] is None else torch.empty((B, T_out, F), dtype=dt, device=dev)
    step = max(1, _CHUNK_ELEMENTS // max(1, B * max(sa["H"], sb["H"], H_out, F)))
    for t0 in range(0, T_out, step):
        sl = slice(t0, t0 + step)
        env, band = [], []
        for s in srcs:
            H = s["H"]
            lam = s["lam64"][:, sl].to(dt)[..., None]                               # [B, Tc, 1]
            u = k_out.double() * s["scale"][:, sl, None]                            # [B, Tc, H']
            m = u.clamp(max=float(H)).floor().long().clamp(1, max(1, H - 1))
            mu = (u - m.double()).to(dt)
            E = [_envelope_at(s["A"].gather(1, idx[..., None].expand(-1, -1, H)), u, m, mu) for idx in (s["i0"][:, sl], s["i1"][:, sl])]
            env.append(torch.where(s["present"][:, sl, None], (1 - lam) * E[0] + lam * E[1], zero))
            if n_out is not None:
                N = [s["noise"].gather(1, idx[..., None].expand(-1, -1, F)) for idx in (s["i0"][:, sl], s["i1"][:, sl])]
                band.append((1 - lam) * N[0] + lam * N[1])
        w = wh[:, sl, None].to(dt)
        amp = (1 - w) * env[0] + w * env[1]
        masked = k_out.float() * f0o[:, sl, None] > sample_rate // 2
        amp = torch.where(live[:, sl, None] & ~masked, amp, zero)
        total = amp.sum(-1)
        a_out[:, sl] = total
        c_out[:, sl] = torch.where(total[..., None] == 0, torch.full((), 1.0 / H_out, dtype=dt, device=dev), amp / total[..., None])
        if n_out is not None:
            w = wn[:, sl, None].to(dt)
            n_out[:, sl] = torch.where(sane[:, sl, None], (1 - w) * band[0] + w * band[1], zero)
    return f0o.to(dt), a_out, c_out, n_out


def _morph_in_kernel_range(src_a, src_b, T_out, H_out) -> bool:
    c_a, c_b, noise = src_a[2], src_b[2], src_a[3]
    B = c_a.shape[0]
    return (c_a.is_cuda and c_a.dtype == torch.float32 and max(c_a.shape[-1], c_b.shape[-1], H_out) <= KERNEL_MAX_HARMONICS
            and (noise is None or noise.shape[-1] <= NOISE_KERNEL_MAX_FILTERS)
            and B * max(c_a.shape[1], c_b.shape[1], T_out) <= MORPH_KERNEL_MAX_FRAMES)


def _morph_device(src_a, src_b, wf, wh, wn, sample_rate, H_out, hz):
    c_a, c_b, noise = src_a[2], src_b[2], src_a[3]
    B, T_out = wf.shape
    F = 1 if noise is None else noise.shape[-1]
    f0_out = torch.empty((B, T_out), device=c_a.device, dtype=torch.float32)
    a_out = torch.empty_like(f0_out)
    c_out = torch.empty((B, T_out, H_out), device=c_a.device, dtype=torch.float32)
    n_out = None if noise is None else torch.empty((B, T_out, F), device=c_a.device, dtype=torch.float32)
    ptr = lambda v: None if v is None else v.data_ptr()                                           # noqa: E731
    with torch.cuda.device(c_a.device):
        rc = _lib.lib().ddsp_morph_controls(*(ptr(v) for v in src_a), *(ptr(v) for v in src_b), wf.data_ptr(), wh.data_ptr(),
                                            wn.data_ptr(), f0_out.data_ptr(), a_out.data_ptr(), c_out.data_ptr(), ptr(n_out), B,
                                            c_a.shape[1], c_b.shape[1], T_out, c_a.shape[-1], c_b.shape[-1], H_out, F, sample_rate,
                                            MORPH_COORDINATES['hz' if hz else 'harmonic'], torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_morph_controls")
    return f0_out, a_out, c_out, n_out


def _mix_weight(value, B, T_out, device, what, name):
    """The weight of sound B (a float or a per-frame tensor) -> contiguous fp32 [B, T']; a float must be finite and is clamped to
    [0, 1], a tensor's values are left to the definition (never synchronised on)."""
    if torch.is_tensor(value):
        return _per_frame(value, B, T_out, device, what, name).float().contiguous()
    weight = float(value)
    if not math.isfinite(weight):
        raise ValueError(f"{what}: {name} = {value!r} is not finite")
    return torch.full((B, T_out), min(1.0, max(0.0, weight)), dtype=torch.float32, device=device)


def morph_controls(ctrl_a, ctrl_b, sample_rate, mix=0.5, mix_f0=None, mix_harmonics=None, mix_noise=None, coordinates='hz',
                   frames=None, positions_a=None, positions_b=None, n_harmonics=None) -> dict:
    """Two control dicts of `harmonic_analysis` (f0, a [B, T_x, 1], c [B, T_x, H_x], optionally the noise bands H [B, T_x, F] in both;
    the same B, device and dtype; T_a != T_b and H_a != H_b are fine; other keys are dropped) -> the dict of a sound whose pitch,
    spectral envelope and noise bands lie between theirs, with T' frames and n_harmonics (None: the
    larger of H_a and H_b) harmonics, for `OscillatorBank` / `Decoder.synthesize`.

    mix: the weight of sound B, 0 is sound A and 1 is sound B; a float (finite, clamped to [0, 1]) or a tensor [T'], [B, T'] or
    [B, T', 1].  mix_f0, mix_harmonics and mix_noise replace it for the pitch (interpolated in log frequency), the harmonic
    amplitudes and the noise bands; None means mix.  A frame with a weight that is not finite is silent.
    coordinates: 'hz' compares the two envelopes at equal frequency (output harmonic k' reads each sound at k' f0' / f_x of its own
    harmonics, so a formant both sounds have stays where it is whatever the pitches); 'harmonic' compares them harmonic by harmonic.
    frames: T' (None: T_a); each sound is read at pos_x[t'] = (t' + 1/2) T_x / T' - 1/2 clamped to [0, T_x - 1].  positions_a and
    positions_b ([T'] or [B, T'], in that sound's frames) replace a sound's map by any map -- an alignment found elsewhere goes in
    here; T' is then their length.
    CUDA fp32 controls with at most 256 harmonics (in and out) and 257 bands take the HIP kernel (csrc/ddsp_morph.hip), one
    launch; CPU tensors, fp64 and larger sizes run the same definition as torch ops.  No backward."""
    what = "morph_controls"
    if coordinates not in MORPH_COORDINATES:
        raise ValueError(f"{what}: coordinates must be 'hz' or 'harmonic', got {coordinates!r}")
    src_a, src_b = _control_arrays(ctrl_a, what + " (sound A)"), _control_arrays(ctrl_b, what + " (sound B)")
    c_a, c_b = src_a[2], src_b[2]
    B, T_a, H_a = c_a.shape
    dt, dev = c_a.dtype, c_a.device
    if c_b.shape[0] != B or c_b.device != dev or ctrl_a["c"].dtype != ctrl_b["c"].dtype:
        raise ValueError(f"{what}: the two sounds must have the same batch, device and dtype, got {tuple(c_a.shape)} {ctrl_a['c'].dtype} "
                         f"on {dev} and {tuple(c_b.shape)} {ctrl_b['c'].dtype} on {c_b.device}")
    if (src_a[3] is None) != (src_b[3] is None) or (src_a[3] is not None and src_a[3].shape[-1] != src_b[3].shape[-1]):
        raise ValueError(f"{what}: the noise bands H must be in both dicts with the same number of bands, or in neither")
    H_out = max(H_a, c_b.shape[-1]) if n_harmonics is None else int(n_harmonics)
    sample_rate = int(sample_rate)
    if H_out < 1 or sample_rate < 1:
        raise ValueError(f"{what}: n_harmonics and sample_rate must be positive, got {n_harmonics} and {sample_rate}")

    given = {}
    for name, positions in (("positions_a", positions_a), ("positions_b", positions_b)):
        if positions is not None:
            if not torch.is_tensor(positions) or positions.dim() not in (1, 2):
                raise ValueError(f"{what}: {name} must be a tensor [T'] or [B, T']")
            given[name] = _per_frame(positions, B, None, dev, what, name).float().contiguous()
    lengths = {v.shape[1] for v in given.values()}
    if len(lengths) > 1:
        raise ValueError(f"{what}: positions_a and positions_b have different lengths {sorted(lengths)}")
    T_out = lengths.pop() if lengths else (T_a if frames is None else int(frames))
    if T_out < 1 or (frames is not None and int(frames) != T_out):
        raise ValueError(f"{what}: frames = {frames!r} must be positive and agree with the {T_out} positions given")
    maps = []
    for name, T in (("positions_a", T_a), ("positions_b", c_b.shape[1])):
        if name in given:
            maps.append(given[name])
        else:
            pos = ((torch.arange(T_out, dtype=torch.float64, device=dev) + 0.5) * T / T_out - 0.5).clamp(0.0, float(T - 1))
            maps.append(pos.float()[None, :].expand(B, -1).contiguous())
    overrides = (("mix_f0", mix_f0), ("mix_harmonics", mix_harmonics), ("mix_noise", mix_noise))
    shared = _mix_weight(mix, B, T_out, dev, what, "mix") if any(v is None for _, v in overrides) else None   # expanded once
    wf, wh, wn = (shared if v is None else _mix_weight(v, B, T_out, dev, what, name) for name, v in overrides)

    if B == 0:
        out = dict(f0=torch.zeros((0, T_out, 1), dtype=dt, device=dev), a=torch.zeros((0, T_out, 1), dtype=dt, device=dev),
                   c=torch.zeros((0, T_out, H_out), dtype=dt, device=dev))
        if src_a[3] is not None:
            out["H"] = torch.zeros((0, T_out, src_a[3].shape[-1]), dtype=dt, device=dev)
        return out
    src_a, src_b = src_a + (maps[0],), src_b + (maps[1],)
    path = _morph_device if _morph_in_kernel_range(src_a, src_b, T_out, H_out) else _morph_torch
    f0_out, a_out, c_out, n_out = path(src_a, src_b, wf, wh, wn, sample_rate, H_out, coordinates == 'hz')
    out = dict(f0=f0_out[..., None], a=a_out[..., None], c=c_out)
    if n_out is not None:
        out["H"] = n_out
    return out


class ControlMorph(nn.Module):
    """forward(ctrl_a, ctrl_b, mix=0.5, mix_f0=None, mix_harmonics=None, mix_noise=None, coordinates='hz', frames=None,
    positions_a=None, positions_b=None, n_harmonics=None) -> dict: `morph_controls` at the configuration's sample_rate.  No parameters."""

    def __init__(self, conf):
        super().__init__()
        self.sample_rate = conf.sample_rate

    def forward(self, ctrl_a, ctrl_b, **keywords):
        return morph_controls(ctrl_a, ctrl_b, self.sample_rate, **keywords)


# ----------------------------------------------------------------------------------------------------------- time alignment

def _dtw_torch(x_a, x_b, radius, penalty):
    """The recurrence of DESIGN.md section 14d as torch ops in the features' dtype, one anti-diagonal at a time, and the walk back
    one step of all rows at a time (no host synchronisation): x_a [B, T_a, D], x_b [B, T_b, D] -> path int32 [B, T_a + T_b - 1, 2]
    (-1 beyond length), length int32 [B], cost [B].  radius: an int or None."""
    dt, dev = x_a.dtype, x_a.device
    B, T_a, D = x_a.shape
    T_b = x_b.shape[1]
    inf = torch.full((), math.inf, dtype=dt, device=dev)
    d = torch.zeros((B, T_a, T_b), dtype=dt, device=dev)
    for k in range(D):                                          # ascending k, one accumulator
        t = x_a[:, :, None, k] - x_b[:, None, :, k]
        d = d + t * t
    d = torch.where(d < inf, d, inf)                            # a NaN too
    if radius is not None:
        p, q = T_a - 1, T_b - 1
        i, j = torch.arange(T_a, device=dev)[:, None], torch.arange(T_b, device=dev)[None, :]
        d = torch.where((i * q - j * p).abs() <= radius * max(p, q), d, inf)
    pen = torch.full((), penalty, dtype=dt, device=dev)
    total = torch.empty_like(d)
    back = torch.zeros((B, T_a, T_b), dtype=torch.uint8, device=dev)
    total[:, 0, 0] = d[:, 0, 0]
    for n in range(1, T_a + T_b - 1):
        i = torch.arange(max(0, n - T_b + 1), min(n, T_a - 1) + 1, device=dev)
        j = n - i
        im, jm = (i - 1).clamp(min=0), (j - 1).clamp(min=0)
        best, up, left = total[:, im, jm], total[:, im, j] + pen, total[:, i, jm] + pen
        code = torch.zeros_like(best, dtype=torch.uint8)
        take = up < best
        best, code = torch.where(take, up, best), torch.where(take, 1, code)
        take = left < best
        best, code = torch.where(take, left, best), torch.where(take, 2, code)
        first_row, first_col = (i == 0)[None, :], (j == 0)[None, :]
        best = torch.where(first_row, left, torch.where(first_col, up, best))
        code = torch.where(first_row, 2, torch.where(first_col, 1, code)).to(torch.uint8)
        total[:, i, j] = d[:, i, j] + best
        back[:, i, j] = code
    longest = T_a + T_b - 1
    rows = torch.arange(B, device=dev)
    i = torch.full((B,), T_a - 1, dtype=torch.long, device=dev)
    j = torch.full((B,), T_b - 1, dtype=torch.long, device=dev)
    active = torch.ones((B,), dtype=torch.bool, device=dev)
    length = torch.zeros((B,), dtype=torch.long, device=dev)
    backwards = torch.full((B, longest, 2), -1, dtype=torch.long, device=dev)
    for n in range(longest):
        backwards[:, n, 0], backwards[:, n, 1] = torch.where(active, i, -1), torch.where(active, j, -1)
        length = length + active
        code = back[rows, i, j]
        active = active & ((i > 0) | (j > 0))
        di = torch.where(i == 0, 0, torch.where(j == 0, 1, (code != 2).long()))
        dj = torch.where(i == 0, 1, torch.where(j == 0, 0, (code != 1).long()))
        i, j = torch.where(active, i - di, i), torch.where(active, j - dj, j)
    k = torch.arange(longest, device=dev)[None, :]
    src = (length[:, None] - 1 - k).clamp(min=0)
    path = torch.where((k < length[:, None])[..., None], backwards.gather(1, src[..., None].expand(-1, -1, 2)), -1)
    return path.int(), length.int(), total[:, T_a - 1, T_b - 1]


def _timeline_torch(path, length, T_a, T_b, tau, T_out):
    """The path resampled onto T' frames in fp64 -> positions_a, positions_b fp32 [B, T']."""
    dev = path.device
    pi, pj = path[..., 0].double(), path[..., 1].double()
    wa, wb = 1.0 - tau, tau
    on = torch.arange(path.shape[1], device=dev)[None, :] < length[:, None]
    s_k = torch.where(on, wa * pi + wb * pj, torch.full((), math.inf, dtype=torch.float64, device=dev))
    S = wa * float(T_a - 1) + wb * float(T_b - 1)
    t = torch.arange(T_out, dtype=torch.float64, device=dev)
    s = (t * S / float(T_out - 1)).clamp(max=S) if T_out > 1 else torch.zeros_like(t)
    s = s[None, :].expand(path.shape[0], -1).contiguous()
    k = (torch.searchsorted(s_k, s, right=True) - 1).clamp(min=0)          # the largest k with s_k <= s
    nxt = torch.minimum(k + 1, length[:, None].long() - 1)
    s0, s1 = s_k.gather(1, k), s_k.gather(1, nxt)
    lam = torch.where(nxt > k, (s - s0) / torch.where(nxt > k, s1 - s0, torch.ones_like(s)), torch.zeros_like(s))
    out = []
    for v in (pi, pj):
        v0 = v.gather(1, k)
        out.append((v0 + lam * (v.gather(1, nxt) - v0)).float())
    return out[0], out[1]


def _dtw_in_kernel_range(x_a, x_b, T_out) -> bool:
    return (x_a.is_cuda and x_a.dtype == torch.float32 and max(x_a.shape[1], x_b.shape[1]) <= DTW_KERNEL_MAX_FRAMES
            and x_a.shape[2] <= DTW_KERNEL_MAX_FEATURES and max(x_a.shape[0], T_out) <= 2 ** 31 - 1)


def _dtw_device(x_a, x_b, radius, penalty, tau, T_out):
    B, T_a, D = x_a.shape
    T_b = x_b.shape[1]
    dev = x_a.device
    L = _lib.lib()
    pos_a = torch.empty((B, T_out), dtype=torch.float32, device=dev)
    pos_b = torch.empty_like(pos_a)
    path = torch.empty((B, T_a + T_b - 1, 2), dtype=torch.int32, device=dev)
    length = torch.empty((B,), dtype=torch.int32, device=dev)
    cost = torch.empty((B,), dtype=torch.float32, device=dev)
    nbytes = L.ddsp_dtw_workspace_bytes(B, T_a, T_b)
    workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.ddsp_dtw_align(x_a.data_ptr(), x_b.data_ptr(), pos_a.data_ptr(), pos_b.data_ptr(), path.data_ptr(), length.data_ptr(),
                              cost.data_ptr(), workspace.data_ptr(), nbytes, B, T_a, T_b, D, T_out, 0 if radius is None else radius,
                              penalty, tau, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_dtw_align")
    return pos_a, pos_b, path, length, cost


def dtw_align(x_a, x_b, radius=None, penalty=0.0, timing=0.0, frames=None, return_path=False):
    """Dynamic time warping of two feature sequences x_a [B, T_a, D] and x_b [B, T_b, D] (any features; `control_features` makes
    them of control dicts) -> positions_a, positions_b fp32 [B, T'], which frame of each sound every output frame reads: what
    `morph_controls` takes.  With return_path=True also path int32 [B, T_a + T_b - 1, 2] (the cells (i, j)
    from (0, 0) to the end cell, -1 beyond length), length int32 [B] and cost [B].

    The local cost of frames i and j is the squared distance of their rows; a value that is not finite counts as +inf.  The path
    steps diagonally, or by one frame of either sound at `penalty` (>= 0, finite) on top of the cost, which discourages long runs
    that freeze one sound; ties go to the diagonal, then to the step in A.  radius (an integer >= 1, None: no band) keeps the path
    within `radius` frames of the longer sound around the straight diagonal (a Sakoe-Chiba band in integer arithmetic).
    timing in [0, 1] (clamped) chooses whose clock the output follows: 0 is A's (T' = T_a: positions_a = 0, 1, 2, ...), 1 is B's,
    between them both are warped; frames sets T' (None: floor((1 - timing) T_a + timing T_b + 1/2), at least 1).
    CUDA fp32 features with D <= 64 and T_a, T_b <= 2048 take the HIP kernel (csrc/ddsp_align.hip), one launch; CPU tensors, fp64
    and larger sizes run the same definition as torch ops, one anti-diagonal at a time.  No backward."""
    what = "dtw_align"
    for name, v in (("x_a", x_a), ("x_b", x_b)):
        if not torch.is_tensor(v) or v.dim() != 3 or v.shape[1] < 1 or v.shape[2] < 1 or not v.is_floating_point():
            raise ValueError(f"{what}: {name} must be a floating-point tensor [B, T, D] with T, D >= 1")
        _refuse_grad(v, what)
    if x_a.shape[0] != x_b.shape[0] or x_a.shape[2] != x_b.shape[2] or x_a.device != x_b.device or x_a.dtype != x_b.dtype:
        raise ValueError(f"{what}: the two sequences must have the same batch, feature count, device and dtype, got "
                         f"{tuple(x_a.shape)} {x_a.dtype} on {x_a.device} and {tuple(x_b.shape)} {x_b.dtype} on {x_b.device}")
    if radius is not None and (isinstance(radius, bool) or not isinstance(radius, int) or radius < 1):
        raise ValueError(f"{what}: radius must be an integer >= 1 or None, got {radius!r}")
    penalty, timing = float(penalty), float(timing)
    if not (0.0 <= penalty < math.inf):
        raise ValueError(f"{what}: penalty must be finite and >= 0, got {penalty}")
    if not math.isfinite(timing):
        raise ValueError(f"{what}: timing must be finite, got {timing}")
    tau = min(1.0, max(0.0, timing))
    B, T_a, D = x_a.shape
    T_b = x_b.shape[1]
    T_out = max(1, int(math.floor((1.0 - tau) * T_a + tau * T_b + 0.5))) if frames is None else int(frames)
    if T_out < 1:
        raise ValueError(f"{what}: frames must be positive, got {frames!r}")
    if radius is not None and radius > max(T_a, T_b) - 1:
        radius = None                                           # such a band holds every cell
    dt = x_a.dtype if x_a.dtype in (torch.float32, torch.float64) else torch.float32
    x_a, x_b = x_a.detach().to(dt).contiguous(), x_b.detach().to(dt).contiguous()
    if B == 0:
        dev = x_a.device
        out = (torch.zeros((0, T_out), dtype=torch.float32, device=dev), torch.zeros((0, T_out), dtype=torch.float32, device=dev))
        return out + (torch.zeros((0, T_a + T_b - 1, 2), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev),
                      torch.zeros((0,), dtype=dt, device=dev)) if return_path else out
    if _dtw_in_kernel_range(x_a, x_b, T_out):
        pos_a, pos_b, path, length, cost = _dtw_device(x_a, x_b, radius, penalty, tau, T_out)
    else:
        path, length, cost = _dtw_torch(x_a, x_b, radius, penalty)
        pos_a, pos_b = _timeline_torch(path, length, T_a, T_b, tau, T_out)
    return (pos_a, pos_b, path, length, cost) if return_path else (pos_a, pos_b)


def _level(x, range_log2):
    """l(x) = (log2(max(x, 2^-L)) + L) / L: 0 at and below 2^-L, 1 at 1."""
    return (torch.log2(x.clamp(min=2.0 ** -range_log2)) + range_log2) / range_log2


def _over_row_max(x):
    """x [B, ...] over its row's largest value; a row whose largest value is 0 stays 0."""
    top = x.flatten(1).amax(1)
    return x / torch.where(top > 0, top, torch.ones_like(top)).reshape((-1,) + (1,) * (x.dim() - 1))


def control_features(ctrl, sample_rate, n_bands=32, noise_groups=8, range_log2=10.0):
    """What makes two control dicts comparable frame by frame: [B, T, D] in the controls' dtype,
    D = n_bands + 2 (+ noise_groups where the dict has the noise bands H), every value in [0, 1] over `range_log2` octaves of level:
      the spectral envelope the bank plays, sampled at m (sample_rate // 2) / n_bands Hz, m = 1 .. n_bands -- on a frequency grid
      that does not move with the pitch, so a phrase aligns with the same phrase sung a fifth higher; relative to the row's
      largest sample, in log2, over sqrt(n_bands);
      the noise bands pooled by their mean into `noise_groups` groups, the same way, over sqrt(noise_groups);
      the level a relative to the row's largest voiced a, in log2 (0 on unvoiced frames); and 1 on voiced frames, 0 on unvoiced."""
    what = "control_features"
    f0, a, c, noise = _control_arrays(ctrl, what)
    n_bands, noise_groups, range_log2, sample_rate = int(n_bands), int(noise_groups), float(range_log2), int(sample_rate)
    if n_bands < 1 or noise_groups < 1 or sample_rate < 2 or not 0.0 < range_log2 < math.inf:
        raise ValueError(f"{what}: n_bands, noise_groups and range_log2 must be positive and sample_rate at least 2")
    dt = c.dtype
    spacing = (sample_rate // 2) / n_bands
    voiced = torch.isfinite(f0) & (f0 > 0)
    semitones = 12.0 * torch.log2(spacing / f0.double())       # unvoiced: no usable ratio, and the frame comes out silent
    on_grid = transform_controls(dict(f0=f0[..., None], a=a[..., None], c=c), sample_rate, transpose=semitones, formant=0.0,
                                 n_harmonics=n_bands)
    parts = [_level(_over_row_max(on_grid["a"] * on_grid["c"]), range_log2) / math.sqrt(n_bands)]
    if noise is not None:
        F = noise.shape[-1]
        edges = [(g * F) // noise_groups for g in range(noise_groups + 1)]
        pooled = torch.stack([noise[..., lo:hi].mean(-1) if hi > lo else torch.zeros_like(a) for lo, hi in zip(edges, edges[1:])], -1)
        parts.append(_level(_over_row_max(pooled), range_log2) / math.sqrt(noise_groups))
    zero = torch.zeros((), dtype=dt, device=c.device)
    parts.append(torch.where(voiced, _level(_over_row_max(torch.where(voiced, a, zero)), range_log2), zero)[..., None])
    parts.append(voiced.to(dt)[..., None])
    return torch.cat(parts, -1)


def align_controls(ctrl_a, ctrl_b, sample_rate, radius=None, penalty=0.0, timing=0.0, frames=None, return_path=False, **features):
    """`control_features` of two control dicts (the same B and device; the noise bands H in both with one F, or in neither) and
    `dtw_align` of the two -> positions_a, positions_b [B, T'] for `morph_controls` (and the path, its length and its cost with
    return_path=True).  `features`: control_features' n_bands, noise_groups and range_log2."""
    what = "align_controls"
    src_a, src_b = _control_arrays(ctrl_a, what + " (sound A)"), _control_arrays(ctrl_b, what + " (sound B)")
    c_a, c_b = src_a[2], src_b[2]
    if c_a.shape[0] != c_b.shape[0] or c_a.device != c_b.device or c_a.dtype != c_b.dtype:
        raise ValueError(f"{what}: the two sounds must have the same batch, device and dtype, got {tuple(c_a.shape)} {c_a.dtype} on "
                         f"{c_a.device} and {tuple(c_b.shape)} {c_b.dtype} on {c_b.device}")
    if (src_a[3] is None) != (src_b[3] is None) or (src_a[3] is not None and src_a[3].shape[-1] != src_b[3].shape[-1]):
        raise ValueError(f"{what}: the noise bands H must be in both dicts with the same number of bands, or in neither")
    return dtw_align(control_features(ctrl_a, sample_rate, **features), control_features(ctrl_b, sample_rate, **features),
                     radius=radius, penalty=penalty, timing=timing, frames=frames, return_path=return_path)


class ControlAlign(nn.Module):
    """forward(ctrl_a, ctrl_b, radius=None, penalty=0.0, timing=0.0, frames=None, return_path=False, **features): `align_controls`
    at the configuration's sample_rate.  No parameters."""

    def __init__(self, conf):
        super().__init__()
        self.sample_rate = conf.sample_rate

    def forward(self, ctrl_a, ctrl_b, **keywords):
        return align_controls(ctrl_a, ctrl_b, self.sample_rate, **keywords)
