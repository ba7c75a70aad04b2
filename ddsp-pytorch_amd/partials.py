"""Inharmonic analysis: the inverse of `InharmonicBank` (include/ddsp_hip.h: ddsp_partials_*).

Given audio [B, N] and K frequency tracks f [B, T, K] in Hz (N = T hop), the per-frame complex amplitudes C [B, T, K] of the
partials along the bank's own fp64 phase tracks, the bank's controls a = sum_k |C| and c = |C| / a, each partial's reassigned
frequency, the tonal part of the audio and the residual the partials do not explain; and on top of these the fit that turns a
recording and a rough pitch track into the controls and the starting parameters of a `synth='inharmonic'` decoder:

  partial_analysis(audio, f, hop, sample_rate, win_length, voiced=None, return_complex=False, reassign=False)
                                                                        -> dict(f, a, c[, C][, f_re])
  partial_resynthesis(C, f, hop, sample_rate) -> harm [B, T hop]
  partial_residual(audio, f, hop, sample_rate, win_length, voiced=None, return_complex=False, reassign=False)
                                                                        -> (harm, resid, the dict of partial_analysis)
  refine_partials(audio, f, hop, sample_rate, win_length, voiced=None, iterations=2, max_cents=50.0) -> f [B, T, K]
  fit_inharmonicity(f, weight, base_ratios=None, f0=None) -> (f0 [B, T, 1], B_coef [B])
  inharmonic_analysis(audio, f0, hop, sample_rate, n_partials, win_length, voiced=None, inharmonicity=0.0, base_ratios=None,
                      iterations=4, max_cents=50.0, model='stiff', return_complex=False)
                                                                        -> dict(f0, ratios [B, T, K], a, c, inharmonicity [B][, C])
  PartialAnalyzer(conf, ...)   nn.Module without parameters over conf.n_harmonics / sample_rate / hop_length / n_fft (the window)

The harmonic analysis (analysis.py) demodulates with k theta from one phase word, which puts partial k at exactly k f0; the 24th
partial of a 110 Hz string with B = 3e-4 sits 140 cents above that, outside a 1024-point window's main lobe.  Here every partial
is demodulated along its own track, its frequency is read back by reassignment (`f_re`, one value per partial and frame), and
`fit_inharmonicity` fits f0 and the stiffness B of f_k = f0 r_k sqrt(1 + B r_k^2) to the measured tracks in closed form.
`inharmonic_analysis` alternates the two; model='stiff' returns the fitted series, model='free' every partial's own measured
track (bells, beating pairs).  `decoder.synthesize` plays the returned dict on a `synth='inharmonic'` decoder, and
`InharmonicBank.init_from` takes the trainable parameters' starting values from it.

The returned `f` (and `f0`) is the track the analysis demodulated with: the input with entries that are not finite or <= 0 set
to 0.  CUDA fp32 tensors with an even win_length <= 4096, at most 256 partials, hop <= 1024 and T hop <= 2^24 take the HIP
kernels (csrc/ddsp_partials.hip); CPU tensors, fp64 and calls outside that range run the same definition as stock torch ops: the
phase is always the fp64 closed form, everything else is in the input's dtype, frames and samples in chunks that bound the
memory.  No backward.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib
from .analysis import _CHUNK_ELEMENTS, _up          # the bank's upsampling; the torch path's largest intermediate
from .encoder import _refuse_grad

KERNEL_MAX_WINDOW = 4096                 # csrc/ddsp_partials.hip: kMaxW, kMaxK, kMaxHop, kMaxSamples
KERNEL_MAX_PARTIALS = 256
KERNEL_MAX_HOP = 1024
KERNEL_MAX_SAMPLES = 1 << 24
KERNEL_MAX_CELLS = 1 << 40               # B T K and B T hop
PHASE_READY = 1                          # include/ddsp_hip.h: DDSP_PARTIALS_PHASE_READY
MODELS = ('stiff', 'free')
MAX_INHARMONICITY = 1.0                  # the fit's B is kept in [0, 1]; a piano's lowest strings reach about 1e-3


def _check(audio, f, hop, sample_rate, win_length, voiced, what):
    if f.dim() != 3 or f.shape[-1] < 1:
        raise ValueError(f"{what}: f must be [B, T, K] with K >= 1, got {tuple(f.shape)}")
    B, T, K = f.shape
    hop, sample_rate = int(hop), int(sample_rate)
    if hop < 1 or sample_rate < 1 or T < 1:
        raise ValueError(f"{what}: hop, sample_rate and the number of frames must be positive")
    if win_length is not None and (int(win_length) < 2 or int(win_length) % 2):
        raise ValueError(f"{what}: win_length must be even and at least 2, got {win_length}")
    if audio is not None:
        if audio.dim() != 2 or audio.shape[0] != B:
            raise ValueError(f"{what}: audio must be [B, N] with f's batch, got {tuple(audio.shape)} and f {tuple(f.shape)}")
        if audio.shape[1] != T * hop:
            raise ValueError(f"{what}: audio has {audio.shape[1]} samples, f has {T} frames of hop {hop} = {T * hop}")
        if audio.device != f.device:
            raise ValueError(f"{what}: audio and f are on different devices")
        _refuse_grad(audio, what)
    _refuse_grad(f, what)
    if voiced is not None and tuple(voiced.shape) != (B, T, 1):
        raise ValueError(f"{what}: voiced must be [B, T, 1], got {tuple(voiced.shape)}")
    if voiced is not None and voiced.device != f.device:         # (the kernel would read a host address)
        raise ValueError(f"{what}: voiced is on {voiced.device}, f on {f.device}")
    return B, T, K, hop, sample_rate


def _in_kernel_range(x: torch.Tensor, B: int, T: int, K: int, hop: int, win_length) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and K <= KERNEL_MAX_PARTIALS and hop <= KERNEL_MAX_HOP
            and T * hop <= KERNEL_MAX_SAMPLES and B * T * max(K, hop) <= KERNEL_MAX_CELLS
            and (win_length is None or win_length <= KERNEL_MAX_WINDOW))


def _usable(f: torch.Tensor) -> torch.Tensor:
    return torch.isfinite(f) & (f > 0)


def _clean(f: torch.Tensor) -> torch.Tensor:
    return torch.where(_usable(f), f, torch.zeros((), dtype=f.dtype, device=f.device))


def _prepare(audio, f, voiced):
    audio = audio.detach()
    if audio.dtype not in (torch.float32, torch.float64):        # integers and 16-bit floats: analysed in fp32
        audio = audio.float()
    return audio.contiguous(), f.detach().to(audio.dtype).contiguous(), None if voiced is None else voiced.detach()


def _interior(T: int, hop: int, W: int):
    """(t_lo, t_hi): the frames whose window lies inside the clip (t_lo > t_hi: none)."""
    lead, N = (W - hop) // 2, T * hop
    t_lo = -(-lead // hop) if lead > 0 else 0
    room = N - W + lead
    return t_lo, (-1 if room < 0 else min(room // hop, T - 1))


# ------------------------------------------------------------------------------------------------------------ torch-op path

class _Tracks:
    """The closed form of section 5d in fp64: g, d and Phi (modulo 1) per segment, and the phase at any samples."""

    def __init__(self, f: torch.Tensor, hop: int, sample_rate: int):
        self.T, self.hop, self.head, self.e = f.shape[1], hop, hop // 2, 1 - hop % 2
        g = _clean(f).double() / sample_rate
        d = torch.cat([g[:, 1:] - g[:, :-1], torch.zeros_like(g[:, :1])], dim=1)
        tot = hop * (g + d * ((hop - 1 + self.e) / (2.0 * hop)))
        phi = self.head * g[:, :1] + torch.cumsum(tot, dim=1) - tot               # exclusive
        self.g, self.d, self.phi = g, d, phi % 1.0

    def turns(self, n: torch.Tensor) -> torch.Tensor:
        """n int64 [L] (inside [0, T hop)) -> P mod 1 as fp64 [B, L, K]."""
        m = n - self.head
        s = torch.div(m, self.hop, rounding_mode='floor').clamp(0, self.T - 1)
        j = (m - s * self.hop).double()[None, :, None]
        P = self.phi[:, s] + (j + 1.0) * (self.g[:, s] + self.d[:, s] * ((j + self.e) / (2.0 * self.hop)))
        head = (n.double() + 1.0)[None, :, None] * self.g[:, :1]
        return torch.where((m < 0)[None, :, None], head, P) % 1.0


def _keep_mask(f: torch.Tensor, voiced, sample_rate: int) -> torch.Tensor:
    """[B, T, K] True where C is kept: a usable entry, not above the bank's Nyquist mask, a voiced frame."""
    keep = _usable(f) & ~(f > sample_rate // 2)
    if voiced is not None:
        keep = keep & voiced.bool()
    return keep


def _analysis_torch(audio, f, voiced, hop, sample_rate, W, reassign):
    dt, dev = audio.dtype, audio.device
    B, N = audio.shape
    T, K = f.shape[1:]
    tracks = _Tracks(f, hop, sample_rate)
    j = torch.arange(W, device=dev)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * j.double() / W)
    wd = (math.pi / W) * torch.sin(2 * math.pi * j.double() / W)
    lead = (W - hop) // 2
    t_lo, t_hi = _interior(T, hop, W)
    keep = _keep_mask(f, voiced, sample_rate)
    cdt = torch.complex128 if dt == torch.float64 else torch.complex64
    C = torch.zeros((B, T, K), dtype=cdt, device=dev)
    f_re = f.clone() if reassign else None
    step = max(1, _CHUNK_ELEMENTS // max(1, B * W * K))
    zero = torch.zeros((), dtype=dt, device=dev)
    zero64 = torch.zeros((), dtype=torch.float64, device=dev)
    for t0 in range(0, T, step):
        t = torch.arange(t0, min(T, t0 + step), device=dev)
        Tc = len(t)
        idx = (t * hop - lead)[:, None] + j[None, :]                              # [Tc, W]
        inside = (idx >= 0) & (idx < N)
        at = idx.clamp(0, N - 1)
        wj = torch.where(inside, w[None, :], zero64)
        norm = wj.sum(-1)                                                         # fp64 [Tc]
        x = audio[:, at]
        wx = torch.where(inside[None], wj.to(dt)[None] * x, zero)                 # [B, Tc, W]
        ang = (2 * math.pi * tracks.turns(at.reshape(-1))).to(dt).reshape(B, Tc, W, K)
        cos, sin = torch.cos(ang), torch.sin(ang)
        re = torch.einsum('btw,btwk->btk', wx, cos)
        im = -torch.einsum('btw,btwk->btk', wx, sin)
        scale = (2.0 / norm).to(dt)[None, :, None]
        C[:, t0:t0 + Tc] = torch.complex(re * scale, im * scale)
        if reassign and t_lo <= t_hi:
            wdx = torch.where(inside[None], wd.to(dt)[None] * x, zero)
            dr = torch.einsum('btw,btwk->btk', wdx, cos)
            di = -torch.einsum('btw,btwk->btk', wdx, sin)
            num, den = di * re - dr * im, re * re + im * im
            mean = ((w[None, :, None] * _up(_clean(f).double(), at.reshape(-1), hop).reshape(B, Tc, W, K)).sum(2) / w.sum()).to(dt)
            value = mean - (sample_rate / (2 * math.pi)) * num / den
            ok = (keep[:, t0:t0 + Tc] & ((t >= t_lo) & (t <= t_hi))[None, :, None] & (den != 0) & torch.isfinite(value))
            f_re[:, t0:t0 + Tc] = torch.where(ok, value, f[:, t0:t0 + Tc])
    C = torch.where(keep, C, torch.zeros((), dtype=cdt, device=dev))
    amp = C.abs()
    a = amp.sum(-1, keepdim=True)
    c = torch.where(a == 0, torch.full((), 1.0 / K, dtype=dt, device=dev), amp / a)
    return C, a, c, f_re


def _resynth_torch(C, f, hop, sample_rate):
    B, T, K = C.shape
    dt = C.real.dtype
    tracks = _Tracks(f, hop, sample_rate)
    parts = torch.view_as_real(C).reshape(B, T, 2 * K)                            # re, im interleaved per partial
    harm = torch.empty((B, T * hop), dtype=dt, device=C.device)
    step = max(1, _CHUNK_ELEMENTS // max(1, B * K))
    for n0 in range(0, T * hop, step):
        n = torch.arange(n0, min(T * hop, n0 + step), device=C.device)
        ang = (2 * math.pi * tracks.turns(n)).to(dt)                              # [B, Nc, K]
        cu = _up(parts, n, hop).reshape(B, -1, K, 2)
        harm[:, n0:n0 + step] = (cu[..., 0] * torch.cos(ang) - cu[..., 1] * torch.sin(ang)).sum(-1)
    return harm


# -------------------------------------------------------------------------------------------------------------- device path

def _workspace(B, T, K, hop, W, device):
    return torch.empty(_lib.lib().ddsp_partials_workspace_bytes(B, T, K, hop, W), device=device, dtype=torch.uint8)


def _analysis_device(audio, f, voiced, hop, sample_rate, W, reassign, workspace):
    B, T, K = f.shape
    C = torch.empty((B, T, K, 2), device=audio.device, dtype=torch.float32)
    a = torch.empty((B, T, 1), device=audio.device, dtype=torch.float32)
    c = torch.empty((B, T, K), device=audio.device, dtype=torch.float32)
    f_re = torch.empty_like(c) if reassign else None
    v = None if voiced is None else voiced.bool().to(torch.uint8).contiguous()
    with torch.cuda.device(audio.device):
        rc = _lib.lib().ddsp_partials_analysis(audio.data_ptr(), f.data_ptr(), None if v is None else v.data_ptr(), C.data_ptr(),
                                               a.data_ptr(), c.data_ptr(), None if f_re is None else f_re.data_ptr(),
                                               workspace.data_ptr(), B, T, K, hop, W, sample_rate,
                                               torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_partials_analysis")
    return torch.view_as_complex(C), a, c, f_re


def _resynth_device(C, f, audio, hop, sample_rate, workspace, phase_ready):
    B, T, K = C.shape
    Cr = torch.view_as_real(C).contiguous()
    harm = torch.empty((B, T * hop), device=C.device, dtype=torch.float32)
    resid = None if audio is None else torch.empty_like(harm)
    with torch.cuda.device(C.device):
        rc = _lib.lib().ddsp_partials_resynth(Cr.data_ptr(), f.data_ptr(), None if audio is None else audio.data_ptr(), harm.data_ptr(),
                                              None if resid is None else resid.data_ptr(), workspace.data_ptr(), B, T, K, hop,
                                              sample_rate, PHASE_READY if phase_ready else 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_partials_resynth")
    return harm, resid


# ------------------------------------------------------------------------------------------------------------------- public

def _analysis(audio, f, voiced, hop, sample_rate, W, reassign, workspace=None):
    """Prepared tensors, B > 0 -> (C, a, c, f_re or None, the workspace the kernels filled or None)."""
    B, T, K = f.shape
    if _in_kernel_range(audio, B, T, K, hop, W):
        ws = _workspace(B, T, K, hop, W, audio.device) if workspace is None else workspace
        return _analysis_device(audio, f, voiced, hop, sample_rate, W, reassign, ws) + (ws,)
    return _analysis_torch(audio, f, voiced, hop, sample_rate, W, reassign) + (None,)


def _controls(f, a, c, C, f_re, return_complex):
    out = dict(f=_clean(f), a=a, c=c)
    if return_complex:
        out['C'] = C
    if f_re is not None:
        out['f_re'] = f_re
    return out


def _empty(f, dt, reassign):
    B, T, K = f.shape
    C = torch.zeros((0, T, K), dtype=torch.complex128 if dt == torch.float64 else torch.complex64, device=f.device)
    return C, torch.zeros((0, T, 1), dtype=dt, device=f.device), torch.zeros((0, T, K), dtype=dt, device=f.device), (f.clone() if reassign else None)


def partial_analysis(audio, f, hop, sample_rate, win_length, voiced=None, return_complex=False, reassign=False):
    """-> dict(f [B, T, K], a [B, T, 1], c [B, T, K]) as `InharmonicBank` reads a and c, plus C (complex [B, T, K]) when asked and,
    with `reassign`, f_re [B, T, K]: every partial's reassigned frequency on the frames whose window lies inside the clip (f where
    it is not defined)."""
    B, T, K, hop, sample_rate = _check(audio, f, hop, sample_rate, win_length, voiced, "partial_analysis")
    audio, f, voiced = _prepare(audio, f, voiced)
    if B == 0:
        C, a, c, f_re = _empty(f, audio.dtype, reassign)
        return _controls(f, a, c, C, f_re, return_complex)
    C, a, c, f_re, _ = _analysis(audio, f, voiced, hop, sample_rate, int(win_length), bool(reassign))
    return _controls(f, a, c, C, f_re, return_complex)


def partial_residual(audio, f, hop, sample_rate, win_length, voiced=None, return_complex=False, reassign=False):
    """-> (harm [B, N], resid = audio - harm, the dict of partial_analysis): the part of `audio` the partials along `f` explain,
    phases kept, and what is left.  The prefix over the tracks runs once for the analysis and the resynthesis."""
    B, T, K, hop, sample_rate = _check(audio, f, hop, sample_rate, win_length, voiced, "partial_residual")
    audio, f, voiced = _prepare(audio, f, voiced)
    if B == 0:
        C, a, c, f_re = _empty(f, audio.dtype, reassign)
        return torch.zeros_like(audio), torch.zeros_like(audio), _controls(f, a, c, C, f_re, return_complex)
    C, a, c, f_re, ws = _analysis(audio, f, voiced, hop, sample_rate, int(win_length), bool(reassign))
    if ws is not None:
        harm, resid = _resynth_device(C, f, audio, hop, sample_rate, ws, True)
    else:
        harm = _resynth_torch(C, f, hop, sample_rate)
        resid = audio - harm
    return harm, resid, _controls(f, a, c, C, f_re, return_complex)


def partial_resynthesis(C, f, hop, sample_rate):
    """C complex [B, T, K] (as partial_analysis returns it, or any other) along `f` [B, T, K] -> harm [B, T hop]."""
    if C.dim() != 3 or C.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"partial_resynthesis: C must be complex64 or complex128 [B, T, K], got {C.dtype} {tuple(C.shape)}")
    B, T, K, hop, sample_rate = _check(None, f, hop, sample_rate, None, None, "partial_resynthesis")
    if tuple(C.shape) != (B, T, K) or C.device != f.device:
        raise ValueError(f"partial_resynthesis: C {tuple(C.shape)} on {C.device} does not match f {tuple(f.shape)} on {f.device}")
    _refuse_grad(C, "partial_resynthesis")
    C = C.detach().contiguous()
    f = f.detach().to(C.real.dtype).contiguous()
    if B == 0:
        return torch.zeros((0, T * hop), dtype=C.real.dtype, device=C.device)
    if _in_kernel_range(C.real, B, T, K, hop, None):
        return _resynth_device(C, f, None, hop, sample_rate, _workspace(B, T, K, hop, 2, C.device), False)[0]
    return _resynth_torch(C, f, hop, sample_rate)


def _check_steps(iterations, max_cents, what):
    iterations, max_cents = int(iterations), float(max_cents)
    if iterations < 0:
        raise ValueError(f"{what}: the number of steps must be at least 0, got {iterations}")
    if not 0 < max_cents < math.inf:
        raise ValueError(f"{what}: max_cents must be positive and finite, got {max_cents}")
    return iterations, max_cents


def _carry_and_clamp(f, f_re, anchor, voiced, hop, W, max_cents):
    """Frame-rate arithmetic behind one reassignment (no host synchronisation): interior frames take f_re, frames whose window
    overhangs the clip the ratio f_re / f of the nearest interior frame of the same partial; every entry is clamped within
    `max_cents` of `anchor`; dead entries (not finite, not positive, unvoiced) come back as they are."""
    T = f.shape[1]
    alive = _usable(f)
    if voiced is not None:
        alive = alive & voiced.bool()
    t_lo, t_hi = _interior(T, hop, W)
    if t_lo > t_hi:
        return f.clone()
    one = torch.ones((), dtype=f.dtype, device=f.device)
    ratio = torch.where(alive, f_re / torch.where(alive, f, one), one)
    moved = f_re.clone()
    moved[:, :t_lo] = f[:, :t_lo] * ratio[:, t_lo:t_lo + 1]
    moved[:, t_hi + 1:] = f[:, t_hi + 1:] * ratio[:, t_hi:t_hi + 1]
    clamped = torch.minimum(torch.maximum(moved, anchor * 2.0 ** (-max_cents / 1200.0)), anchor * 2.0 ** (max_cents / 1200.0))
    return torch.where(alive & torch.isfinite(clamped), clamped, f)


def refine_partials(audio, f, hop, sample_rate, win_length, voiced=None, iterations=2, max_cents=50.0):
    """-> f [B, T, K] after `iterations` reassignment steps (each one analysis launch and frame-rate torch arithmetic), every entry
    within `max_cents` of the track given; dead entries come back as they are."""
    B, T, K, hop, sample_rate = _check(audio, f, hop, sample_rate, win_length, voiced, "refine_partials")
    iterations, max_cents = _check_steps(iterations, max_cents, "refine_partials")
    audio, f, voiced = _prepare(audio, f, voiced)
    if B == 0 or iterations == 0:
        return f.clone()
    W, track, ws = int(win_length), f, None
    for _ in range(iterations):
        _, _, _, f_re, ws = _analysis(audio, track, voiced, hop, sample_rate, W, True, ws)
        track = _carry_and_clamp(track, f_re, f, voiced, hop, W, max_cents)
    return track


def _base_ratios(base_ratios, K, device):
    if base_ratios is None:
        return torch.arange(1, K + 1, dtype=torch.float64, device=device)
    r = torch.as_tensor(base_ratios).detach().double().reshape(-1)
    # (values on a device are not read back: the check would synchronise, which a graph capture does not allow)
    if r.numel() != K or (not r.is_cuda and not bool((torch.isfinite(r) & (r > 0)).all())):
        raise ValueError(f"base_ratios must be {K} finite, positive numbers")
    return r.to(device)


def _stretched(r: torch.Tensor, B_coef: torch.Tensor) -> torch.Tensor:
    """r [K], B_coef [B] (fp64) -> rho [B, K] = r sqrt(1 + B r^2)."""
    return r[None, :] * torch.sqrt(1.0 + B_coef[:, None] * (r * r)[None, :])


def _fit(f, weight, r, f0):
    """fit_inharmonicity on checked tensors: f, weight [B, T, K] (any float dtype), r fp64 [K], f0 [B, T, 1] or None -> fp64."""
    f64, w = f.double(), weight.double()
    ok = _usable(f64) & torch.isfinite(w) & (w > 0)
    zero = torch.zeros((), dtype=torch.float64, device=f.device)
    w, f64 = torch.where(ok, w, zero), torch.where(ok, f64, zero)
    x = (r * r)[None, None, :]
    y = (f64 / r) ** 2
    sw = w.sum(-1, keepdim=True)
    safe = torch.where(sw > 0, sw, torch.ones_like(sw))
    xm, ym = (w * x).sum(-1, keepdim=True) / safe, (w * y).sum(-1, keepdim=True) / safe
    sxx = (w * (x - xm) ** 2).sum(-1, keepdim=True)
    sxy = (w * (x - xm) * (y - ym)).sum(-1, keepdim=True)
    beta = sxy / torch.where(sxx > 0, sxx, torch.ones_like(sxx))
    alpha = ym - beta * xm
    valid = (sw > 0) & (sxx > 0) & (alpha > 0)
    B_t = torch.where(valid, beta / torch.where(valid, alpha, torch.ones_like(alpha)), zero)
    omega = torch.where(valid, sxx, zero)
    total = omega.sum(1)[:, 0]
    # (clamped at 0; the upper end, far above any string, only keeps the tracks of a row of noise finite)
    B_coef = ((omega * B_t).sum(1)[:, 0] / torch.where(total > 0, total, torch.ones_like(total))).clamp(0.0, MAX_INHARMONICITY)
    rho = _stretched(r, B_coef)[:, None, :]
    den = (w * rho * rho).sum(-1, keepdim=True)
    fitted = (w * rho * f64).sum(-1, keepdim=True) / torch.where(den > 0, den, torch.ones_like(den))
    given = torch.zeros_like(fitted) if f0 is None else f0.double()
    return torch.where(den > 0, fitted, given), B_coef


def fit_inharmonicity(f, weight, base_ratios=None, f0=None):
    """f, weight [B, T, K] -> (f0 [B, T, 1], B_coef [B]) in fp64: the closed-form fit of f_k = f0 r_k sqrt(1 + B r_k^2).  With
    x_k = r_k^2 and y_tk = (f_tk / r_k)^2 the model is the line y = f0^2 + f0^2 B x: per frame the weighted least-squares line
    y = alpha_t + beta_t x gives B_t = beta_t / alpha_t; the row's B is the mean of B_t over the frames with alpha_t > 0, weighted
    by omega_t = sum_k weight (x - xbar_t)^2, clamped at 0; the frame's f0 is then the weighted least-squares scale of
    rho_k = r_k sqrt(1 + B r_k^2) onto f.  Callers pass |C|^2 as the weight.  Entries of f that are not finite or <= 0 carry no
    weight; a frame without weight keeps the `f0` given (0 without one)."""
    if f.dim() != 3 or tuple(weight.shape) != tuple(f.shape) or weight.device != f.device:
        raise ValueError(f"fit_inharmonicity: f and weight must be [B, T, K] on one device, got {tuple(f.shape)} and {tuple(weight.shape)}")
    if f0 is not None and (tuple(f0.shape) != tuple(f.shape[:2]) + (1,) or f0.device != f.device):
        raise ValueError(f"fit_inharmonicity: f0 must be {tuple(f.shape[:2]) + (1,)} on f's device, got {tuple(f0.shape)}")
    return _fit(f.detach(), weight.detach(), _base_ratios(base_ratios, f.shape[-1], f.device), None if f0 is None else f0.detach())


def _bank_frequencies(f0: torch.Tensor, ratios: torch.Tensor) -> torch.Tensor:
    """f0 [B, T, 1] times ratios [B, T, K] in fp32, as InharmonicBank.frequencies forms it."""
    return f0.float() * ratios.float()


def inharmonic_analysis(audio, f0, hop, sample_rate, n_partials, win_length, voiced=None, inharmonicity=0.0, base_ratios=None,
                        iterations=4, max_cents=50.0, model='stiff', return_complex=False):
    """-> dict(f0 [B, T, 1], ratios [B, T, K], a [B, T, 1], c [B, T, K], inharmonicity [B][, C]) as `InharmonicBank` reads it.
    From the pitch track `f0` and the stiffness `inharmonicity` (a float or [B]), `iterations` times: f = f0 rho(B), an analysis
    with reassignment along f, every measured entry clamped within `max_cents` of f, and `fit_inharmonicity` of the measured
    tracks weighted by |C|^2 (the frames whose window overhangs the clip carry no weight; their f0 moves by the ratio of the
    nearest frame that was measured); then a plain analysis along f0 * ratios, formed in fp32 as the bank forms it, so the bank on the
    dict runs the phases the amplitudes were measured along.  model='stiff': ratios = rho(B), the same in every frame;
    model='free': ratios = (the last measured tracks) / f0, each partial on its own track."""
    what = "inharmonic_analysis"
    if model not in MODELS:
        raise ValueError(f"{what}: model must be one of {MODELS}, got {model!r}")
    if f0.dim() != 3 or f0.shape[-1] != 1:
        raise ValueError(f"{what}: f0 must be [B, T, 1], got {tuple(f0.shape)}")
    K = int(n_partials)
    if K < 1:
        raise ValueError(f"{what}: n_partials must be positive, got {n_partials}")
    iterations, max_cents = _check_steps(iterations, max_cents, what)
    B, T, _, hop, sample_rate = _check(audio, f0, hop, sample_rate, win_length, voiced, what)
    W = int(win_length)
    audio, f0, voiced = _prepare(audio, f0, voiced)
    dt, dev = audio.dtype, audio.device
    r = _base_ratios(base_ratios, K, dev)
    if torch.is_tensor(inharmonicity):
        B_coef = inharmonicity.detach().to(device=dev, dtype=torch.float64).reshape(-1).expand(B).clamp(min=0)
    else:
        B_coef = torch.full((B,), max(float(inharmonicity), 0.0), dtype=torch.float64, device=dev)
    track0 = _clean(f0).double()
    measured, ws = None, None
    t_lo, t_hi = _interior(T, hop, W)
    if B > 0 and t_lo <= t_hi:
        inside = torch.zeros((1, T, 1), dtype=torch.bool, device=dev)
        inside[:, t_lo:t_hi + 1] = True
        for _ in range(iterations):
            f = (track0 * _stretched(r, B_coef)[:, None, :]).to(dt)
            C, _, _, f_re, ws = _analysis(audio, f, voiced, hop, sample_rate, W, True, ws)
            measured = _carry_and_clamp(f, f_re, f, voiced, hop, W, max_cents)
            # the fit reads the frames that were measured; a frame whose window overhangs the clip follows the nearest of them
            weight = torch.where(inside, C.real * C.real + C.imag * C.imag, torch.zeros((), dtype=dt, device=dev))
            fitted, B_coef = _fit(measured, weight, r, track0)
            moved = torch.where(track0 > 0, fitted / torch.where(track0 > 0, track0, torch.ones_like(track0)), torch.ones_like(track0))
            fitted[:, :t_lo] = track0[:, :t_lo] * moved[:, t_lo:t_lo + 1]
            fitted[:, t_hi + 1:] = track0[:, t_hi + 1:] * moved[:, t_hi:t_hi + 1]
            track0 = fitted
    f0_out = track0.float()
    rho = _stretched(r, B_coef).float()[:, None, :].expand(B, T, K)
    if model == 'free' and measured is not None:
        alive = (f0_out > 0) & _usable(measured)
        ratios = torch.where(alive, measured.float() / torch.where(f0_out > 0, f0_out, torch.ones_like(f0_out)), rho)
    else:
        ratios = rho
    ratios = ratios.contiguous()
    f = _bank_frequencies(f0_out, ratios).to(dt).contiguous()
    if B == 0:
        C, a, c, _ = _empty(f, dt, False)
    else:
        C, a, c, _, _ = _analysis(audio, f, voiced, hop, sample_rate, W, False, ws)
    out = dict(f0=f0_out.to(dt), ratios=ratios.to(dt), a=a, c=c, inharmonicity=B_coef.to(dt))
    if return_complex:
        out['C'] = C
    return out


class PartialAnalyzer(nn.Module):
    """forward(audio [B, T hop], f0 [B, T, 1], voiced=None) -> dict(f0, ratios, a, c, inharmonicity): `inharmonic_analysis` at the
    configuration's n_harmonics (the partials), sample_rate, hop_length and n_fft (the window).  No parameters."""

    def __init__(self, conf, iterations=4, model='stiff', inharmonicity=0.0, base_ratios=None, max_cents=50.0):
        super().__init__()
        if model not in MODELS:
            raise ValueError(f"PartialAnalyzer: model must be one of {MODELS}, got {model!r}")
        self.iterations, self.max_cents = _check_steps(iterations, max_cents, "PartialAnalyzer")
        self.model = model
        self.inharmonicity = float(inharmonicity)
        self.base_ratios = None if base_ratios is None else torch.as_tensor(base_ratios, dtype=torch.float64).reshape(-1).clone()
        self.n_partials = conf.n_harmonics if self.base_ratios is None else self.base_ratios.numel()
        self.sample_rate = conf.sample_rate
        self.hop_length = conf.hop_length
        self.win_length = conf.n_fft

    def forward(self, audio, f0, voiced=None):
        return inharmonic_analysis(audio, f0, self.hop_length, self.sample_rate, self.n_partials, self.win_length, voiced=voiced,
                                   inharmonicity=self.inharmonicity, base_ratios=self.base_ratios, iterations=self.iterations,
                                   max_cents=self.max_cents, model=self.model)
