"""Differentiable wavetable synthesis on the HIP kernels (include/ddsp_hip.h: ddsp_wavetable_*).

`WavetableBank` is the second tonal synthesiser beside `OscillatorBank`: N learnable single-cycle tables of L points, one phase
accumulator per batch row reading them at f0 with linear interpolation, mixed per frame by the controller's weights.  It reads the
control dict the bank reads -- `x['f0'] [B,T,1]`, `x['c'] [B,T,N]`, `x['a'] [B,T,1]` -- so a `Decoder(conf, synth='wavetable')` runs
with the same controller, noise, reverb, loss and trainer.

  wavetable_forward(f0, c, a, tables, hop, sample_rate, phase=None) -> y [B, T hop]
  wavetable_backward(grad_y, f0, c, a, tables, hop, sample_rate, phase=None) -> (grad_c, grad_a, grad_tables)
  wavetable_form(B, T, N, L, hop) -> dict(forward='lds' | 'global', backward=...)      the planner's answer

Band-limited tables, opt-in with `WavetableBank(conf, band_limited=True)` or `conf.wavetable_band_limited`:
every sample reads two mip levels of the tables, chosen from its increment, so that no harmonic above sample_rate / 2 is played.

  dirichlet_kernels(L, device) -> D [Q+1, L]            the levels' kernels, fp64 on the host, cached per (L, device)
  wavetable_mipmaps(tables) -> M [Q+1, N, L]            differentiable: the backward is the adjoint launch
  wavetable_forward_bl(f0, c, a, levels, hop, sample_rate, phase=None) -> y
  wavetable_backward_bl(grad_y, f0, c, a, levels, hop, sample_rate, phase=None) -> (grad_c, grad_a, grad_levels)

Without the switch the tables are played as given: a table with content above sample_rate / (2 f0) aliases, as in the published
method.  With it, inside an octave the top band fades out linearly (up to one octave of brightness is given away), and the images
that linear interpolation itself creates are not addressed.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib
from .harmonic_oscillator import _dev_ptr

FORMS = {1: "lds", 2: "global"}


def wavetable_form(B: int, T: int, N: int, L: int, hop: int) -> dict:
    """Which kernel form ddsp_wavetable_forward / _backward take for the shape (under the current test hooks)."""
    rc = _lib.lib().ddsp_wavetable_form(B, T, N, L, hop)
    _lib.check(rc if rc < 0 else 0, "ddsp_wavetable_form")
    return dict(forward=FORMS[rc & 3], backward=FORMS[(rc >> 2) & 3])


def wavetable_form_bl(B: int, T: int, N: int, L: int, hop: int) -> dict:
    """The band-limited plan for the shape (under the current test hooks): 'lds' -- a unit stages the levels it hears when at most
    `*_fit` of them are needed -- or 'global' for the forward and the backward."""
    rc = _lib.lib().ddsp_wavetable_form_bl(B, T, N, L, hop)
    _lib.check(rc if rc < 0 else 0, "ddsp_wavetable_form_bl")
    return dict(forward=FORMS[rc & 3], backward=FORMS[(rc >> 2) & 3], forward_fit=(rc >> 8) & 0xff, backward_fit=(rc >> 16) & 0xff)


def _check_inputs(f0, c, a):
    if f0.dim() != 3 or c.dim() != 3 or a.dim() != 3 or f0.shape[-1] != 1 or a.shape[-1] != 1:
        raise ValueError("expected f0 [B,T,1], c [B,T,N], a [B,T,1]")
    if f0.shape[:2] != c.shape[:2] or a.shape[:2] != c.shape[:2]:
        raise ValueError(f"batch/frame mismatch: f0 {tuple(f0.shape)}, c {tuple(c.shape)}, a {tuple(a.shape)}")
    if not c.is_cuda:
        raise _lib.DdspHipError("WavetableBank runs on the GPU only (no CPU fallback): move the controls to cuda")
    if f0.device != c.device or a.device != c.device:
        raise _lib.DdspHipError(f"wavetable: f0 ({f0.device}), c ({c.device}) and a ({a.device}) must be on one device")


def _check_tables(c, tables):
    if tables.device != c.device:
        raise _lib.DdspHipError(f"wavetable: the tables are on {tables.device}, the controls on {c.device}: move the module or the "
                                "controls (nothing is copied between devices behind the caller's back)")
    if tables.dim() != 2 or tables.shape[0] != c.shape[-1]:
        raise ValueError(f"expected tables [N, L] with N = c's last dimension, got tables {tuple(tables.shape)}, c {tuple(c.shape)}")
    if not _lib.lib().ddsp_wavetable_supported(tables.shape[0], tables.shape[1]):
        raise _lib.DdspHipError(f"wavetable: {tables.shape[0]} tables of {tables.shape[1]} points are outside the kernels' range "
                                "(DDSP_ERANGE): N <= 1024, 2 <= L <= 65536, N L <= 2^18")


def wavetable_forward(f0, c, a, tables, hop: int, sample_rate: int, phase=None):
    """Raw launcher of ddsp_wavetable_forward -> y [B, T hop].  `phase` [B] fp64 on the device: the start phases (cycles), replaced
    IN PLACE by the phase after the block."""
    _check_inputs(f0, c, a)
    _check_tables(c, tables)
    f0 = f0.detach().contiguous().float()
    c = c.detach().contiguous().float()
    a = a.detach().contiguous().float()
    tables = tables.detach().contiguous().float()
    B, T, N = c.shape
    y = torch.empty((B, T * hop), device=c.device, dtype=torch.float32)
    if B == 0:
        return y
    if phase is not None and (phase.dtype != torch.float64 or phase.shape != (B,) or phase.device != c.device or not phase.is_contiguous()):
        raise ValueError(f"phase must be a contiguous fp64 tensor [{B}] on {c.device}")
    lib = _lib.lib()
    n = lib.ddsp_wavetable_scratch_bytes(B, T, N, tables.shape[1], hop)
    scratch = torch.empty(n, device=c.device, dtype=torch.uint8) if n else None
    with torch.cuda.device(c.device):
        rc = lib.ddsp_wavetable_forward(f0.data_ptr(), c.data_ptr(), a.data_ptr(), tables.data_ptr(), y.data_ptr(), _dev_ptr(scratch),
                                        _dev_ptr(phase), B, T, N, tables.shape[1], hop, sample_rate,
                                        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_wavetable_forward")
    return y


def wavetable_backward(grad_y, f0, c, a, tables, hop: int, sample_rate: int, phase=None):
    """Raw launcher of ddsp_wavetable_backward -> (grad_c [B,T,N], grad_a [B,T,1], grad_tables [N,L]).  `phase`: the start phases
    the forward was given (as they were BEFORE it ran), or None."""
    _check_inputs(f0, c, a)
    _check_tables(c, tables)
    f0 = f0.detach().contiguous().float()
    c = c.detach().contiguous().float()
    a = a.detach().contiguous().float()
    tables = tables.detach().contiguous().float()
    grad_y = grad_y.detach().contiguous().float()
    B, T, N = c.shape
    L = tables.shape[1]
    grad_c, grad_a, grad_t = torch.empty_like(c), torch.empty_like(a), torch.empty_like(tables)
    if B == 0:
        return grad_c, grad_a, grad_t.zero_()
    lib = _lib.lib()
    scratch = torch.empty(lib.ddsp_wavetable_backward_scratch_bytes(B, T, N, L, hop), device=c.device, dtype=torch.uint8)
    with torch.cuda.device(c.device):
        rc = lib.ddsp_wavetable_backward(grad_y.data_ptr(), f0.data_ptr(), c.data_ptr(), a.data_ptr(), tables.data_ptr(), _dev_ptr(phase),
                                         scratch.data_ptr(), grad_c.data_ptr(), grad_a.data_ptr(), grad_t.data_ptr(), B, T, N, L, hop,
                                         sample_rate, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_wavetable_backward")
    return grad_c, grad_a, grad_t


_KERNELS = {}


def mip_levels(L: int) -> int:
    """Q + 1 = log2 L + 1, or ValueError for a table size that cannot be band-limited"""
    L = int(L)
    if L < 16 or L > 4096 or L & (L - 1):
        raise ValueError(f"band-limited wavetables need a table size that is a power of two with 16 <= L <= 4096, got {L}")
    return L.bit_length()


def dirichlet_kernels(L: int, device="cpu") -> torch.Tensor:
    """D [Q+1, L] fp32 on `device`: D[q, j] = fl32((1 + 2 sum_{h=1..L>>(q+1)} cos(2 pi h j / L)) / L), computed in fp64 on the host;
    row 0 (level 0 is the table itself) is zero.  Cached per (L, device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(L), str(device))
    if key not in _KERNELS:
        n = mip_levels(L)
        j = torch.arange(L, dtype=torch.float64)
        D = torch.zeros(n, L, dtype=torch.float64)
        for q in range(1, n):
            h = torch.arange(1, (L >> (q + 1)) + 1, dtype=torch.float64)
            D[q] = (1.0 + 2.0 * torch.cos(2.0 * math.pi * h[:, None] * j[None, :] / L).sum(0)) / L
        _KERNELS[key] = D.float().to(device)
    return _KERNELS[key]


def _check_levels(c, levels):
    if levels.device != c.device:
        raise _lib.DdspHipError(f"wavetable: the levels are on {levels.device}, the controls on {c.device}")
    if levels.dim() != 3 or levels.shape[1] != c.shape[-1]:
        raise ValueError(f"expected levels [Q+1, N, L] with N = c's last dimension, got levels {tuple(levels.shape)}, c {tuple(c.shape)}")
    if levels.shape[0] != mip_levels(levels.shape[2]):
        raise ValueError(f"expected {mip_levels(levels.shape[2])} levels of {levels.shape[2]} points, got {levels.shape[0]}")


def _mip_build(tables):
    """tables [N, L] fp32 contiguous on the device -> M [Q+1, N, L] (one launch)"""
    N, L = tables.shape
    n = mip_levels(L)
    if not tables.is_cuda:
        raise _lib.DdspHipError("wavetable_mipmaps runs on the GPU only (no CPU fallback): move the tables to cuda")
    D = dirichlet_kernels(L, tables.device)
    M = torch.empty((n, N, L), device=tables.device, dtype=torch.float32)
    with torch.cuda.device(tables.device):
        rc = _lib.lib().ddsp_wavetable_mip_build(tables.data_ptr(), D.data_ptr(), M.data_ptr(), N, L, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_wavetable_mip_build")
    return M


class _MipFunction(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, tables):
        return _mip_build(tables.detach().contiguous().float())

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_levels):
        g = grad_levels.detach().contiguous().float()
        n, N, L = g.shape
        out = torch.empty((N, L), device=g.device, dtype=torch.float32)
        D = dirichlet_kernels(L, g.device)
        with torch.cuda.device(g.device):
            rc = _lib.lib().ddsp_wavetable_mip_adjoint(g.data_ptr(), D.data_ptr(), out.data_ptr(), N, L, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_wavetable_mip_adjoint")
        return out


def wavetable_mipmaps(tables):
    """tables [N, L] -> the mip levels M [Q+1, N, L] (M[0] is the tables bit for bit); differentiable with respect to the tables."""
    if tables.dim() != 2:
        raise ValueError(f"expected tables [N, L], got {tuple(tables.shape)}")
    mip_levels(tables.shape[1])
    return _MipFunction.apply(tables)


def wavetable_forward_bl(f0, c, a, levels, hop: int, sample_rate: int, phase=None):
    """Raw launcher of ddsp_wavetable_forward_bl -> y [B, T hop]; `phase` as in wavetable_forward."""
    _check_inputs(f0, c, a)
    _check_levels(c, levels)
    f0 = f0.detach().contiguous().float()
    c = c.detach().contiguous().float()
    a = a.detach().contiguous().float()
    levels = levels.detach().contiguous().float()
    B, T, N = c.shape
    y = torch.empty((B, T * hop), device=c.device, dtype=torch.float32)
    if B == 0:
        return y
    if phase is not None and (phase.dtype != torch.float64 or phase.shape != (B,) or phase.device != c.device or not phase.is_contiguous()):
        raise ValueError(f"phase must be a contiguous fp64 tensor [{B}] on {c.device}")
    with torch.cuda.device(c.device):
        rc = _lib.lib().ddsp_wavetable_forward_bl(f0.data_ptr(), c.data_ptr(), a.data_ptr(), levels.data_ptr(), y.data_ptr(), _dev_ptr(phase),
                                                  B, T, N, levels.shape[2], hop, sample_rate, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_wavetable_forward_bl")
    return y


def wavetable_backward_bl(grad_y, f0, c, a, levels, hop: int, sample_rate: int, phase=None):
    """Raw launcher of ddsp_wavetable_backward_bl -> (grad_c [B,T,N], grad_a [B,T,1], grad_levels [Q+1,N,L])."""
    _check_inputs(f0, c, a)
    _check_levels(c, levels)
    f0 = f0.detach().contiguous().float()
    c = c.detach().contiguous().float()
    a = a.detach().contiguous().float()
    levels = levels.detach().contiguous().float()
    grad_y = grad_y.detach().contiguous().float()
    B, T, N = c.shape
    L = levels.shape[2]
    grad_c, grad_a, grad_l = torch.empty_like(c), torch.empty_like(a), torch.empty_like(levels)
    if B == 0:
        return grad_c, grad_a, grad_l.zero_()
    lib = _lib.lib()
    scratch = torch.empty(lib.ddsp_wavetable_backward_bl_scratch_bytes(B, T, N, L, hop), device=c.device, dtype=torch.uint8)
    with torch.cuda.device(c.device):
        rc = lib.ddsp_wavetable_backward_bl(grad_y.data_ptr(), f0.data_ptr(), c.data_ptr(), a.data_ptr(), levels.data_ptr(), _dev_ptr(phase),
                                            scratch.data_ptr(), grad_c.data_ptr(), grad_a.data_ptr(), grad_l.data_ptr(), B, T, N, L, hop,
                                            sample_rate, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_wavetable_backward_bl")
    return grad_c, grad_a, grad_l


class _WavetableBlFunction(torch.autograd.Function):
    """The band-limited synthesis on given levels: differentiable w.r.t. c, a and the levels (wavetable_mipmaps carries that on to
    the tables)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, f0, c, a, levels, hop, sample_rate):
        f0 = f0.detach().contiguous().float()
        c = c.detach().contiguous().float()
        a = a.detach().contiguous().float()
        levels = levels.detach().contiguous().float()
        y = wavetable_forward_bl(f0, c, a, levels, hop, sample_rate)
        ctx.save_for_backward(f0, c, a, levels)
        ctx.hop, ctx.sample_rate = hop, sample_rate
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y):
        f0, c, a, levels = ctx.saved_tensors
        grad_c, grad_a, grad_l = wavetable_backward_bl(grad_y, f0, c, a, levels, ctx.hop, ctx.sample_rate)
        return None, grad_c, grad_a, grad_l, None, None


class _WavetableFunction(torch.autograd.Function):
    """Differentiable w.r.t. c, a and the tables; f0 carries no gradient, as in the oscillator bank."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, f0, c, a, tables, hop, sample_rate):
        f0 = f0.detach().contiguous().float()
        c = c.detach().contiguous().float()
        a = a.detach().contiguous().float()
        tables = tables.detach().contiguous().float()
        y = wavetable_forward(f0, c, a, tables, hop, sample_rate)
        ctx.save_for_backward(f0, c, a, tables)
        ctx.hop, ctx.sample_rate = hop, sample_rate
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y):
        f0, c, a, tables = ctx.saved_tensors
        grad_c, grad_a, grad_t = wavetable_backward(grad_y, f0, c, a, tables, ctx.hop, ctx.sample_rate)
        return None, grad_c, grad_a, grad_t, None, None


def harmonic_tables(n_wavetables: int, table_size: int) -> torch.Tensor:
    """W[k, j] = sin(2 pi (k + 1) j / L): table k is harmonic k + 1, so the module starts as the oscillator bank below Nyquist."""
    if 2 * n_wavetables >= table_size:
        raise ValueError(f"init='harmonic' needs 2 n_wavetables < table_size (harmonic N has to fit the table), got "
                         f"{n_wavetables} tables of {table_size} points")
    j = torch.arange(table_size, dtype=torch.float64)
    k = torch.arange(1, n_wavetables + 1, dtype=torch.float64)
    return torch.sin(2.0 * math.pi * k[:, None] * j[None, :] / table_size).float()


def resample_tables(tables: torch.Tensor, table_size: int) -> torch.Tensor:
    """[N, L'] -> [N, table_size]: each table read linearly on the circle at table_size evenly spaced phases (host code)."""
    t = tables.detach().to(device="cpu", dtype=torch.float64)
    Lp = t.shape[1]
    if Lp == table_size:
        return tables.detach().to(device="cpu", dtype=torch.float32).clone()
    pos = torch.arange(table_size, dtype=torch.float64) * (Lp / table_size)
    j = pos.floor().long().clamp_(max=Lp - 1)
    fr = pos - j
    return (t[:, j] + fr * (t[:, (j + 1) % Lp] - t[:, j])).float()


class WavetableBank(nn.Module):
    def __init__(self, conf, n_wavetables=None, table_size=None, init='harmonic', band_limited=None):
        super().__init__()
        if band_limited is None:
            band_limited = bool(getattr(conf, 'wavetable_band_limited', False))
        self.band_limited = bool(band_limited)
        if n_wavetables is None:
            n_wavetables = getattr(conf, 'n_wavetables', None) or conf.n_harmonics
        if table_size is None:
            table_size = getattr(conf, 'wavetable_size', None) or 512
        self.n_wavetables, self.table_size = int(n_wavetables), int(table_size)
        self.sample_rate = conf.sample_rate
        self.hop_size = conf.hop_length
        if self.n_wavetables < 1 or self.table_size < 2:
            raise ValueError(f"WavetableBank needs n_wavetables >= 1 and table_size >= 2, got {n_wavetables} and {table_size}")
        if self.band_limited:
            mip_levels(self.table_size)         # (ValueError for a size that cannot be band-limited)
        if torch.is_tensor(init):
            if tuple(init.shape) != (self.n_wavetables, self.table_size):
                raise ValueError(f"init must be [{self.n_wavetables}, {self.table_size}], got {tuple(init.shape)}")
            tables = init.detach().to(dtype=torch.float32).clone()
        elif init == 'harmonic':
            tables = harmonic_tables(self.n_wavetables, self.table_size)
        else:
            raise ValueError(f"init must be 'harmonic' or a tensor [N, L], got {init!r}")
        self.wavetables = nn.Parameter(tables)
        # the live stream's phase per batch row (cycles, fp64), updated in place by the kernel; not part of the state dict
        self.register_buffer("phase", torch.zeros(0, dtype=torch.float64), persistent=False)
        # band-limited, live() only: the levels of the tables as they were at `_levels_key` (the parameter's version and
        # storage), rebuilt when either changes or after invalidate_levels(); not a buffer, not part of the state dict
        self._levels, self._levels_key = None, None

    def levels(self) -> torch.Tensor:
        """The mip levels [Q+1, N, L] of the tables for the live path, without gradient: cached, and rebuilt (one launch) after the
        parameter was written to in a way autograd's version counter sees (an eager optimiser step, `load_tables`,
        `load_state_dict`), after it moved, and after `invalidate_levels()`.  A write the counter does not see -- the replay of
        a captured optimiser update -- needs `invalidate_levels()`; `GraphedTrainStep` calls it after every step.  `forward`
        does not use this cache: it builds the levels from the tables on every call."""
        w = self.wavetables
        key = (w._version, w.data_ptr(), str(w.device))
        if self._levels is None or self._levels_key != key:
            with torch.no_grad():
                self._levels = _mip_build(w.detach().contiguous().float())
            self._levels_key = key
        return self._levels

    def invalidate_levels(self) -> None:
        """Forget the cached mip levels: the next `live()` builds them from the tables as they are then."""
        self._levels, self._levels_key = None, None

    def _forward_bl(self, f0, c, a):
        _check_tables(c, self.wavetables)
        if torch.is_grad_enabled() and (c.requires_grad or a.requires_grad or self.wavetables.requires_grad):
            return _WavetableBlFunction.apply(f0, c, a, wavetable_mipmaps(self.wavetables), self.hop_size, self.sample_rate)
        # (no cache here: one 30 us launch, and nothing that rewrote the tables behind autograd's back can be missed)
        with torch.no_grad():
            levels = _mip_build(self.wavetables.detach().contiguous().float())
        return wavetable_forward_bl(f0, c, a, levels, self.hop_size, self.sample_rate)

    def forward(self, x):
        f0, c, a = x['f0'], x['c'], x['a']
        _check_inputs(f0, c, a)
        if self.band_limited:
            return self._forward_bl(f0, c, a)
        if torch.is_grad_enabled() and (c.requires_grad or a.requires_grad or self.wavetables.requires_grad):
            _check_tables(c, self.wavetables)
            return _WavetableFunction.apply(f0, c, a, self.wavetables, self.hop_size, self.sample_rate)
        return wavetable_forward(f0, c, a, self.wavetables, self.hop_size, self.sample_rate)

    def live(self, x):
        """One block of a stream: the phase per row is carried on the device.  Band-limited: the block is one launch on the
        cached levels (`levels()`).  The first band-limited call on a device copies the Dirichlet kernels to it and builds the
        levels, so call `live()` (or `levels()`) once before capturing it in a graph; a captured graph replays the levels it was
        captured with."""
        f0, c, a = x['f0'], x['c'], x['a']
        _check_inputs(f0, c, a)
        B = c.shape[0]
        if self.phase.shape[0] != B or self.phase.device != c.device:
            self.phase = torch.zeros(B, dtype=torch.float64, device=c.device)
        if self.band_limited:
            _check_tables(c, self.wavetables)
            return wavetable_forward_bl(f0, c, a, self.levels(), self.hop_size, self.sample_rate, phase=self.phase)
        return wavetable_forward(f0, c, a, self.wavetables, self.hop_size, self.sample_rate, phase=self.phase)

    def reset_phase(self):
        self.phase.zero_()

    def export_tables(self) -> torch.Tensor:
        """The learned tables [N, L] on the CPU: the timbre as a tensor to inspect, edit, store or give to another model."""
        return self.wavetables.detach().to(device="cpu", dtype=torch.float32).clone()

    def load_tables(self, tables: torch.Tensor) -> None:
        """Take tables [N, L'] (any L': resampled linearly on the circle to this module's L) as the new timbre."""
        if tables.dim() != 2 or tables.shape[0] != self.n_wavetables or tables.shape[1] < 2:
            raise ValueError(f"load_tables: expected [{self.n_wavetables}, L'], got {tuple(tables.shape)}")
        with torch.no_grad():
            self.wavetables.copy_(resample_tables(tables, self.table_size))


def is_wavetable(decoder) -> bool:
    return isinstance(getattr(decoder, 'harmonics', None), WavetableBank)


def refuse_wavetable(decoder_or_flag, what: str) -> None:
    """The one refusal of every entry point whose meaning rests on `c` being harmonic amplitudes or on the bank's `last_phases`."""
    flag = decoder_or_flag if isinstance(decoder_or_flag, bool) else is_wavetable(decoder_or_flag)
    if flag:
        raise ValueError(f"{what}: not available with the wavetable synthesiser (synth='wavetable'): it rests on the oscillator "
                         "bank's harmonic amplitudes or its carried phases; build the decoder with synth='harmonic'")
