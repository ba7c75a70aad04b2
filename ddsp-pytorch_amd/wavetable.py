"""Differentiable wavetable synthesis on the HIP kernels (include/ddsp_hip.h: ddsp_wavetable_*).

`WavetableBank` is the second tonal synthesiser beside `OscillatorBank`: N learnable single-cycle tables of L points, one phase
accumulator per batch row reading them at f0 with linear interpolation, mixed per frame by the controller's weights.  It reads the
control dict the bank reads -- `x['f0'] [B,T,1]`, `x['c'] [B,T,N]`, `x['a'] [B,T,1]` -- so a `Decoder(conf, synth='wavetable')` runs
with the same controller, noise, reverb, loss and trainer.

  wavetable_forward(f0, c, a, tables, hop, sample_rate, phase=None) -> y [B, T hop]
  wavetable_backward(grad_y, f0, c, a, tables, hop, sample_rate, phase=None) -> (grad_c, grad_a, grad_tables)
  wavetable_form(B, T, N, L, hop) -> dict(forward='lds' | 'global', backward=...)      the planner's answer

Known limit: the tables are not band-limited (no mip-maps).  A table with content above sample_rate / (2 f0) aliases, as in the
published method.
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
    def __init__(self, conf, n_wavetables=None, table_size=None, init='harmonic'):
        super().__init__()
        if n_wavetables is None:
            n_wavetables = getattr(conf, 'n_wavetables', None) or conf.n_harmonics
        if table_size is None:
            table_size = getattr(conf, 'wavetable_size', None) or 512
        self.n_wavetables, self.table_size = int(n_wavetables), int(table_size)
        self.sample_rate = conf.sample_rate
        self.hop_size = conf.hop_length
        if self.n_wavetables < 1 or self.table_size < 2:
            raise ValueError(f"WavetableBank needs n_wavetables >= 1 and table_size >= 2, got {n_wavetables} and {table_size}")
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

    def forward(self, x):
        f0, c, a = x['f0'], x['c'], x['a']
        _check_inputs(f0, c, a)
        if torch.is_grad_enabled() and (c.requires_grad or a.requires_grad or self.wavetables.requires_grad):
            _check_tables(c, self.wavetables)
            return _WavetableFunction.apply(f0, c, a, self.wavetables, self.hop_size, self.sample_rate)
        return wavetable_forward(f0, c, a, self.wavetables, self.hop_size, self.sample_rate)

    def live(self, x):
        f0, c, a = x['f0'], x['c'], x['a']
        _check_inputs(f0, c, a)
        B = c.shape[0]
        if self.phase.shape[0] != B or self.phase.device != c.device:
            self.phase = torch.zeros(B, dtype=torch.float64, device=c.device)
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
