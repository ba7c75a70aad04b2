"""Inharmonic partials on the HIP kernels (include/ddsp_hip.h: ddsp_sinusoids_*).

`InharmonicBank` is the third tonal synthesiser beside `OscillatorBank` and `WavetableBank`: K sinusoids per batch row, each with
its own frame-rate frequency track, so a partial need not sit on a multiple of f0 -- stiff strings (f_k = k f0 sqrt(1 + B k^2)),
bells and bars (mode ratios that are not integers), detuned partials that beat.  It reads the control dict the bank reads --
`x['f0'] [B,T,1]`, `x['c'] [B,T,K]`, `x['a'] [B,T,1]` -- so a `Decoder(conf, synth='inharmonic')` runs with the same controller,
noise, reverb, loss and trainer.  It is the one synthesiser here whose frequencies receive a gradient, which reaches the module's
`inharmonicity` and `detune_cents` through the torch operations that build the tracks.

  sinusoids_forward(f, c, a, hop, sample_rate, phase=None, normalize=True) -> y [B, T hop]
  sinusoids_backward(grad_y, f, c, a, hop, sample_rate, phase=None, normalize=True, want_grad_f=True) -> (grad_f | None, grad_c, grad_a)
  stretched_ratios(K, B_coef) -> k sqrt(1 + B k^2), k = 1 .. K
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .harmonic_oscillator import _dev_ptr


def _check_inputs(f, c, a):
    if f.dim() != 3 or c.dim() != 3 or a.dim() != 3 or a.shape[-1] != 1:
        raise ValueError("expected f [B,T,K], c [B,T,K], a [B,T,1]")
    if f.shape != c.shape or a.shape[:2] != c.shape[:2]:
        raise ValueError(f"shape mismatch: f {tuple(f.shape)}, c {tuple(c.shape)}, a {tuple(a.shape)}")
    if not c.is_cuda:
        raise _lib.DdspHipError("InharmonicBank runs on the GPU only (no CPU fallback): move the controls to cuda")
    if f.device != c.device or a.device != c.device:
        raise _lib.DdspHipError(f"sinusoids: f ({f.device}), c ({c.device}) and a ({a.device}) must be on one device")


def _check_range(K: int, hop: int):
    if not _lib.lib().ddsp_sinusoids_supported(K, hop):
        raise _lib.DdspHipError(f"sinusoids: {K} partials at hop {hop} are outside the kernels' range (DDSP_ERANGE): "
                                "1 <= K <= 1024, 1 <= hop <= 1024")


def _check_phase(phase, B, K, device):
    if phase is not None and (phase.dtype != torch.float64 or phase.shape != (B, K) or phase.device != device or not phase.is_contiguous()):
        raise ValueError(f"phase must be a contiguous fp64 tensor [{B}, {K}] on {device}")


def sinusoids_forward(f, c, a, hop: int, sample_rate: int, phase=None, normalize: bool = True):
    """Raw launcher of ddsp_sinusoids_forward -> y [B, T hop].  `phase` [B, K] fp64 on the device: the start phases (turns),
    replaced IN PLACE by the phases after the block."""
    _check_inputs(f, c, a)
    f = f.detach().contiguous().float()
    c = c.detach().contiguous().float()
    a = a.detach().contiguous().float()
    B, T, K = c.shape
    _check_range(K, hop)
    y = torch.empty((B, T * hop), device=c.device, dtype=torch.float32)
    if B == 0:
        return y
    _check_phase(phase, B, K, c.device)
    lib = _lib.lib()
    n = lib.ddsp_sinusoids_scratch_bytes(B, T, K, hop)
    scratch = torch.empty(n, device=c.device, dtype=torch.uint8) if n else None
    with torch.cuda.device(c.device):
        rc = lib.ddsp_sinusoids_forward(f.data_ptr(), c.data_ptr(), a.data_ptr(), y.data_ptr(), _dev_ptr(scratch), _dev_ptr(phase),
                                        B, T, K, hop, sample_rate, int(bool(normalize)), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_sinusoids_forward")
    return y


def sinusoids_backward(grad_y, f, c, a, hop: int, sample_rate: int, phase=None, normalize: bool = True, want_grad_f: bool = True):
    """Raw launcher of ddsp_sinusoids_backward -> (grad_f [B,T,K] or None, grad_c [B,T,K], grad_a [B,T,1]).  `phase`: the start
    phases the forward was given (as they were BEFORE it ran), or None.  Without `want_grad_f` the call passes no grad_f buffer
    and the kernels skip everything that serves it."""
    _check_inputs(f, c, a)
    f = f.detach().contiguous().float()
    c = c.detach().contiguous().float()
    a = a.detach().contiguous().float()
    grad_y = grad_y.detach().contiguous().float()
    B, T, K = c.shape
    _check_range(K, hop)
    grad_f = torch.empty_like(f) if want_grad_f else None
    grad_c, grad_a = torch.empty_like(c), torch.empty_like(a)
    if B == 0:
        return grad_f, grad_c, grad_a
    _check_phase(phase, B, K, c.device)
    lib = _lib.lib()
    scratch = torch.empty(lib.ddsp_sinusoids_backward_scratch_bytes(B, T, K, hop, int(want_grad_f)), device=c.device, dtype=torch.uint8)
    with torch.cuda.device(c.device):
        rc = lib.ddsp_sinusoids_backward(grad_y.data_ptr(), f.data_ptr(), c.data_ptr(), a.data_ptr(), scratch.data_ptr(), _dev_ptr(grad_f),
                                         grad_c.data_ptr(), grad_a.data_ptr(), _dev_ptr(phase), B, T, K, hop, sample_rate,
                                         int(bool(normalize)), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_sinusoids_backward")
    return grad_f, grad_c, grad_a


class _SinusoidsFunction(torch.autograd.Function):
    """Differentiable w.r.t. f, c and a; grad_f is computed only when f requires a gradient."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, f, c, a, hop, sample_rate, normalize):
        ctx.want_grad_f = bool(ctx.needs_input_grad[0])
        f = f.detach().contiguous().float()
        c = c.detach().contiguous().float()
        a = a.detach().contiguous().float()
        y = sinusoids_forward(f, c, a, hop, sample_rate, normalize=normalize)
        ctx.save_for_backward(f, c, a)
        ctx.hop, ctx.sample_rate, ctx.normalize = hop, sample_rate, normalize
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y):
        f, c, a = ctx.saved_tensors
        grad_f, grad_c, grad_a = sinusoids_backward(grad_y, f, c, a, ctx.hop, ctx.sample_rate, normalize=ctx.normalize,
                                                    want_grad_f=ctx.want_grad_f)
        return grad_f, grad_c, grad_a, None, None, None


def stretched_ratios(K: int, B_coef: float = 0.0) -> torch.Tensor:
    """[K] fp32: k sqrt(1 + B k^2) for k = 1 .. K, the partials of a stiff string; B = 0 gives exactly 1 .. K."""
    k = torch.arange(1, int(K) + 1, dtype=torch.float64)
    return (k * torch.sqrt(1.0 + float(B_coef) * k * k)).float()


class InharmonicBank(nn.Module):
    def __init__(self, conf, n_partials=None, ratios=None, inharmonicity: float = 0.0, learn: bool = True):
        super().__init__()
        if ratios is not None:
            ratios = torch.as_tensor(ratios, dtype=torch.float32).detach().clone().reshape(-1)
            if n_partials is not None and int(n_partials) != ratios.numel():
                raise ValueError(f"InharmonicBank: n_partials = {n_partials} but {ratios.numel()} ratios were given")
            n_partials = ratios.numel()
        if n_partials is None:
            n_partials = conf.n_harmonics
        self.n_partials = int(n_partials)
        if self.n_partials < 1:
            raise ValueError(f"InharmonicBank needs n_partials >= 1, got {n_partials}")
        self.sample_rate = conf.sample_rate
        self.hop_size = conf.hop_length
        self.learn = bool(learn)
        self.inharmonicity = nn.Parameter(torch.tensor(float(inharmonicity)), requires_grad=self.learn)
        self.detune_cents = nn.Parameter(torch.zeros(self.n_partials), requires_grad=self.learn)
        self.register_buffer("base_ratios", torch.arange(1, self.n_partials + 1, dtype=torch.float32) if ratios is None else ratios)
        # the live stream's phase per batch row and partial (turns, fp64), updated in place by the kernel; not part of the state dict
        self.register_buffer("phase", torch.zeros((1, self.n_partials), dtype=torch.float64), persistent=False)

    def ratios(self) -> torch.Tensor:
        """[K]: base_ratios sqrt(1 + B base_ratios^2) 2^(detune / 1200), differentiable w.r.t. the two parameters.  Partials that
        are neither stretched nor detuned keep their base ratio to the bit (B = 0, detune = 0: the harmonic series)."""
        r = self.base_ratios
        B = self.inharmonicity.clamp(min=0)
        return r * torch.sqrt(1.0 + B * r * r) * torch.exp2(self.detune_cents / 1200.0)

    def frequencies(self, x) -> torch.Tensor:
        """f [B,T,K] in Hz from `x['f0']` and `x['ratios']` [B,T,K] where given, else the module's own ratios; f0 gets no gradient"""
        f0 = x['f0'].detach().float()
        if f0.dim() != 3 or f0.shape[-1] != 1:
            raise ValueError(f"expected f0 [B,T,1], got {tuple(f0.shape)}")
        r = x.get('ratios') if hasattr(x, 'get') else None
        if r is not None:
            if r.dim() != 3 or r.shape[:2] != f0.shape[:2] or r.shape[-1] != self.n_partials:
                raise ValueError(f"expected ratios {tuple(f0.shape[:2]) + (self.n_partials,)}, got {tuple(r.shape)}")
            return f0 * r.float()
        return f0 * self.ratios().to(f0.device)

    def forward(self, x):
        c, a = x['c'], x['a']
        f = self.frequencies(x)
        _check_inputs(f, c, a)
        if torch.is_grad_enabled() and (f.requires_grad or c.requires_grad or a.requires_grad):
            _check_range(c.shape[-1], self.hop_size)
            return _SinusoidsFunction.apply(f, c, a, self.hop_size, self.sample_rate, True)
        return sinusoids_forward(f, c, a, self.hop_size, self.sample_rate)

    def live(self, x):
        """One block of a stream: the phase per row and partial is carried on the device (one launch, capturable in a graph once
        the phase buffer has its size, i.e. after a first call)."""
        c, a = x['c'], x['a']
        with torch.no_grad():
            f = self.frequencies(x)
        _check_inputs(f, c, a)
        B, K = c.shape[0], c.shape[-1]
        if self.phase.shape != (B, K) or self.phase.device != c.device:
            self.phase = torch.zeros((B, K), dtype=torch.float64, device=c.device)
        return sinusoids_forward(f, c, a, self.hop_size, self.sample_rate, phase=self.phase)

    def reset_phase(self):
        self.phase.zero_()

    def init_from(self, ctrl) -> None:
        """Starting values of the two trainable parameters from an analysed dict (partials.inharmonic_analysis): `inharmonicity`
        becomes the mean of ctrl['inharmonicity'] [B], `detune_cents` [K] the a c weighted mean over the frames of
        1200 log2(ratios / rho(B)), rho(B) = base_ratios sqrt(1 + B base_ratios^2); a partial without weight keeps detune 0.  The
        state-dict keys are unchanged."""
        with torch.no_grad():
            B_coef = ctrl['inharmonicity'].detach().double().reshape(-1).mean().clamp(min=0)
            self.inharmonicity.copy_(B_coef.to(self.inharmonicity))
            r = self.base_ratios.double().to(B_coef.device)
            rho = r * torch.sqrt(1.0 + B_coef * r * r)
            ratios = ctrl['ratios'].detach().double()
            if ratios.dim() != 3 or ratios.shape[-1] != self.n_partials:
                raise ValueError(f"init_from: expected ratios [B, T, {self.n_partials}], got {tuple(ratios.shape)}")
            weight = (ctrl['a'].detach().double() * ctrl['c'].detach().double()).expand_as(ratios)
            ok = torch.isfinite(ratios) & (ratios > 0) & torch.isfinite(weight) & (weight > 0)
            weight = torch.where(ok, weight, torch.zeros_like(weight))
            cents = 1200.0 * torch.log2(torch.where(ok, ratios, rho.expand_as(ratios)) / rho)
            total = weight.sum((0, 1))
            detune = (weight * cents).sum((0, 1)) / torch.where(total > 0, total, torch.ones_like(total))
            self.detune_cents.copy_(detune.to(self.detune_cents))

    def export_ratios(self) -> torch.Tensor:
        """The learned frequency ratios [K] on the CPU: the inharmonicity as a tensor to inspect, store or give to another model."""
        with torch.no_grad():
            return self.ratios().detach().to(device="cpu", dtype=torch.float32).clone()


def is_inharmonic(decoder) -> bool:
    return isinstance(getattr(decoder, 'harmonics', None), InharmonicBank)


def refuse_inharmonic(decoder_or_flag, what: str) -> None:
    """The one refusal of every entry point whose meaning rests on the partials being harmonics of f0 or on the bank's `last_phases`."""
    flag = decoder_or_flag if isinstance(decoder_or_flag, bool) else is_inharmonic(decoder_or_flag)
    if flag:
        raise ValueError(f"{what}: not available with the inharmonic synthesiser (synth='inharmonic'): it rests on partials at whole "
                         "multiples of f0 or on the oscillator bank's carried phases; build the decoder with synth='harmonic'")
