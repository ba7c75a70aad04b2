"""The audio encoder: audio in, control features out (model/autoencoder/encoder.py, crepe/crepe.py of the reference).

  Crepe            the CREPE pitch network ('tiny' / 'full'); parameter and buffer names as crepe/crepe.py:12-91, so that a
                   CREPE `.pth` state dict loads with strict=True
  F0Encoder        resample to 16 kHz -> normalise -> frame by 1024 -> CREPE -> argmax pitch (encoder.py:13-88, 120-128)
  LoudnessEncoder  A-weighted loudness of the un-windowed STFT (encoder.py:131-156)
  Encoder          both, as the dict {f0, harmonicity, loudness, probabilities, normalized_cents} (encoder.py:159-177)

On CUDA tensors the work runs on hand-written HIP (csrc/ddsp_encoder.hip, csrc/ddsp_loudness.hip; include/ddsp_hip.h) around
the library work it keeps: CREPE's convolutions on MIOpen (F.conv1d on a [N, C, L] view of the (k, 1) weights) and its
classifier on rocBLAS.  CPU tensors run the reference's arithmetic as stock torch ops (the restatement the fixtures pin).

Two pieces restate libraries the reference imports and this package does not have; their parity with those libraries
cannot be pinned here:
  * `sinc_resample_kernel`: torchaudio.transforms.Resample(orig, new) with its defaults (Hann-windowed sinc, lowpass
    width 6, rolloff 0.99), kernel built in float64 and stored as float32;
  * `a_weighting`: librosa.A_weighting's published formula (min_db = -80), float64 (what librosa returns for float32
    frequencies under NumPy 2's promotion rules, and so the dtype of the reference's parameter).

There is no autograd: the reference runs the pitch path under no_grad and nothing differentiates through loudness, so an
input that requires grad is refused rather than silently detached.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

PITCH_BINS = 360
CREPE_RATE = 16000
CREPE_WINDOW = 1024
_BN_EPS = 0.0010000000474974513          # the MMdnn-converted CREPE's BatchNorm epsilon
_LOWPASS_WIDTH = 6
_ROLLOFF = 0.99

# channel plans: in / out channels of conv1 .. conv6 and the classifier's input width (crepe.py:17-26)
CREPE_PLANS = {
    'full': ([1, 1024, 128, 128, 128, 256], [1024, 128, 128, 128, 256, 512], 2048),
    'tiny': ([1, 128, 16, 16, 16, 32], [128, 16, 16, 16, 32, 64], 256),
}


def _refuse_grad(x: torch.Tensor, what: str) -> None:
    if x.requires_grad:
        raise RuntimeError(f"{what} has no backward (the reference encodes under no_grad); pass a tensor that does not require grad")


# ---------------------------------------------------------------------------------------------------------------- resampler

def sinc_resample_kernel(orig: int, new: int):
    """Restatement of torchaudio's windowed-sinc kernel: -> (kernel [new', 1, 2 width + orig'] fp32, width, orig', new') with the
    rates reduced by their gcd.  Row r holds the taps of output phase r against the input window starting at (j div new') orig'."""
    g = math.gcd(int(orig), int(new))
    orig, new = int(orig) // g, int(new) // g
    base = min(orig, new) * _ROLLOFF
    width = math.ceil(_LOWPASS_WIDTH * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float32)[:, None, None] / new + idx
    t *= base
    t = t.clamp_(-_LOWPASS_WIDTH, _LOWPASS_WIDTH)
    window = torch.cos(t * math.pi / _LOWPASS_WIDTH / 2) ** 2
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * (base / orig)
    return kernels.to(torch.float32), width, orig, new


def support_taps(orig: int, new: int):
    """The device table: per phase row only the taps inside the sinc's support (|t| < lowpass width before the clamp); the
    others are the clamped window's residue (<= 1.8e-24 at 441 -> 160) and are skipped.  -> (table [new', K] fp32,
    first [new'] int32 = offset of the row's first kept tap relative to the unpadded window start, K)."""
    kernel, width, o, n = sinc_resample_kernel(orig, new)
    base = min(o, n) * _ROLLOFF
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    t = (torch.arange(0, -n, -1, dtype=torch.float32)[:, None] / n + idx) * base
    inside = t.abs() < _LOWPASS_WIDTH
    lo = [int(torch.nonzero(inside[r])[0]) for r in range(n)]
    hi = [int(torch.nonzero(inside[r])[-1]) for r in range(n)]
    K = max(h - l + 1 for l, h in zip(lo, hi))
    K = min(K, kernel.shape[-1])
    lo = [min(l, kernel.shape[-1] - K) for l in lo]
    table = torch.stack([kernel[r, 0, l:l + K] for r, l in enumerate(lo)])
    first = torch.tensor([l - width for l in lo], dtype=torch.int32)
    return table.contiguous(), first, K


def resampled_length(L: int, orig: int, new: int) -> int:
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    return int(math.ceil(n * L / o)) if o != n else L


class Resample(nn.Module):
    """orig -> new Hz (torchaudio.transforms.Resample semantics; equal rates are the identity).  The kernel is not part of the
    state dict (torchaudio keeps it out as well)."""

    def __init__(self, orig: int, new: int):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig), int(new)
        self.identity = self.orig_freq == self.new_freq
        if not self.identity:
            kernel, self.width, self.orig, self.new = sinc_resample_kernel(orig, new)
            table, first, self.ntaps = support_taps(orig, new)
            self.register_buffer("kernel", kernel, persistent=False)
            self.register_buffer("table", table, persistent=False)
            self.register_buffer("first", first, persistent=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.identity:
            return x
        B, L = x.shape
        target = resampled_length(L, self.orig_freq, self.new_freq)
        if x.is_cuda:
            x = x.contiguous().float()
            y = torch.empty((B, target), device=x.device, dtype=torch.float32)
            with torch.cuda.device(x.device):
                rc = _lib.lib().ddsp_resample(x.data_ptr(), self.table.data_ptr(), self.first.data_ptr(), y.data_ptr(), B, L,
                                              self.orig, self.new, self.ntaps, torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "ddsp_resample")
            return y
        xp = F.pad(x, (self.width, self.width + self.orig))
        y = F.conv1d(xp[:, None], self.kernel, stride=self.orig)
        return y.transpose(1, 2).reshape(B, -1)[..., :target]


# ------------------------------------------------------------------------------------------------------------------- CREPE

class Crepe(nn.Module):
    """CREPE: six (conv (k, 1) -> ReLU -> BatchNorm -> max-pool (2, 1)) layers and a 360-bin sigmoid classifier.  Input
    [N, 1024] frames at 16 kHz, output probabilities [N, 360]."""

    def __init__(self, model: str = 'full'):
        super().__init__()
        if model not in CREPE_PLANS:
            raise ValueError(f"CREPE model {model!r}: expected 'tiny' or 'full'")
        cin, cout, self.in_features = CREPE_PLANS[model]
        self.capacity = model
        for i in range(6):
            k, s = (512, 4) if i == 0 else (64, 1)
            setattr(self, f"conv{i + 1}", nn.Conv2d(cin[i], cout[i], (k, 1), (s, 1)))
            setattr(self, f"conv{i + 1}_BN", nn.BatchNorm2d(cout[i], eps=_BN_EPS, momentum=0.0))
        self.classifier = nn.Linear(self.in_features, PITCH_BINS)

    def layers(self):
        return [(getattr(self, f"conv{i}"), getattr(self, f"conv{i}_BN")) for i in range(1, 7)]

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        """CPU / stock-torch form: pad -> conv -> ReLU -> BatchNorm -> max-pool per layer, then sigmoid(Linear)."""
        x = frames[:, None, :, None]
        for i, (conv, bn) in enumerate(self.layers()):
            x = F.pad(x, (0, 0, 254, 254) if i == 0 else (0, 0, 31, 32))
            x = F.max_pool2d(bn(F.relu(conv(x))), (2, 1), (2, 1))
        x = x.permute(0, 2, 1, 3).reshape(-1, self.in_features)
        return torch.sigmoid(self.classifier(x))

    def logits_device(self, padded: torch.Tensor) -> torch.Tensor:
        """HIP form, eval only: padded [N, 1532] (conv1's padded input, ddsp_crepe_frames) -> classifier logits [N, 360]
        without the bias (ddsp_pitch_decode adds it).  Convolutions on MIOpen, the rest of each layer one HIP launch."""
        L = _lib.lib()
        N = padded.shape[0]
        x = padded.view(N, 1, -1)
        stream = torch.cuda.current_stream().cuda_stream
        for i, (conv, bn) in enumerate(self.layers()):
            w = conv.weight
            y = F.conv1d(x, w.view(w.shape[0], w.shape[1], w.shape[2]), stride=conv.stride[0])
            C, Lc = y.shape[1], y.shape[2]
            last = i == 5
            out = torch.empty((N, (Lc // 2) * C) if last else (N, C, Lc // 2 + 63), device=y.device, dtype=torch.float32)
            rc = L.ddsp_crepe_epilogue(y.data_ptr(), conv.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                       bn.weight.data_ptr(), bn.bias.data_ptr(), out.data_ptr(), N, C, Lc, int(last), stream)
            _lib.check(rc, "ddsp_crepe_epilogue")
            x = out
        return torch.mm(x, self.classifier.weight.t())


def pitch_tables():
    """f0 and normalised-cents lookups of the 360 bins, with the reference's own ops on an int64 bin index
    (encoder.py:41-50, 120-128): bit-exact with what pitch_argmax computes, and no device exp2."""
    bins = torch.arange(PITCH_BINS)
    cents = bins * 20 + 1997.3794084376191
    return 10 * 2 ** (cents / 1200), bins / 359.


def _load_crepe_weights(weights):
    if isinstance(weights, (str, os.PathLike)):
        return torch.load(weights, map_location="cpu", weights_only=True)
    return weights


class F0Encoder(nn.Module):
    """Pitch features of audio at conf.sample_rate: forward(batch [B, L]) -> (freq, harmonicity, probabilities,
    normalized_cents), shapes [B, T, 1], [B, T, 1], [B, T, 360], [B, T, 1].

    The reference loads crepe/pretrained/{capacity}.pth from its own tree; this package ships no weights, so they come from
    `weights` (a path to a CREPE state dict or the dict itself), else from `conf.crepe_weights`.  With neither it raises
    rather than run untrained weights."""

    def __init__(self, conf, weights=None):
        super().__init__()
        self.hop_length = conf.hop_length
        self.window_size = conf.n_fft
        self.rs = Resample(conf.sample_rate, CREPE_RATE)
        self.model = Crepe(conf.crepe_capacity)
        if weights is None:
            weights = getattr(conf, 'crepe_weights', None)
        if weights is None:
            raise ValueError("F0Encoder needs CREPE weights: pass weights=<path or state dict> or set conf.crepe_weights "
                             f"(a '{conf.crepe_capacity}' CREPE state dict; this package ships none)")
        self.model.load_state_dict(_load_crepe_weights(weights), strict=True)
        self.model.eval()
        for p in self.model.parameters():
            p.requires_grad = False
        f0_table, cents_table = pitch_tables()
        self.register_buffer("f0_table", f0_table, persistent=False)
        self.register_buffer("cents_table", cents_table, persistent=False)

    def resampled_hop(self, orig_len: int, resampled_len: int) -> int:
        """encoder.py:66-69 in Python arithmetic; refuses inputs shorter than one frame."""
        if orig_len <= self.window_size or resampled_len < CREPE_WINDOW:
            raise ValueError(f"audio of {orig_len} samples is too short for one frame (needs more than n_fft = {self.window_size})")
        hop = int(self.hop_length * ((resampled_len - 1024) / (orig_len - self.window_size)))
        if hop <= 0:
            raise ValueError(f"audio of {orig_len} samples gives a resampled hop of {hop}: too short to frame")
        return hop

    def forward(self, batch: torch.Tensor):
        _refuse_grad(batch, "F0Encoder")
        with torch.no_grad():
            if batch.is_cuda:
                return self._forward_device(batch)
            orig_len = batch.shape[1]
            x = self.rs(batch)
            x = x - x.mean(dim=1, keepdim=True)
            x = x / x.std(dim=1, keepdim=True)
            hop = self.resampled_hop(orig_len, x.shape[1])
            x = x.unfold(1, CREPE_WINDOW, hop)
            B, T = x.shape[:2]
            probabilities = self.model(x.reshape(-1, CREPE_WINDOW)).reshape(B, T, PITCH_BINS)
            bins = probabilities.argmax(dim=-1, keepdim=True)
            freq = 10 * 2 ** ((bins * 20 + 1997.3794084376191) / 1200)
            return freq, probabilities.gather(-1, bins), probabilities, bins / 359.

    def _forward_device(self, batch: torch.Tensor):
        L = _lib.lib()
        B, orig_len = batch.shape
        with torch.cuda.device(batch.device):
            stream = torch.cuda.current_stream().cuda_stream
            y = self.rs(batch.contiguous().float()).contiguous()
            Lr = y.shape[1]
            hop = self.resampled_hop(orig_len, Lr)
            T = 1 + (Lr - CREPE_WINDOW) // hop
            stats = torch.empty((B, 2), device=y.device, dtype=torch.float32)
            frames = torch.empty((B * T, CREPE_WINDOW + 2 * 254), device=y.device, dtype=torch.float32)
            _lib.check(L.ddsp_crepe_frames(y.data_ptr(), stats.data_ptr(), frames.data_ptr(), B, Lr, hop, T, stream), "ddsp_crepe_frames")
            logits = self.model.logits_device(frames)
            N = B * T
            probs = torch.empty((B, T, PITCH_BINS), device=y.device, dtype=torch.float32)
            out = torch.empty((3, B, T, 1), device=y.device, dtype=torch.float32)
            rc = L.ddsp_pitch_decode(logits.data_ptr(), self.model.classifier.bias.data_ptr(), self.f0_table.data_ptr(),
                                     self.cents_table.data_ptr(), probs.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                     out[2].data_ptr(), N, stream)
            _lib.check(rc, "ddsp_pitch_decode")
        return out[0], out[1], probs, out[2]


# ---------------------------------------------------------------------------------------------------------------- loudness

def a_weighting(frequencies: np.ndarray, min_db: float = -80.0) -> np.ndarray:
    """Restatement of librosa.A_weighting (the published IEC 61672 curve, min_db = -80 so bin 0 is -80 dB), in float64."""
    f_sq = np.asarray(frequencies, dtype=np.float64) ** 2.0
    const = np.array([12194.217, 20.598997, 107.65265, 737.86223]) ** 2.0
    with np.errstate(divide="ignore"):
        weights = 2.0 + 20.0 * (np.log10(const[0]) + 2 * np.log10(f_sq) - np.log10(f_sq + const[0]) - np.log10(f_sq + const[1])
                                - 0.5 * np.log10(f_sq + const[2]) - 0.5 * np.log10(f_sq + const[3]))
    return np.maximum(min_db, weights)


class LoudnessEncoder(nn.Module):
    """forward(signal [B, L]) -> loudness [B, F, 1], F = 1 + (L - n_fft) // hop.  On the device one HIP launch
    (ddsp_loudness) for n_fft a power of two in [64, 2048]; any other n_fft runs the stock torch ops on the device."""

    def __init__(self, conf):
        super().__init__()
        self.n_fft = conf.n_fft
        self.hop_length = conf.hop_length
        self.sample_rate = conf.sample_rate
        freqs = np.linspace(0, float(self.sample_rate) / 2, int(1 + self.n_fft // 2), endpoint=True, dtype='float32')
        self.a_weight = nn.Parameter(torch.from_numpy(a_weighting(freqs)), requires_grad=False)

    def forward(self, signal: torch.Tensor) -> torch.Tensor:
        _refuse_grad(signal, "LoudnessEncoder")
        if signal.shape[-1] < self.n_fft:
            raise ValueError(f"audio of {signal.shape[-1]} samples is too short for one frame of n_fft = {self.n_fft}")
        if signal.is_cuda and _lib.lib().ddsp_loudness_supported(self.n_fft):
            x = signal.contiguous().float()
            B, Ls = x.shape
            out = torch.empty((B, 1 + (Ls - self.n_fft) // self.hop_length, 1), device=x.device, dtype=torch.float32)
            aw = self.a_weight.detach().to(torch.float64).contiguous()
            with torch.cuda.device(x.device):
                rc = _lib.lib().ddsp_loudness(x.data_ptr(), aw.data_ptr(), out.data_ptr(), B, Ls, self.n_fft, self.hop_length,
                                              torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "ddsp_loudness")
            return out
        with torch.no_grad():
            stft = torch.stft(signal, n_fft=self.n_fft, hop_length=self.hop_length, center=False, return_complex=True).permute(0, 2, 1)
            db = torch.log10(torch.abs(stft) + 1e-20) * 20
            db += self.a_weight
            db = db / 90 + 1
            return torch.mean(db, dim=-1, keepdim=True)


class Encoder(nn.Module):
    """audio [B, L] -> {f0, harmonicity, loudness, probabilities, normalized_cents} (encoder.py:159-177)."""

    def __init__(self, conf, weights=None):
        super().__init__()
        self.conf = conf
        self.f0_encoder = F0Encoder(conf, weights)
        self.loudness_encoder = LoudnessEncoder(conf)

    def forward(self, x: torch.Tensor) -> dict:
        f0, harmonicity, probabilities, normalized_cents = self.f0_encoder(x)
        loudness = self.loudness_encoder(x)
        return dict(f0=f0, harmonicity=harmonicity, loudness=loudness, probabilities=probabilities, normalized_cents=normalized_cents)
