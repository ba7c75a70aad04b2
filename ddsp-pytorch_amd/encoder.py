"""The audio encoder: audio in, control features out (model/autoencoder/encoder.py, crepe/crepe.py of the reference).

  Crepe            the CREPE pitch network ('tiny' / 'full'); parameter and buffer names as crepe/crepe.py:12-91, so that a
                   CREPE `.pth` state dict loads with strict=True
  F0Encoder        resample to 16 kHz -> normalise -> frame by 1024 -> CREPE -> pitch (encoder.py:13-128): the argmax bin by
                   default, or the nine-bin weighted average around the argmax ('weighted') or around a Viterbi path ('viterbi')
  pitch_argmax, pitch_centered, pitch_weighted, pitch_viterbi   the decoders themselves, over probabilities [B, T, 360]
  pitch_salience_yin   a salience [B, T, 360] without a network: the YIN difference function of CREPE's own frames,
                   cumulative-mean normalised and read at each bin's lag (one launch; `F0Encoder(tracker='yin')` decodes it)
  pitch_voicing    what follows a decoder: periodicity smoothing and hysteresis, loudness gate, median-filtered voiced pitch,
                   unvoiced gaps held or interpolated (one launch; `Encoder(voicing=...)` applies it, off by default)
  LoudnessEncoder  A-weighted loudness of the un-windowed STFT (encoder.py:131-156)
  Encoder          both, as the dict {f0, harmonicity, loudness, probabilities, normalized_cents} (encoder.py:159-177)
  mfcc, MFCC       mel-frequency cepstral coefficients on LoudnessEncoder's frame grid (one launch, csrc/ddsp_mfcc.hip)
  ZEncoder         the timbre latent z of the DDSP autoencoder: MFCC -> LayerNorm -> GRU -> Linear (the decoder owns one when
                   conf.z_dims > 0)

On CUDA tensors the work runs on hand-written HIP (csrc/ddsp_encoder.hip, csrc/ddsp_pitch.hip, csrc/ddsp_yin.hip, csrc/ddsp_loudness.hip;
include/ddsp_hip.h) around the library work it keeps: CREPE's convolutions on MIOpen (F.conv1d on a [N, C, L] view of the
(k, 1) weights) and its classifier on rocBLAS.  CPU tensors run the reference's arithmetic as stock torch ops (the
restatement the fixtures pin).

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

import contextlib
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import dense
from .gru import GRU

PITCH_BINS = 360
PITCH_DECODERS = ('argmax', 'weighted', 'viterbi')
PITCH_TRACKERS = ('crepe', 'yin')
CENTS_OF_BIN_0 = 1997.3794084376191
CENTERED_HALF_WIDTH = 4                  # pitch_centered averages bins c - 4 .. c + 4
VITERBI_BAND = 11                        # a Viterbi path moves at most 11 bins (220 cents) per frame
CREPE_RATE = 16000
CREPE_WINDOW = 1024
YIN_LAGS = 512                           # the difference function: lags 0 .. 511, 512 terms each
YIN_OCTAVE_COST = 0.05
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


RESAMPLE_TABLE_MAX = 16384               # floats of LDS that resample_kernel keeps its taps in (csrc/ddsp_encoder.hip: kMaxTable;
                                         # tests/test_encoder_reference_host.py holds the two together)


class Resample(nn.Module):
    """orig -> new Hz (torchaudio.transforms.Resample semantics; equal rates are the identity).  The kernel is not part of the
    state dict (torchaudio keeps it out as well).  On the device one HIP launch (ddsp_resample) where the rate pair's table of
    new' x ntaps support taps fits the kernel's LDS (`fits_kernel`; every pair of common audio rates does); a pair that does not
    (44056 -> 16000 reduces to 5507 : 2000, 2000 x 34 taps) runs the stock pad + conv1d formulation on the device."""

    def __init__(self, orig: int, new: int):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig), int(new)
        self.identity = self.orig_freq == self.new_freq
        self.fits_kernel = True
        if not self.identity:
            kernel, self.width, self.orig, self.new = sinc_resample_kernel(orig, new)
            table, first, self.ntaps = support_taps(orig, new)
            self.register_buffer("kernel", kernel, persistent=False)
            self.register_buffer("table", table, persistent=False)
            self.register_buffer("first", first, persistent=False)
            self.fits_kernel = self.new * self.ntaps <= RESAMPLE_TABLE_MAX

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.identity:
            return x
        B, L = x.shape
        target = resampled_length(L, self.orig_freq, self.new_freq)
        if x.is_cuda and self.fits_kernel:
            x = x.contiguous().float()
            y = torch.empty((B, target), device=x.device, dtype=torch.float32)
            with torch.cuda.device(x.device):
                rc = _lib.lib().ddsp_resample(x.data_ptr(), self.table.data_ptr(), self.first.data_ptr(), y.data_ptr(), B, L,
                                              self.orig, self.new, self.ntaps, torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "ddsp_resample")
            return y
        xp = F.pad(x.float() if x.is_cuda else x, (self.width, self.width + self.orig))
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


# ------------------------------------------------------------------------------------------------------------ pitch decoders
# Definitions: DESIGN.md section 10.  CUDA fp32 tensors run csrc/ddsp_pitch.hip; CPU tensors run the same definitions as stock
# torch / numpy ops (the Viterbi recurrence in fp64).

def _cents_map(bins):
    return bins * 20 + CENTS_OF_BIN_0


def _freq_map(cents):
    return 10 * 2 ** (cents / 1200)


def viterbi_log_transition() -> torch.Tensor:
    """log A as the kernel reads it: [360, 23] fp32 indexed by target bin j and k - j + 11, A[k][j] = max(12 - |k - j|, 0) / S_k
    with S_k the row sum (144 in the interior, less within 11 bins of an end); -inf where k is outside 0 .. 359.  Built in
    fp64 and rounded once."""
    k = np.arange(PITCH_BINS)
    A = np.maximum(VITERBI_BAND + 1 - np.abs(k[:, None] - k[None, :]), 0).astype(np.float64)
    A /= A.sum(axis=1, keepdims=True)
    table = np.full((PITCH_BINS, 2 * VITERBI_BAND + 1), -np.inf)
    for d in range(2 * VITERBI_BAND + 1):
        src = k + d - VITERBI_BAND
        ok = (src >= 0) & (src < PITCH_BINS)
        table[k[ok], d] = np.log(A[src[ok], k[ok]])
    return torch.from_numpy(table.astype(np.float32))


_DEVICE_TABLES = {}


def _tables_on(device, build):
    """The host tables `build()` returns, copied to `device` once (a copy per call would also keep a caller out of a graph)."""
    key = (build.__name__, str(device))
    if key not in _DEVICE_TABLES:
        made = build()
        _DEVICE_TABLES[key] = tuple(t.to(device) for t in made) if isinstance(made, tuple) else made.to(device)
    return _DEVICE_TABLES[key]


def _decoder_input(probabilities: torch.Tensor, what: str) -> torch.Tensor:
    if probabilities.dim() != 3 or probabilities.shape[-1] != PITCH_BINS:
        raise ValueError(f"{what}: probabilities must be [B, T, {PITCH_BINS}], got {tuple(probabilities.shape)}")
    _refuse_grad(probabilities, what)
    if probabilities.is_cuda:
        return probabilities.detach().contiguous().float()
    return probabilities.detach()


def _centered_device(center, p: torch.Tensor):
    """ddsp_pitch_centered: center None = the kernel's own argmax.  -> (freq, harmonicity, normalized_cents, bins int32 [B, T])"""
    B, T = p.shape[:2]
    out = torch.empty((3, B, T, 1), device=p.device, dtype=torch.float32)
    bins = torch.empty((B, T), device=p.device, dtype=torch.int32)
    if center is not None:
        center = center.to(device=p.device, dtype=torch.int32).reshape(B, T).contiguous()
    with torch.cuda.device(p.device):
        rc = _lib.lib().ddsp_pitch_centered(p.data_ptr(), center.data_ptr() if center is not None else None, out[0].data_ptr(),
                                            out[1].data_ptr(), out[2].data_ptr(), bins.data_ptr(), B * T,
                                            torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_pitch_centered")
    return out[0], out[1], out[2], bins


def pitch_argmax(probabilities: torch.Tensor):
    """encoder.py:120-128: -> (freq, harmonicity, normalized_cents) of each frame's argmax bin, each [B, T, 1]."""
    p = _decoder_input(probabilities, "pitch_argmax")
    if p.is_cuda:
        _, harmonicity, _, bins = _centered_device(None, p)
        f0_table, cents_table = _tables_on(p.device, pitch_tables)
        bins = bins.long().unsqueeze(-1)
        return f0_table[bins], harmonicity, cents_table[bins]
    bins = p.argmax(dim=-1, keepdim=True)
    return _freq_map(_cents_map(bins)), p.gather(-1, bins), bins / 359.


def pitch_centered(center: torch.Tensor, probabilities: torch.Tensor):
    """The weighted average of the bins center - 4 .. center + 4 (those inside 0 .. 359), every probability with its own
    bin's cents: -> (freq, harmonicity, normalized_cents), each [B, T, 1]; center [B, T, 1] integer bins.  The reference's
    method of this name (encoder.py:95-118) pairs the nine probabilities with a rotated list of cents; this is its evident
    intent."""
    p = _decoder_input(probabilities, "pitch_centered")
    B, T = p.shape[:2]
    if tuple(center.shape) != (B, T, 1) or center.dtype.is_floating_point:
        raise ValueError(f"pitch_centered: center must be integer bins [B, T, 1] = {(B, T, 1)}, got {center.dtype} {tuple(center.shape)}")
    if p.is_cuda:
        return _centered_device(center, p)[:3]
    center = center.long().clamp(0, PITCH_BINS - 1)
    p = p.float()
    idx = center + torch.arange(-CENTERED_HALF_WIDTH, CENTERED_HALF_WIDTH + 1)
    w = p.gather(-1, idx.clamp(0, PITCH_BINS - 1))
    w = torch.where((idx >= 0) & (idx < PITCH_BINS), w, torch.zeros((), dtype=w.dtype))
    num = torch.zeros((B, T, 1), dtype=torch.float32)
    den = torch.zeros((B, T, 1), dtype=torch.float32)
    for i in range(2 * CENTERED_HALF_WIDTH + 1):             # ascending offsets, as the kernel sums them
        num = num + float(i - CENTERED_HALF_WIDTH) * w[..., i:i + 1]
        den = den + w[..., i:i + 1]
    offset = (20 * (num / den)).double()                     # the fp32 quantity; the rest in fp64, rounded once (as the kernel)
    base = (center * 20).double()
    cents = (base + CENTS_OF_BIN_0) + offset
    return _freq_map(cents).float(), p.gather(-1, center), ((base + offset) / (20. * (PITCH_BINS - 1))).float()


def pitch_weighted(probabilities: torch.Tensor):
    """encoder.py:91-93: pitch_centered around each frame's own argmax."""
    p = _decoder_input(probabilities, "pitch_weighted")
    if p.is_cuda:
        return _centered_device(None, p)[:3]
    return pitch_centered(p.argmax(dim=-1, keepdim=True), p)


def _viterbi_host(p: np.ndarray, state):
    """The recurrence of ddsp_pitch_viterbi in fp64 numpy: p [B, T, 360] -> (bins int64 [B, T], last scores [B, 360])."""
    B, T, _ = p.shape
    log_a = viterbi_log_transition().numpy().astype(np.float64)
    e = np.log(np.fmax(p.astype(np.float64), np.float64(np.float32(1e-30))))       # fmax drops a NaN

    def step(v):
        padded = np.full((B, PITCH_BINS + 2 * VITERBI_BAND), -np.inf)
        padded[:, VITERBI_BAND:VITERBI_BAND + PITCH_BINS] = v
        cand = np.stack([padded[:, d:d + PITCH_BINS] for d in range(2 * VITERBI_BAND + 1)], axis=-1) + log_a
        arg = cand.argmax(axis=-1)                                                    # first maximum: the lower predecessor
        return np.take_along_axis(cand, arg[..., None], axis=-1)[..., 0], arg - VITERBI_BAND

    back = np.zeros((B, T, PITCH_BINS), dtype=np.int64)
    v = e[:, 0] if state is None else step(np.asarray(state, dtype=np.float64))[0] + e[:, 0]
    for t in range(1, T):
        best, back[:, t] = step(v)
        v = best + e[:, t]
    bins = np.empty((B, T), dtype=np.int64)
    s = v.argmax(axis=-1)                                                             # first maximum: the lower final state
    bins[:, T - 1] = s
    rows = np.arange(B)
    for t in range(T - 1, 0, -1):
        s = s + back[rows, t, s]
        bins[:, t - 1] = s
    return bins, v - v.max(axis=-1, keepdims=True)


def pitch_viterbi(probabilities: torch.Tensor, state=None, return_state: bool = False):
    """The bins [B, T, 1] (int64) of the path maximising sum_t log max(p_t[s_t], 1e-30) + sum_{t >= 1} log A[s_{t-1}][s_t]
    under the triangular +-11-bin transition of `viterbi_log_transition`; ties go to the lower predecessor and to the lower
    final state, and a NaN frame is uninformative.  `state` [B, 360] fp32 (the scores a previous call returned) replaces
    the uniform prior, so a block-wise caller can carry the recurrence across calls; with a state, or return_state=True,
    the result is (bins, state).  Scores are defined up to one constant per row."""
    p = _decoder_input(probabilities, "pitch_viterbi")
    B, T = p.shape[:2]
    if T < 1:
        raise ValueError("pitch_viterbi: needs at least one frame")
    if state is not None and tuple(state.shape) != (B, PITCH_BINS):
        raise ValueError(f"pitch_viterbi: state must be [B, {PITCH_BINS}] = {(B, PITCH_BINS)}, got {tuple(state.shape)}")
    want_state = return_state or state is not None
    if p.is_cuda:
        L = _lib.lib()
        bins = torch.empty((B, T), device=p.device, dtype=torch.int32)
        if state is not None:
            state = state.to(device=p.device, dtype=torch.float32).contiguous()
        out = torch.empty((B, PITCH_BINS), device=p.device, dtype=torch.float32) if want_state else None
        nbytes = L.ddsp_pitch_viterbi_workspace_bytes(B, T)
        work = torch.empty(nbytes, device=p.device, dtype=torch.uint8) if nbytes else None
        with torch.cuda.device(p.device):
            rc = L.ddsp_pitch_viterbi(p.data_ptr(), _tables_on(p.device, viterbi_log_transition).data_ptr(),
                                      state.data_ptr() if state is not None else None, out.data_ptr() if want_state else None,
                                      bins.data_ptr(), work.data_ptr() if nbytes else None, B, T,
                                      torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_pitch_viterbi")
        bins = bins.long().unsqueeze(-1)
        return (bins, out) if want_state else bins
    path, last = _viterbi_host(p.float().numpy(), None if state is None else state.detach().cpu().numpy())
    bins = torch.from_numpy(path).unsqueeze(-1)
    return (bins, torch.from_numpy(last.astype(np.float32))) if want_state else bins


# -------------------------------------------------------------------------------------------------------------- YIN salience
# Definition: DESIGN.md section 10c (include/ddsp_hip.h: ddsp_yin_salience).  CUDA tensors take one launch of
# csrc/ddsp_yin.hip; CPU tensors run the same arithmetic as fp32 torch ops.

def yin_bin_table(octave_cost: float = YIN_OCTAVE_COST) -> torch.Tensor:
    """The per-bin constants ddsp_yin_salience reads, [360, 4] fp32 = {i_b, w_b, cost_b, 0}: integer part and fraction of the
    bin's lag tau_b = 16000 / f_b (f_b from pitch_tables) and cost_b = octave_cost * log2(tau_b / tau_359); built in fp64 and
    rounded once."""
    tau = CREPE_RATE / pitch_tables()[0].numpy().astype(np.float64)
    whole = np.floor(tau)
    table = np.zeros((PITCH_BINS, 4))
    table[:, 0], table[:, 1], table[:, 2] = whole, tau - whole, float(octave_cost) * np.log2(tau / tau[-1])
    assert whole.min() >= 1 and whole.max() + 2 < YIN_LAGS
    return torch.from_numpy(table.astype(np.float32))


def _yin_table_on(device, octave_cost: float) -> torch.Tensor:
    key = ('yin_bin_table', str(device), float(octave_cost))
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = yin_bin_table(octave_cost).to(device)
    return _DEVICE_TABLES[key]


def _yin_salience_host(y: torch.Tensor, hop: int, table: torch.Tensor) -> torch.Tensor:
    """ddsp_yin_salience as torch ops on y [B, Lr] fp32 (torch's own summation orders)."""
    x = y.unfold(1, CREPE_WINDOW, hop)                                            # [B, T, 1024]
    head = x[..., :YIN_LAGS]
    d = torch.stack([((head - x[..., tau:tau + YIN_LAGS]) ** 2).sum(-1) for tau in range(YIN_LAGS)], dim=-1)
    c = torch.cumsum(d[..., 1:], dim=-1)
    lags = torch.arange(1, YIN_LAGS, dtype=torch.float32)
    one = torch.ones((), dtype=torch.float32)
    dp = torch.cat([torch.ones_like(d[..., :1]), torch.where(c > 0, (d[..., 1:] * lags) / c, one)], dim=-1)
    i = table[:, 0].long().clamp(1, YIN_LAGS - 3)
    u, cost = table[:, 1], table[:, 2]
    p0, p1, p2, p3 = dp[..., i - 1], dp[..., i], dp[..., i + 1], dp[..., i + 2]
    k3 = 3 * (p1 - p2) + (p3 - p0)
    k2 = 4 * p2 + (-5 * p1 + (2 * p0 - p3))
    v = (0.5 * u) * (u * (u * k3 + k2) + (p2 - p0)) + p1
    s = (1 - v) - cost
    s = torch.where(torch.isfinite(s), s.clamp(0, 1), torch.zeros((), dtype=torch.float32))
    dead = ~torch.isfinite(x).all(dim=-1, keepdim=True)                           # a frame with a sample that is not finite
    return torch.where(dead, torch.zeros((), dtype=torch.float32), s)


def pitch_salience_yin(audio16k: torch.Tensor, hop: int, octave_cost: float = YIN_OCTAVE_COST) -> torch.Tensor:
    """A pitch salience [B, T, 360] on CREPE's bin grid without CREPE: audio16k [B, Lr] at 16 kHz (what `Resample` returns),
    frames of 1024 samples every `hop` (CREPE's own, not normalised), T = 1 + (Lr - 1024) // hop.  Per frame the YIN
    difference function d(tau) = sum_{j < 512} (x[j] - x[j + tau])^2 over tau = 0 .. 511, its cumulative-mean normalisation
    d', and per bin the Catmull-Rom value of d' at the bin's lag 16000 / f_b: salience = clip(1 - d' - octave_cost *
    log2(lag_b / lag_359), 0, 1).  `octave_cost` breaks the tie between a period and its multiples towards the period.  A
    frame with a sample that is not finite, a silent and a constant frame are 0 in every bin.  The decoders (pitch_argmax,
    pitch_weighted, pitch_viterbi + pitch_centered) and pitch_voicing read it as they read CREPE's probabilities; the peak
    value is the periodicity.  DESIGN.md section 10c has the definition and its limits."""
    what = "pitch_salience_yin"
    if audio16k.dim() != 2:
        raise ValueError(f"{what}: audio must be [B, Lr], got {tuple(audio16k.shape)}")
    _refuse_grad(audio16k, what)
    B, Lr = audio16k.shape
    hop = int(hop)
    if Lr < CREPE_WINDOW or hop < 1:
        raise ValueError(f"{what}: needs at least {CREPE_WINDOW} samples and a positive hop, got {Lr} samples and hop {hop}")
    T = 1 + (Lr - CREPE_WINDOW) // hop
    if audio16k.is_cuda:
        y = audio16k.detach().contiguous().float()
        probs = torch.empty((B, T, PITCH_BINS), device=y.device, dtype=torch.float32)
        with torch.cuda.device(y.device):
            rc = _lib.lib().ddsp_yin_salience(y.data_ptr(), _yin_table_on(y.device, octave_cost).data_ptr(), probs.data_ptr(),
                                              B, Lr, hop, T, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_yin_salience")
        return probs
    return _yin_salience_host(audio16k.detach().float(), hop, yin_bin_table(octave_cost))


# ------------------------------------------------------------------------------------------------------------------ voicing
# Definition: DESIGN.md section 10b (include/ddsp_hip.h: ddsp_pitch_voicing).  CUDA tensors take one launch of
# csrc/ddsp_pitch.hip; CPU tensors run the same definition in numpy.

VOICING_WINDOWS = (1, 3, 5, 7, 9)
VOICING_FILLS = ('none', 'hold', 'interpolate')                   # DDSP_VOICING_FILL_*
VOICING_OPTIONS = ('period_window', 'pitch_window', 'upper', 'lower', 'silence', 'fill')


def _lower_median_column(values: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """values, valid [..., K] with the columns in frame order -> the column of each row's lower median: element
    (count - 1) div 2 of the valid entries sorted by value, then by column.  Rows without a valid entry give column 0."""
    K = values.shape[-1]
    column = np.broadcast_to(np.arange(K), values.shape)
    order = np.lexsort((column, ~valid, np.where(valid, values, np.inf)), axis=-1)     # the last key is the primary one
    rank = np.maximum(valid.sum(axis=-1) - 1, 0) // 2
    return np.take_along_axis(order, rank[..., None], axis=-1)[..., 0]


def _voicing_host(f0, n, p, loud, state, period_window, pitch_window, upper, lower, silence, fill):
    """ddsp_pitch_voicing on fp32 numpy rows [B, T] (loud, state may be None; upper, lower, silence np.float32)
    -> (f0, voiced bool, normalized, periodicity, state [B, 3])."""
    B, T = p.shape
    frames = np.arange(T)
    offsets = np.arange(-4, 5)
    window = frames[:, None] + offsets                                         # [T, 9] frame of every window slot
    inside = (window >= 0) & (window < T)
    at = np.clip(window, 0, T - 1)
    # 1. periodicity
    q = np.where(np.isnan(p), np.float32(0), p)
    valid = np.broadcast_to(inside & (np.abs(offsets) <= (period_window - 1) // 2), (B, T, 9))
    pick = _lower_median_column(q[:, at], valid)
    ps = np.take_along_axis(q[:, at], pick[..., None], axis=-1)[..., 0]
    # 2. hysteresis
    v = np.zeros((B, T), dtype=bool)
    now = np.zeros(B, dtype=bool) if state is None else state[:, 0] != 0
    for t in range(T):
        now = np.where(ps[:, t] >= upper, True, np.where(ps[:, t] < lower, False, now))
        v[:, t] = now
    # 3. gate
    m = v & np.isfinite(n)
    if loud is not None:
        with np.errstate(invalid="ignore"):
            m &= loud >= silence
    # 4. voiced pitch: the chosen frame carries both values
    valid = m[:, at] & inside & (np.abs(offsets) <= (pitch_window - 1) // 2) & m[:, :, None]
    pick = _lower_median_column(n[:, at], valid)
    chosen = np.where(m, np.take_along_axis(np.broadcast_to(at, (B, T, 9)), pick[..., None], axis=-1)[..., 0], frames)
    sn = np.take_along_axis(n, chosen, axis=1)
    sf = np.take_along_axis(f0, chosen, axis=1)
    # 5. unvoiced frames.  Column 0 of the extended rows is the state's virtual frame at t = -1.
    virtual = np.zeros(B, dtype=bool) if state is None else ~np.isnan(state[:, 1])
    nan = np.full((B, 1), np.nan, dtype=np.float32)
    en = np.concatenate([nan if state is None else state[:, 1:2], sn], axis=1)
    ef = np.concatenate([nan if state is None else state[:, 2:3], sf], axis=1)
    em = np.concatenate([virtual[:, None], m], axis=1)
    slots = np.arange(T + 1)
    a = np.maximum.accumulate(np.where(em, slots, -1), axis=1)[:, 1:]           # extended column of the voiced frame before, -1: none
    b = np.minimum.accumulate(np.where(m, frames, T)[:, ::-1], axis=1)[:, ::-1]  # frame of the voiced one after, T: none
    has_a, has_b = a >= 0, b < T
    na, fa = np.take_along_axis(en, np.maximum(a, 0), axis=1), np.take_along_axis(ef, np.maximum(a, 0), axis=1)
    nb, fb = np.take_along_axis(sn, np.minimum(b, T - 1), axis=1), np.take_along_axis(sf, np.minimum(b, T - 1), axis=1)
    out_n, out_f = sn.copy(), sf.copy()
    if fill != 'none':
        held = ~m & (has_a | has_b)
        out_n[held] = np.where(has_a, na, nb)[held]
        out_f[held] = np.where(has_a, fa, fb)[held]
    if fill == 'interpolate':
        both = ~m & has_a & has_b
        with np.errstate(all="ignore"):
            w = (frames + 1 - a).astype(np.float32) / (b + 1 - a).astype(np.float32)   # a counts from the virtual frame
            step = (nb - na) * w                                                       # fp32 arrays: every operation rounds
            out_n[both] = (na + step)[both]
        cents = 7180.0 * out_n[both].astype(np.float64) + CENTS_OF_BIN_0
        out_f[both] = np.array([10.0 * 2.0 ** (c / 1200.0) for c in cents.tolist()], dtype=np.float64).astype(np.float32)
    # 6. state
    last = a[:, -1]
    some = last >= 0
    state_out = np.stack([v[:, -1].astype(np.float32),
                          np.where(some, np.take_along_axis(en, np.maximum(last, 0)[:, None], axis=1)[:, 0], np.float32(np.nan)),
                          np.where(some, np.take_along_axis(ef, np.maximum(last, 0)[:, None], axis=1)[:, 0], np.float32(np.nan))], axis=1)
    return out_f, m, out_n, ps, state_out.astype(np.float32)


def pitch_voicing(freq: torch.Tensor, harmonicity: torch.Tensor, normalized_cents: torch.Tensor, loudness=None, *,
                  period_window: int = 3, pitch_window: int = 3, upper: float = 0.31, lower: float = 0.19, silence=None,
                  fill: str = 'hold', state=None, return_state: bool = False):
    """What a CREPE front end does after decoding, on a decoder's outputs [B, T, 1]: the periodicity (`harmonicity`) is
    median-filtered over `period_window` frames and thresholded with hysteresis (voiced from `upper` up, unvoiced below
    `lower`, unchanged in between), frames quieter than `silence` (in LoudnessEncoder's units; None, or no `loudness`: no
    loudness gate) or without a finite pitch are unvoiced as well, a voiced frame takes the decoded (freq, normalized_cents)
    pair of the lower median, by normalized cents, of the voiced frames within `pitch_window`, and an unvoiced frame keeps
    its decoded pitch ('none'), takes the nearest voiced frame's before it, else after it ('hold'), or moves linearly in
    normalized cents between the two ('interpolate', as 'hold' with one side only).  DESIGN.md section 10b has the
    definition to the bit.

    -> (freq, voiced bool, normalized_cents, periodicity), each [B, T, 1]; with a `state` [B, 3] (what a previous call on the
    rows' earlier frames returned: the hysteresis flag and the last voiced pair) or return_state=True, the state is a
    fifth element.  The default thresholds are the conventional hysteresis pair for CREPE periodicity; they are not tuned
    here.  Windows are 1, 3, 5, 7 or 9 frames."""
    what = "pitch_voicing"
    shape = tuple(harmonicity.shape)
    if len(shape) != 3 or shape[-1] != 1 or shape[1] < 1:
        raise ValueError(f"{what}: harmonicity must be [B, T, 1] with T >= 1, got {shape}")
    B, T = shape[:2]
    for name, x in (("freq", freq), ("normalized_cents", normalized_cents), ("loudness", loudness)):
        if x is not None and tuple(x.shape) != shape:
            raise ValueError(f"{what}: {name} must be [B, T, 1] = {shape} as harmonicity, got {tuple(x.shape)}")
    if state is not None and tuple(state.shape) != (B, 3):
        raise ValueError(f"{what}: state must be [B, 3] = {(B, 3)}, got {tuple(state.shape)}")
    if period_window not in VOICING_WINDOWS or pitch_window not in VOICING_WINDOWS:
        raise ValueError(f"{what}: windows must be among {VOICING_WINDOWS}, got {period_window!r} and {pitch_window!r}")
    if fill not in VOICING_FILLS:
        raise ValueError(f"{what}: fill {fill!r}: expected one of {VOICING_FILLS}")
    upper, lower = np.float32(upper), np.float32(lower)
    if not upper >= lower:
        raise ValueError(f"{what}: upper ({upper}) must not be below lower ({lower})")
    inputs = [freq, harmonicity, normalized_cents] + ([loudness] if loudness is not None else [])
    for x in inputs:
        _refuse_grad(x, what)
        if x.device != harmonicity.device:
            raise ValueError(f"{what}: the inputs are on different devices")
    if loudness is None or silence is None:
        loudness, silence = None, np.float32(0)
    silence = np.float32(silence)
    want_state = return_state or state is not None
    if harmonicity.is_cuda:
        dev = harmonicity.device
        f, p, n = (x.detach().contiguous().float() for x in (freq, harmonicity, normalized_cents))
        ld = loudness.detach().contiguous().float() if loudness is not None else None
        if state is not None:
            state = state.detach().to(device=dev, dtype=torch.float32).contiguous()
        L = _lib.lib()
        out = torch.empty((3, B, T, 1), device=dev, dtype=torch.float32)
        voiced = torch.empty((B, T, 1), device=dev, dtype=torch.uint8)
        state_out = torch.empty((B, 3), device=dev, dtype=torch.float32) if want_state else None
        nbytes = L.ddsp_pitch_voicing_workspace_bytes(B, T)
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        with torch.cuda.device(dev):
            rc = L.ddsp_pitch_voicing(f.data_ptr(), n.data_ptr(), p.data_ptr(), ld.data_ptr() if ld is not None else None,
                                      state.data_ptr() if state is not None else None, out[0].data_ptr(), out[1].data_ptr(),
                                      voiced.data_ptr(), out[2].data_ptr(), state_out.data_ptr() if want_state else None,
                                      work.data_ptr() if nbytes else None, B, T, period_window, pitch_window, float(upper),
                                      float(lower), float(silence), VOICING_FILLS.index(fill),
                                      torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_pitch_voicing")
        result = (out[0], voiced.view(torch.bool), out[1], out[2])
        return result + (state_out,) if want_state else result
    rows = [x.detach().float().numpy().reshape(B, T) for x in (freq, normalized_cents, harmonicity)]
    ld = loudness.detach().float().numpy().reshape(B, T) if loudness is not None else None
    st = state.detach().float().cpu().numpy() if state is not None else None
    f, m, n, ps, state_out = _voicing_host(rows[0], rows[1], rows[2], ld, st, period_window, pitch_window, upper, lower, silence, fill)
    result = tuple(torch.from_numpy(np.ascontiguousarray(x)).unsqueeze(-1) for x in (f, m, n, ps))
    return result + (torch.from_numpy(state_out),) if want_state else result


def voicing_options(voicing) -> dict | None:
    """Encoder's `voicing` argument as keyword arguments of pitch_voicing: None / False -> None (off), True -> the defaults,
    a dict -> itself (its keys among VOICING_OPTIONS)."""
    if voicing is None or voicing is False:
        return None
    if voicing is True:
        return {}
    if not isinstance(voicing, dict):
        raise ValueError(f"voicing must be None, a bool or a dict of pitch_voicing's keyword arguments, got {type(voicing).__name__}")
    unknown = sorted(set(voicing) - set(VOICING_OPTIONS))
    if unknown:
        raise ValueError(f"voicing: unknown keys {unknown}; expected some of {VOICING_OPTIONS}")
    return dict(voicing)


def _load_crepe_weights(weights):
    if isinstance(weights, (str, os.PathLike)):
        return torch.load(weights, map_location="cpu", weights_only=True)
    return weights


class F0Encoder(nn.Module):
    """Pitch features of audio at conf.sample_rate: forward(batch [B, L]) -> (freq, harmonicity, probabilities,
    normalized_cents), shapes [B, T, 1], [B, T, 1], [B, T, 360], [B, T, 1].

    The reference loads crepe/pretrained/{capacity}.pth from its own tree; this package ships no weights, so they come from
    `weights` (a path to a CREPE state dict or the dict itself), else from `conf.crepe_weights`.  With neither it raises
    rather than run untrained weights.

    `decoder` (else conf.pitch_decoder, else 'argmax') chooses how the probabilities become a pitch: 'argmax' (the
    reference's forward), 'weighted' (pitch_weighted) or 'viterbi' (pitch_centered around the bins of pitch_viterbi).

    `tracker` (else conf.pitch_tracker, else 'crepe') chooses where the probabilities come from: 'crepe', or 'yin'
    (pitch_salience_yin on the same resampled audio and hop: no weights, no `model` submodule and so no `model.*` state-dict
    keys; `probabilities` is the YIN salience and `harmonicity` its value at the decoded bin).  Unlike CREPE's sigmoid, the
    salience can be 0 in every bin (silence, a constant, some noise frames): 'argmax' then returns bin 0 with harmonicity 0,
    'weighted' and 'viterbi' return NaN as pitch_centered does for any all-zero row; pitch_voicing (`Encoder(voicing=...)`)
    marks such frames unvoiced and fills them."""

    def __init__(self, conf, weights=None, decoder=None, tracker=None):
        super().__init__()
        if tracker is None:
            tracker = getattr(conf, 'pitch_tracker', 'crepe')
        if tracker not in PITCH_TRACKERS:
            raise ValueError(f"pitch tracker {tracker!r}: expected one of {PITCH_TRACKERS}")
        self.tracker = tracker
        if decoder is None:
            decoder = getattr(conf, 'pitch_decoder', 'argmax')
        if decoder not in PITCH_DECODERS:
            raise ValueError(f"pitch decoder {decoder!r}: expected one of {PITCH_DECODERS}")
        self.decoder = decoder
        self.min_cents = self.cents_map(0)
        self.max_cents = self.cents_map(PITCH_BINS - 1)
        self.hop_length = conf.hop_length
        self.window_size = conf.n_fft
        self.rs = Resample(conf.sample_rate, CREPE_RATE)
        self.octave_cost = YIN_OCTAVE_COST
        if tracker == 'crepe':
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

    @staticmethod
    def cents_map(bins):
        return _cents_map(bins)

    def normalize_cents(self, cents):
        return (cents - self.min_cents) / (self.max_cents - self.min_cents)

    @staticmethod
    def freq_map(cents):
        return _freq_map(cents)

    def pitch_argmax(self, probabilities):
        return pitch_argmax(probabilities)

    def pitch_centered(self, center, probabilities):
        return pitch_centered(center, probabilities)

    def pitch_weighted(self, probabilities):
        return pitch_weighted(probabilities)

    def pitch_viterbi(self, probabilities, state=None):
        return pitch_viterbi(probabilities, state)

    def decode(self, probabilities: torch.Tensor):
        """probabilities [B, T, 360] -> (freq, harmonicity, normalized_cents) by this encoder's decoder."""
        if self.decoder == 'viterbi':
            return pitch_centered(pitch_viterbi(probabilities), probabilities)
        return pitch_weighted(probabilities) if self.decoder == 'weighted' else pitch_argmax(probabilities)

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
            if self.tracker == 'yin':
                return self._forward_yin(batch)
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
            if self.decoder != 'argmax':
                freq, harmonicity, normalized_cents = self.decode(probabilities)
                return freq, harmonicity, probabilities, normalized_cents
            bins = probabilities.argmax(dim=-1, keepdim=True)
            freq = 10 * 2 ** ((bins * 20 + 1997.3794084376191) / 1200)
            return freq, probabilities.gather(-1, bins), probabilities, bins / 359.

    def _forward_yin(self, batch: torch.Tensor):
        """Either device: resample, the YIN salience on CREPE's hop grid, this encoder's decoder."""
        if batch.is_cuda:
            batch = batch.contiguous().float()
        with torch.cuda.device(batch.device) if batch.is_cuda else contextlib.nullcontext():
            y = self.rs(batch)
            probabilities = pitch_salience_yin(y, self.resampled_hop(batch.shape[1], y.shape[1]), self.octave_cost)
            freq, harmonicity, normalized_cents = self.decode(probabilities)
        return freq, harmonicity, probabilities, normalized_cents

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
            if self.decoder != 'argmax':
                freq, harmonicity, normalized_cents = self.decode(probs)
                return freq, harmonicity, probs, normalized_cents
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
    """audio [B, L] -> {f0, harmonicity, loudness, probabilities, normalized_cents} (encoder.py:159-177).

    `voicing` (else conf.pitch_voicing, else off): True, or a dict of pitch_voicing's keyword arguments (VOICING_OPTIONS),
    runs pitch_voicing on the decoded pitch with this encoder's own loudness: `f0` and `normalized_cents` are replaced and
    `voiced` (bool [B, T, 1]) is added; `harmonicity` and `probabilities` stay as decoded.  Off, the dict is the reference's.

    `tracker` (else conf.pitch_tracker, else 'crepe') is F0Encoder's: 'yin' needs no weights."""

    def __init__(self, conf, weights=None, voicing=None, tracker=None):
        super().__init__()
        self.conf = conf
        self.f0_encoder = F0Encoder(conf, weights, tracker=tracker)
        self.loudness_encoder = LoudnessEncoder(conf)
        self.voicing = voicing_options(getattr(conf, 'pitch_voicing', None) if voicing is None else voicing)

    def forward(self, x: torch.Tensor) -> dict:
        f0, harmonicity, probabilities, normalized_cents = self.f0_encoder(x)
        loudness = self.loudness_encoder(x)
        out = dict(f0=f0, harmonicity=harmonicity, loudness=loudness, probabilities=probabilities, normalized_cents=normalized_cents)
        if self.voicing is not None:
            out['f0'], out['voiced'], out['normalized_cents'], _ = pitch_voicing(f0, harmonicity, normalized_cents, loudness,
                                                                                 **self.voicing)
        return out


# ------------------------------------------------------------------------------------------------- timbre latent (MFCC -> z)
# DESIGN.md section 10h.  The definition is restated in fp64 as plain loops in tests/mfcc_reference.py.

MFCC_MAX_MELS = 128                      # csrc/ddsp_mfcc.hip: kMaxMels, kMaxMfcc
MFCC_MAX_COEFFS = 64
MFCC_FLOOR = 1e-5                        # -100 dB relative to a full-scale sine


def hann_window(n_fft: int) -> torch.Tensor:
    """Periodic Hann, 0.5 - 0.5 cos(2 pi n / n_fft), in fp64 and rounded to fp32 (what the kernel computes for itself)."""
    n = np.arange(int(n_fft), dtype=np.float64)
    return torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(np.float32))


def _hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_filterbank(n_fft: int, sample_rate: float, n_mels: int = 128, fmin: float = 20.0, fmax: float = 8000.0):
    """HTK-mel triangles with slopes in the mel domain, built in fp64 and rounded to fp32: n_mels + 2 edges equally spaced in
    mel between fmin and min(fmax, sample_rate / 2); bin 0 has weight 0.  -> (dense [n_mels, n_fft / 2 + 1] fp32,
    band_start [n_mels] int32, band_count [n_mels] int32, band_w fp32: every band's contiguous run of non-zero weights, packed
    band after band).  A band that covers no bin has count 0."""
    bins = int(n_fft) // 2 + 1
    top = min(float(fmax), float(sample_rate) / 2.0)
    if not (0.0 <= float(fmin) < top):
        raise ValueError(f"mel_filterbank: need 0 <= fmin < min(fmax, sample_rate / 2), got fmin = {fmin}, fmax = {fmax}, rate {sample_rate}")
    edges = np.linspace(_hz_to_mel(fmin), _hz_to_mel(top), int(n_mels) + 2, dtype=np.float64)
    mel_k = _hz_to_mel(np.arange(bins, dtype=np.float64) * float(sample_rate) / float(n_fft))
    lo, ce, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    dense64 = np.maximum(0.0, np.minimum((mel_k[None] - lo) / (ce - lo), (hi - mel_k[None]) / (hi - ce)))
    dense64[:, 0] = 0.0
    dense = dense64.astype(np.float32)
    start = np.zeros(n_mels, dtype=np.int32)
    count = np.zeros(n_mels, dtype=np.int32)
    packed = []
    for m in range(n_mels):
        nz = np.nonzero(dense[m])[0]
        if nz.size:
            start[m], count[m] = nz[0], nz[-1] - nz[0] + 1
            packed.append(dense[m, nz[0]:nz[-1] + 1])
    band_w = np.concatenate(packed) if packed else np.zeros(0, dtype=np.float32)
    if band_w.size == 0:
        band_w = np.zeros(1, dtype=np.float32)           # (never read: every count is 0; keeps the pointer valid)
    return torch.from_numpy(dense), torch.from_numpy(start), torch.from_numpy(count), torch.from_numpy(band_w.astype(np.float32))


def dct_table(n_mels: int, n_mfcc: int) -> torch.Tensor:
    """D[j, m] = sqrt(2 / n_mels) cos(pi j (m + 1/2) / n_mels) (tf.signal.mfccs_from_log_mel_spectrograms), fp32 from fp64."""
    j = np.arange(int(n_mfcc), dtype=np.float64)[:, None]
    m = np.arange(int(n_mels), dtype=np.float64)[None]
    return torch.from_numpy((np.sqrt(2.0 / n_mels) * np.cos(np.pi * j * (m + 0.5) / n_mels)).astype(np.float32))


def _check_mfcc_sizes(n_fft: int, hop: int, n_mels: int, n_mfcc: int) -> None:
    if n_fft < 64 or n_fft > 2048 or n_fft & (n_fft - 1):
        raise ValueError(f"mfcc: n_fft must be a power of two in 64 .. 2048, got {n_fft}")
    if hop < 1:
        raise ValueError(f"mfcc: hop must be positive, got {hop}")
    if not (1 <= n_mfcc <= n_mels <= MFCC_MAX_MELS) or n_mfcc > MFCC_MAX_COEFFS:
        raise ValueError(f"mfcc: need 1 <= n_mfcc <= n_mels <= {MFCC_MAX_MELS} and n_mfcc <= {MFCC_MAX_COEFFS}, "
                         f"got n_mels = {n_mels}, n_mfcc = {n_mfcc}")


def mfcc_tables(n_fft: int, sample_rate: float, n_mels: int = 128, n_mfcc: int = 30, fmin: float = 20.0, fmax: float = 8000.0) -> dict:
    """Every table of the MFCC definition, on the CPU: window, scale (fp32(2 / sum window)), fbank (dense), band_start,
    band_count, band_w, dct."""
    window = hann_window(n_fft)
    dense, start, count, band_w = mel_filterbank(n_fft, sample_rate, n_mels, fmin, fmax)
    scale = float(np.float32(2.0 / window.double().sum().item()))
    return dict(window=window, scale=scale, fbank=dense, band_start=start, band_count=count, band_w=band_w, dct=dct_table(n_mels, n_mfcc))


_MFCC_TABLES = {}


def _mfcc_tables_on(device, *key) -> dict:
    full = key + (str(device),)
    if full not in _MFCC_TABLES:
        t = mfcc_tables(*key)
        _MFCC_TABLES[full] = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    return _MFCC_TABLES[full]


def _mfcc_run(x: torch.Tensor, t: dict, n_fft: int, hop: int, floor: float, return_logmel: bool):
    """x [B, L] (detached) -> mfcc [B, F, n_mfcc] (and logmel [B, F, n_mels]) with the tables `t` on x's device."""
    if x.dim() != 2:
        raise ValueError(f"mfcc: audio must be [B, L], got {tuple(x.shape)}")
    B, L = x.shape
    if L < n_fft:
        raise ValueError(f"audio of {L} samples is too short for one frame of n_fft = {n_fft}")
    n_mfcc, n_mels = t['dct'].shape
    Fr = 1 + (L - n_fft) // hop
    x = x.detach()
    if x.is_cuda:
        x = x.contiguous().float()
        out = torch.empty((B, Fr, n_mfcc), device=x.device, dtype=torch.float32)
        logmel = torch.empty((B, Fr, n_mels), device=x.device, dtype=torch.float32) if return_logmel else None
        with torch.cuda.device(x.device):
            rc = _lib.lib().ddsp_mfcc(x.data_ptr(), t['band_start'].data_ptr(), t['band_count'].data_ptr(), t['band_w'].data_ptr(),
                                      t['dct'].data_ptr(), out.data_ptr(), None if logmel is None else logmel.data_ptr(), B, L,
                                      n_fft, hop, n_mels, n_mfcc, t['scale'], float(floor), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_mfcc")
        return (out, logmel) if return_logmel else out
    out, logmel = mfcc_torch(x.float(), t, n_fft, hop, floor)
    return (out, logmel) if return_logmel else out


def mfcc_torch(x: torch.Tensor, t: dict, n_fft: int, hop: int, floor: float = MFCC_FLOOR):
    """The MFCC definition as fp32 torch operations on x's device (the CPU path; tools/bench_mfcc.py times it on the GPU):
    framing, window, torch.fft.rfft, magnitude, the dense filterbank and the DCT as two matmuls.  -> (mfcc, logmel)."""
    with torch.no_grad():
        frames = x.unfold(-1, n_fft, hop) * t['window']
        dead = ~torch.isfinite(frames).all(dim=-1, keepdim=True)
        spec = torch.fft.rfft(torch.where(dead, torch.zeros((), dtype=frames.dtype, device=frames.device), frames))
        mel = torch.matmul(spec.abs() * t['scale'], t['fbank'].t())
        logmel = torch.log(mel + floor)
        out = torch.matmul(logmel, t['dct'].t())
        nan = torch.full((), float('nan'), dtype=out.dtype, device=out.device)
        return torch.where(dead, nan, out), torch.where(dead, nan, logmel)


def mfcc(x: torch.Tensor, n_fft: int, hop: int, sample_rate: float, n_mels: int = 128, n_mfcc: int = 30, fmin: float = 20.0,
         fmax: float = 8000.0, floor: float = MFCC_FLOOR, return_logmel: bool = False):
    """Mel-frequency cepstral coefficients of x [B, L] fp32 -> [B, F, n_mfcc] fp32, F = (L - n_fft) // hop + 1 (and, with
    return_logmel, the log-mel spectrogram [B, F, n_mels] as well).  Frame f is x[f hop : f hop + n_fft) as in LoudnessEncoder,
    under a periodic Hann window; magnitudes are scaled by 2 / sum(window), so that a full-scale sine reads 1 and `floor` is
    a level relative to full scale; HTK-mel triangles between fmin and min(fmax, sample_rate / 2); natural log; the DCT-II of
    tf.signal.mfccs_from_log_mel_spectrograms.  n_fft a power of two in 64 .. 2048, 1 <= n_mfcc <= n_mels <= 128, n_mfcc <= 64.
    A frame holding a NaN or an infinite sample is NaN; no other frame is affected.

    CUDA tensors run one HIP launch (ddsp_mfcc); CPU tensors the same definition as fp32 torch operations.  No gradient flows
    to x: the input is detached."""
    n_fft, hop, n_mels, n_mfcc = int(n_fft), int(hop), int(n_mels), int(n_mfcc)
    _check_mfcc_sizes(n_fft, hop, n_mels, n_mfcc)
    t = _mfcc_tables_on(x.device, n_fft, float(sample_rate), n_mels, n_mfcc, float(fmin), float(fmax))
    return _mfcc_run(x, t, n_fft, hop, floor, return_logmel)


class MFCC(nn.Module):
    """`mfcc` with its tables held as buffers (non-persistent: state dicts do not grow).  Reads conf.n_fft, conf.hop_length,
    conf.sample_rate and, where present, z_mels (128), z_mfcc (30), z_fmin (20.0), z_fmax (8000.0).  forward(audio [B, L]) ->
    [B, F, n_mfcc] on LoudnessEncoder's frame grid; the audio is detached (no gradient flows to it)."""

    def __init__(self, conf):
        super().__init__()
        self.n_fft, self.hop_length, self.sample_rate = int(conf.n_fft), int(conf.hop_length), conf.sample_rate
        self.n_mels, self.n_mfcc = int(getattr(conf, 'z_mels', 128)), int(getattr(conf, 'z_mfcc', 30))
        self.fmin, self.fmax = float(getattr(conf, 'z_fmin', 20.0)), float(getattr(conf, 'z_fmax', 8000.0))
        self.floor = MFCC_FLOOR
        _check_mfcc_sizes(self.n_fft, self.hop_length, self.n_mels, self.n_mfcc)
        t = mfcc_tables(self.n_fft, float(self.sample_rate), self.n_mels, self.n_mfcc, self.fmin, self.fmax)
        self.scale = t.pop('scale')
        for name, value in t.items():
            self.register_buffer(name, value, persistent=False)

    def tables(self) -> dict:
        return dict(window=self.window, scale=self.scale, fbank=self.fbank, band_start=self.band_start, band_count=self.band_count,
                    band_w=self.band_w, dct=self.dct)

    def forward(self, audio: torch.Tensor, return_logmel: bool = False):
        return _mfcc_run(audio, self.tables(), self.n_fft, self.hop_length, self.floor, return_logmel)


class ZEncoder(nn.Module):
    """The timbre latent of the DDSP autoencoder: MFCC -> LayerNorm(n_mfcc) -> GRU(n_mfcc, z_gru_units) -> Linear(z_gru_units, z_dims).
    The normalisation is per frame (the original's instance norm runs over time, which has no causal form; this one runs live
    on a one-block window).  conf.z_dims > 0; conf.z_gru_units defaults to 512; the MFCC options are `MFCC`'s.

      forward(audio [B, T hop])          the clip as the dataset stores it, padded (p // 2, p - p // 2) with p = n_fft - hop as
                                         AutoEncoder.forward pads it -> z [B, T, z_dims]
      forward(audio, padded=True)        the audio is padded already
      live(window [B, L], state)         a block whose frames are the window's own (no padding) -> (z, new GRU state)

    Gradients reach the module's parameters, not the audio."""

    def __init__(self, conf):
        super().__init__()
        self.z_dims = int(getattr(conf, 'z_dims', 0) or 0)
        if self.z_dims <= 0:
            raise ValueError("ZEncoder needs conf.z_dims > 0")
        units = int(getattr(conf, 'z_gru_units', 512))
        self.padding = int(conf.n_fft) - int(conf.hop_length)
        self.mfcc = MFCC(conf)
        self.norm = nn.LayerNorm(self.mfcc.n_mfcc)
        self.gru = GRU(self.mfcc.n_mfcc, units, batch_first=True)
        self.out = nn.Linear(units, self.z_dims)

    def _encode(self, audio: torch.Tensor, state):
        h = self.norm(self.mfcc(audio))
        h, state = self.gru(h) if state is None else self.gru(h, state)
        return dense.linear(h, self.out.weight, self.out.bias), state

    def forward(self, audio: torch.Tensor, padded: bool = False) -> torch.Tensor:
        if not padded:
            audio = F.pad(audio, (self.padding // 2, self.padding - self.padding // 2))
        return self._encode(audio, None)[0]

    def live(self, window: torch.Tensor, state=None):
        return self._encode(window, state)
