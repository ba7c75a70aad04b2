"""Spectral style transfer: the reference's style_transfer.py (with helper.py's variant behind film_ui.py) as functions that
take audio arrays.  A random 1-D convolution (FeatureExtractor) turns a log-magnitude spectrogram into features; LBFGS moves
the content's spectrogram towards the content's features and the style's Gram matrix; Griffin-Lim (ddsp_pytorch_amd.griffinlim,
HIP on the device) turns the result back into audio.

The convolution and the Gram GEMM stay on MIOpen / rocBLAS through torch, as CREPE's layers do; the new HIP of
this part is Griffin-Lim.
"""
from __future__ import annotations

import time
from typing import Optional, Union

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F  # noqa: N812

from .spectral import griffinlim

__all__ = ["normalize_audio", "prepare_spectra", "gram_matrix", "FeatureExtractor", "ContentLoss", "StyleLoss", "style_transfer"]


def normalize_audio(x):
    """Remove the DC offset, then scale to a peak of 1 (style_transfer.py:19-25).  numpy arrays and tensors alike."""
    x = x - x.mean()
    peak = np.max(np.abs(x)) if isinstance(x, np.ndarray) else x.abs().max()
    return x / peak


def _periodic_hann(n: int) -> np.ndarray:
    """scipy.signal.get_window('hann', n, fftbins=True) in float64 (what librosa 0.8.1's stft windows with): the symmetric
    (n + 1)-point cosine sum 0.5 + 0.5 cos(linspace(-pi, pi, n + 1)), last point dropped."""
    fac = np.linspace(-np.pi, np.pi, n + 1)
    w = np.zeros(n + 1)
    for k, a in enumerate((0.5, 0.5)):
        w += a * np.cos(k * fac)
    return w[:-1]


def _stft_librosa(y: np.ndarray, n_fft: int, hop_length: int) -> np.ndarray:
    """librosa 0.8.1 stft(y, n_fft, hop_length) with its defaults: win_length = n_fft, periodic Hann, center=True with reflect
    padding, each windowed frame's rfft in float64 stored as complex64.  [1 + n_fft // 2, frames]."""
    window = _periodic_hann(n_fft)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    n_frames = 1 + (len(yp) - n_fft) // hop_length
    frames = np.lib.stride_tricks.as_strided(yp, shape=(n_frames, n_fft), strides=(yp.strides[0] * hop_length, yp.strides[0]))
    out = np.empty((1 + n_fft // 2, n_frames), dtype=np.complex64, order="F")
    out[...] = np.fft.rfft(window[None, :] * frames, axis=-1).T
    return out


def prepare_spectra(audio: Union[np.ndarray, torch.Tensor], sample_rate: int, win_length: int, hop_length: int):
    """(log1p |STFT|  [1 + win_length // 2, frames] float32, number of samples) of mono audio at `sample_rate`, normalised
    first (style_transfer.py:28-36).  Takes the samples rather than a path: the reference's librosa.load (resampy resampling,
    any format) is not available here; read a file with `ddsp_pytorch_amd.load_audio` and bring it to `sample_rate` with
    `ddsp_pytorch_amd.encoder.Resample`.  `sample_rate` is the audio's rate (kept for the reference's signature)."""
    if isinstance(audio, torch.Tensor):
        audio = audio.detach().cpu().numpy()
    audio = np.asarray(audio, dtype=np.float32)
    if audio.ndim != 1:
        raise ValueError(f"prepare_spectra takes mono audio [L], got shape {audio.shape}")
    if audio.shape[0] <= win_length // 2:
        raise ValueError(f"{audio.shape[0]} samples are too short for the reflect padding of {win_length // 2}")
    audio = normalize_audio(audio)
    mag = np.abs(_stft_librosa(audio, win_length, hop_length))
    return np.log1p(mag), len(audio)


def gram_matrix(x: torch.Tensor) -> torch.Tensor:
    """[batch, channels, frames] -> the [batch * channels]^2 Gram matrix over frames, divided by the element count."""
    batch, channels, frames = x.size()
    features = x.view(batch * channels, frames)
    return torch.mm(features, features.t()).div(batch * channels * frames)


class ContentLoss(nn.Module):
    """Identity that records `loss` = mse(x, target) (style_transfer.py:39-46)."""

    def __init__(self, target: torch.Tensor):
        super().__init__()
        self.target = target.detach()

    def forward(self, x):
        self.loss = F.mse_loss(x, self.target)
        return x


class StyleLoss(nn.Module):
    """Identity that records `loss` = mse(gram(x), gram(target)) (style_transfer.py:57-65)."""

    def __init__(self, target_feature: torch.Tensor):
        super().__init__()
        self.target = gram_matrix(target_feature).detach()

    def forward(self, x):
        self.loss = F.mse_loss(gram_matrix(x), self.target)
        return x


class FeatureExtractor(nn.Module):
    """relu(conv1d(zero-pad(x), conv_kernel)) with a fixed random kernel [out_ch, in_ch, size] drawn from torch's global RNG as
    randn * sqrt(2) * sqrt(2 / ((in_ch + out_ch) size)) (style_transfer.py:68-81)."""

    def __init__(self, in_ch: int, out_ch: int, size: int):
        super().__init__()
        self.padding = (size - 1) // 2
        std = np.sqrt(2) * np.sqrt(2 / ((in_ch + out_ch) * size))
        self.register_buffer('conv_kernel', torch.randn(out_ch, in_ch, size) * std)

    def forward(self, x):
        return F.relu(F.conv1d(F.pad(x, (self.padding, self.padding)), self.conv_kernel))


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def style_transfer(content, style, sample_rate: int = 44100, win_length: int = 2048, hop_length: int = 256,
                   n_features: int = 4096, kernel_size: int = 17, alpha: float = 1, beta: float = 1e13, lr: float = 1,
                   max_iter: int = 1000, gl_iter: int = 5000, momentum: float = 0.99, length: Optional[Union[str, int]] = 'content',
                   device=None, *, generator: Optional[torch.Generator] = None, stats: Optional[dict] = None) -> np.ndarray:
    """The steps of style_transfer.py's main() on two mono clips at `sample_rate`; returns the normalised audio (float32).

    The spectra are normalised with the content's mean and deviation; both are trimmed to the shorter one's frame count, the
    style from frame T_style // 8 over four times that many frames; LBFGS (lr, max_iter) minimises
    beta * style loss + alpha * content loss over the content spectrum; the result is un-normalised, exp - 1, and inverted by
    Griffin-Lim (gl_iter iterations, momentum, a random start from `generator` or torch's global generator).
    `length='content'` asks Griffin-Lim for the content's sample count, as main() does (a ValueError when the style clip is
    the shorter one: its frame count no longer matches); `length=None` is helper.py's variant (hop * (frames - 1) samples).
    `stats`, if given, receives the closure losses ('losses') and the seconds spent in LBFGS and Griffin-Lim."""
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    device = torch.device(device)
    content_db, content_length = prepare_spectra(content, sample_rate, win_length, hop_length)
    style_db, _ = prepare_spectra(style, sample_rate, win_length, hop_length)

    elem_mean = np.mean(content_db)
    elem_std = np.std(content_db)
    content_db = (content_db - elem_mean) / elem_std
    style_db = (style_db - elem_mean) / elem_std
    frames = min(content_db.shape[1], style_db.shape[1])
    offset = style_db.shape[1] // 8
    content_db, style_db = content_db[:, :frames], style_db[:, offset:offset + frames * 4]

    x = torch.from_numpy(np.ascontiguousarray(content_db)).unsqueeze(0).to(device)
    s = torch.from_numpy(np.ascontiguousarray(style_db)).unsqueeze(0).to(device)
    net = nn.Sequential(FeatureExtractor(content_db.shape[0], n_features, kernel_size).to(device))
    with torch.no_grad():
        content_features = net(x)
        style_features = net(s)
    net.add_module('content_loss', ContentLoss(content_features))
    net.add_module('style_loss', StyleLoss(style_features))
    del s, style_features

    optimizer = torch.optim.LBFGS([x.requires_grad_()], lr=lr, max_iter=max_iter)
    losses = []

    def closure():
        optimizer.zero_grad()
        net(x)
        loss = beta * net.style_loss.loss + alpha * net.content_loss.loss
        loss.backward()
        losses.append(loss.detach())
        return loss

    _sync(device)
    t0 = time.perf_counter()
    optimizer.step(closure)
    _sync(device)
    t1 = time.perf_counter()
    del net, optimizer

    with torch.no_grad():
        x = x.detach() * elem_std + elem_mean
        result = torch.exp(x) - 1
        gl_length = content_length if length == 'content' else length
        y = griffinlim(result, window=torch.hann_window(win_length, True).to(device), n_fft=win_length, hop_length=hop_length,
                       win_length=win_length, power=1, n_iter=gl_iter, momentum=momentum, length=gl_length, rand_init=True,
                       generator=generator)
        y = y.cpu().numpy()[0]
    t2 = time.perf_counter()
    if stats is not None:
        stats["losses"] = [float(v) for v in losses]
        stats["lbfgs_s"] = t1 - t0
        stats["griffinlim_s"] = t2 - t1
    return normalize_audio(y)
