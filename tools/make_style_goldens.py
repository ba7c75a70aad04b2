#!/usr/bin/env python3
"""Generate the style-transfer fixtures tests/golden/g28_* by running the REFERENCE's own style_transfer.py on the CPU.

Needs a checkout of the reference (read-only): $DDSP_REFERENCE, default ../reference next to this repository.  librosa,
torchaudio and soundfile are not installed; style_transfer.py imports them, so three stub modules stand in, each labelled:
  * librosa.load(path, sr, mono) -> (the float32 samples handed in as `path`, sr)   (a harness setting: inputs are arrays)
  * librosa.stft                 -> RESTATEMENT of librosa 0.8.1's stft with its defaults: scipy.signal.get_window('hann',
                                    n_fft, fftbins=True), center=True with np.pad(mode='reflect'), frames hop apart, numpy's
                                    rfft of window * frames along axis 0 (float64) stored into a complex64 F-ordered matrix
  * torchaudio.functional.griffinlim -> tools/make_griffinlim_goldens.py's restatement of torchaudio 0.8.1
  * soundfile.write              -> not called
Everything else -- normalize_audio, prepare_spectra, gram_matrix, FeatureExtractor's seeded draw, ContentLoss, StyleLoss --
is the reference's code running; the glue of main() (normalisation, trimming, network, LBFGS closure) is restated step by step
below on the reference's classes, with 1 s / 2 s clips, 256 features and max_iter = 3.

Recorded: the two clips; the spectra of both, the normalisation statistics and the trim; a seeded FeatureExtractor's kernel
and output; the Gram matrices and both losses; the closure losses and the content spectrum after the LBFGS step; and main()'s
Griffin-Lim end on that spectrum (GL_ITER iterations from a start seeded with torch.manual_seed(GL_SEED), normalised).  The
clips, losses and statistics are stored as they are; every other array, which the tests compare bit for bit, as its SHA-256
with its shape, dtype, sum and largest magnitude (`<name>_sha256`, `_shape`, `_dtype`, `_sum`, `_absmax`): the arrays
themselves would make the fixture several megabytes.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_style_goldens.py
"""
import hashlib
import os
import sys
import types

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DDSP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import scipy.signal  # noqa: E402
import torch  # noqa: E402

from make_griffinlim_goldens import griffinlim_081  # noqa: E402

torch.backends.mkldnn.enabled = False          # CPU convolutions on the native path (the tests pin the same)
OUT = os.path.join(ROOT, "tests", "golden")
SR, WIN, HOP, FEATURES, KSIZE = 44100, 2048, 256, 256, 17
GL_ITER, GL_SEED = 16, 4


def digest(out, name, a):
    """Record array `a` as its SHA-256 (of the C-ordered bytes) plus shape, dtype, sum and largest magnitude."""
    a = np.ascontiguousarray(a)
    out[name + "_sha256"] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
    out[name + "_shape"] = np.array(a.shape, dtype=np.int64)
    out[name + "_dtype"] = np.array(a.dtype.str)
    out[name + "_sum"] = np.float64(a.astype(np.float64).sum())
    out[name + "_absmax"] = np.float64(np.abs(a).max())


# ---- stubs --------------------------------------------------------------------------------------------------------------
def _librosa_stft(y, n_fft=2048, hop_length=None, win_length=None, window='hann', center=True, dtype=np.complex64,
                  pad_mode='reflect'):
    """RESTATEMENT of librosa 0.8.1 core.stft (win_length = n_fft, no window padding needed)."""
    hop_length = hop_length or n_fft // 4
    fft_window = scipy.signal.get_window(window, win_length or n_fft, fftbins=True).reshape((-1, 1))
    if center:
        y = np.pad(y, int(n_fft // 2), mode=pad_mode)
    n_frames = 1 + (len(y) - n_fft) // hop_length
    y_frames = np.lib.stride_tricks.as_strided(y, shape=(n_fft, n_frames), strides=(y.strides[0], y.strides[0] * hop_length))
    stft_matrix = np.empty((int(1 + n_fft // 2), n_frames), dtype=dtype, order='F')
    stft_matrix[:, :] = np.fft.rfft(fft_window * y_frames, axis=0)
    return stft_matrix


def _install_stubs():
    librosa = types.ModuleType("librosa")
    librosa.load = lambda path, sr=22050, mono=True: (np.asarray(path, dtype=np.float32), sr)
    librosa.stft = _librosa_stft
    torchaudio = types.ModuleType("torchaudio")
    torchaudio.functional = types.SimpleNamespace(griffinlim=griffinlim_081)
    soundfile = types.ModuleType("soundfile")

    def _no_write(*a, **k):
        raise RuntimeError("soundfile.write is not part of the fixtures")
    soundfile.write = _no_write
    sys.modules.update(librosa=librosa, torchaudio=torchaudio, soundfile=soundfile)


def clips():
    """A 1 s harmonic content clip and a 2 s noisy, decaying style clip (float32, 44.1 kHz)."""
    rng = np.random.default_rng(2800)
    t = np.arange(SR) / SR
    content = sum(0.4 / h * np.sin(2 * np.pi * 196.0 * h * t + rng.uniform(0, 6.28)) for h in range(1, 12))
    content = content * (0.6 + 0.4 * np.sin(2 * np.pi * 2 * t)) + 0.01 * rng.standard_normal(t.size)
    ts = np.arange(2 * SR) / SR
    style = rng.standard_normal(ts.size) * np.exp(-(ts % 0.25) * 12) + 0.3 * np.sin(2 * np.pi * 523.25 * ts)
    return content.astype(np.float32), style.astype(np.float32)


def main():
    _install_stubs()
    import style_transfer as ref          # the reference's module, on the stubs above

    torch.set_num_threads(1)
    content_audio, style_audio = clips()
    out = {"content_audio": content_audio, "style_audio": style_audio,
           "params": np.array([SR, WIN, HOP, FEATURES, KSIZE], dtype=np.int64)}
    content, content_length = ref.prepare_spectra(content_audio, SR, WIN, HOP)
    style, _ = ref.prepare_spectra(style_audio, SR, WIN, HOP)
    digest(out, "content_db", content)
    digest(out, "style_db", style)
    out["content_length"] = np.int64(content_length)

    # main(), restated on the reference's classes (style_transfer.py:89-137), CPU, FEATURES features, max_iter = 3
    elem_mean = np.mean(content)
    elem_std = np.std(content)
    content = (content - elem_mean) / elem_std
    style = (style - elem_mean) / elem_std
    length = min(content.shape[1], style.shape[1])
    offset = style.shape[1] // 8
    content, style = content[:, :length], style[:, offset:offset + length * 4]
    out.update(trim=np.array([length, offset], dtype=np.int64), elem_mean=np.float64(elem_mean), elem_std=np.float64(elem_std))
    content = torch.from_numpy(np.ascontiguousarray(content)).unsqueeze(0)
    style = torch.from_numpy(np.ascontiguousarray(style)).unsqueeze(0)

    torch.manual_seed(28)
    net = torch.nn.Sequential(ref.FeatureExtractor(content.shape[1], FEATURES, KSIZE))
    with torch.no_grad():
        content_features = net(content)
        style_features = net(style)
    digest(out, "conv_kernel", net[0].conv_kernel.numpy())
    digest(out, "content_features", content_features.numpy())
    digest(out, "style_features", style_features.numpy())
    content_loss = ref.ContentLoss(content_features)
    net.add_module('content_loss', content_loss)
    style_loss = ref.StyleLoss(style_features)
    net.add_module('style_loss', style_loss)
    digest(out, "gram_content", ref.gram_matrix(content_features).numpy())
    digest(out, "gram_style", style_loss.target.numpy())
    with torch.no_grad():
        net(content)
    out.update(style_loss0=np.float64(net.style_loss.loss), content_loss0=np.float64(net.content_loss.loss))

    alpha, beta, lr, max_iter = 1, 1e13, 1, 3
    optimizer = torch.optim.LBFGS([content.requires_grad_()], lr=lr, max_iter=max_iter)
    losses = []

    def closure():
        optimizer.zero_grad()
        net(content)
        loss = beta * net.style_loss.loss + alpha * net.content_loss.loss
        loss.backward()
        losses.append(float(loss.detach()))
        return loss

    optimizer.step(closure)
    out["lbfgs_losses"] = np.array(losses, dtype=np.float64)
    digest(out, "content_after", content.detach().numpy())

    # main()'s end (style_transfer.py:146-162) on the stubbed torchaudio, GL_ITER iterations
    with torch.no_grad():
        result = torch.exp(content * elem_std + elem_mean) - 1
        torch.manual_seed(GL_SEED)
        result = sys.modules["torchaudio"].functional.griffinlim(result, window=torch.hann_window(WIN, True), n_fft=WIN,
                                                                hop_length=HOP, win_length=WIN, power=1, n_iter=GL_ITER,
                                                                momentum=0.99, length=content_length, rand_init=True)
    digest(out, "result", ref.normalize_audio(result.numpy()[0]))
    out["gl"] = np.array([GL_ITER, GL_SEED], dtype=np.int64)
    path = os.path.join(OUT, "g28_style.npz")
    np.savez_compressed(path, **out)
    print(path, "losses", losses)


if __name__ == "__main__":
    sys.exit(main())
