"""The training set (dataset/audio_dataset.py of the reference): a folder of WAV files -> overlapping examples -> encoder features.

  AudioData     the examples [E, duration] of every file: mono, resampled to conf.sample_rate, hop-padded, unfolded
                (audio_dataset.py:14-68); cached as data_dir/audio_dataset.pth (a tensor)
  PLHDataset    the Encoder's features of every example plus the example itself, the dict {f0, harmonicity, loudness,
                probabilities, normalized_cents, audio} that Decoder and train_step take (audio_dataset.py:71-113); cached as
                data_dir/plh_dataset.pth (a dict of CPU tensors)
  load_audio    restatement of torchaudio.load's file read on scipy.io.wavfile: -> (raw interleaved PCM [L, C], rate)
  example_geometry  the reference's example length and unfold step (audio_dataset.py:50-59)

The caches are the reference's files with the reference's contents, so a cache written by either side loads in the other.

On CUDA everything after the file read runs on the device: the raw PCM crosses PCIe (int16 moves half the bytes of fp32),
ddsp_pcm_to_mono makes it mono fp32, ddsp_resample brings it to conf.sample_rate, and ddsp_make_examples cuts the examples of
all files (hop-pad, unfold, the encoder's margins) in one launch per chunk of rows; only the finished features come back, into
preallocated pinned host tensors.  On CPU the same steps are the reference's stock torch ops (the branch the fixtures pin).

Two departures, both documented choices rather than restatements:
  * files are found with the reference's non-recursive globs (data_dir + '/**/*.wav': exactly one sub-directory level), and
    SORTED -- the reference's order is whatever the file system returns;
  * .mp3 / .ogg files (also in the reference's globs) have no decoder here: they raise a ValueError naming them rather than
    being dropped.  Other WAV sample formats than int16, int32 (24-bit arrives left-justified in int32) and float32 raise too.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from . import _lib
from .encoder import Encoder, Resample, resampled_length

AUDIO_CACHE = 'audio_dataset.pth'
PLH_CACHE = 'plh_dataset.pth'
FEATURES = ('f0', 'harmonicity', 'loudness', 'probabilities', 'normalized_cents')

_PCM_FORMATS = {np.dtype(np.int16): (1, 32768.0), np.dtype(np.int32): (2, 2147483648.0), np.dtype(np.float32): (3, None)}
_TORCH_FORMATS = {torch.int16: 1, torch.int32: 2, torch.float32: 3}
_ROWS_PER_COPY = 256          # AudioData on the device: examples cut and copied back per launch


# ------------------------------------------------------------------------------------------------------------ file reading

def find_audio_files(data_dir: str):
    """The reference's globs (audio_dataset.py:21-23), sorted.  Raises for .mp3 / .ogg files and for an empty folder."""
    others = sorted(glob.glob(data_dir + '/**/*.mp3') + glob.glob(data_dir + '/**/*.ogg'))
    if others:
        raise ValueError(f"no mp3 / ogg decoder in this package; convert these files to WAV: {others}")
    files = sorted(glob.glob(data_dir + '/**/*.wav'))
    if not files:
        raise ValueError('No valid audio files found!')
    return files


def load_audio(path):
    """Restatement of torchaudio.load's read: the WAV file's samples as scipy.io.wavfile returns them, interleaved [L, C]
    (int16, int32 or float32), and the sample rate.  The scaling of torchaudio.load(normalize=True) is pcm_to_float's
    (or, on the device, ddsp_pcm_to_mono's)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.dtype not in _PCM_FORMATS:
        raise ValueError(f"{path}: WAV sample format {data.dtype} is not supported (int16, int32 / 24-bit or float32)")
    if data.ndim == 1:
        data = data[:, None]
    return np.ascontiguousarray(data), int(sr)


def pcm_to_float(pcm: np.ndarray) -> torch.Tensor:
    """[L, C] PCM -> the float32 [C, L] tensor torchaudio.load(normalize=True) returns (int16 / 32768, int32 / 2^31)."""
    scale = _PCM_FORMATS[pcm.dtype][1]
    y = torch.from_numpy(np.ascontiguousarray(pcm.T))
    return y if scale is None else y.float() / scale


def pcm_to_mono(pcm: torch.Tensor) -> torch.Tensor:
    """Device PCM [L, C] (int16 / int32 / float32, as load_audio returns it) -> mono fp32 [L] (ddsp_pcm_to_mono)."""
    if not pcm.is_cuda:
        raise ValueError("pcm_to_mono runs on the device; the CPU restatement is pcm_to_float + mean")
    fmt = _TORCH_FORMATS.get(pcm.dtype)
    if fmt is None or pcm.dim() != 2:
        raise ValueError(f"pcm_to_mono takes [L, C] int16 / int32 / float32, got {tuple(pcm.shape)} {pcm.dtype}")
    pcm = pcm.contiguous()
    L, C = pcm.shape
    y = torch.empty(L, device=pcm.device, dtype=torch.float32)
    with torch.cuda.device(pcm.device):
        rc = _lib.lib().ddsp_pcm_to_mono(pcm.data_ptr(), y.data_ptr(), L, C, fmt, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_pcm_to_mono")
    return y


# ------------------------------------------------------------------------------------------------------------- geometry

def example_geometry(conf):
    """(duration, step) of audio_dataset.py:50-59 exactly: duration = int(example_duration * sr) rounded down to a multiple of
    the hop; step = int(example_overlap * sr) - duration % hop, which subtracts zero, so the step is NOT hop-aligned
    (22 050 at the default Config)."""
    duration = int(conf.example_duration * conf.sample_rate)
    duration -= duration % conf.hop_length
    step = int(conf.example_overlap * conf.sample_rate)
    step -= duration % conf.hop_length
    if duration <= 0 or step <= 0:
        raise ValueError(f"example_duration / example_overlap give duration {duration}, step {step}: both must be positive")
    return duration, step


def hop_pad(length: int, hop: int):
    """audio_dataset.py:46-47: pad = length % hop (NOT a round-up to a multiple of the hop), split (pad // 2, pad - pad // 2)."""
    pad = length % hop
    return pad // 2, pad - pad // 2


def count_examples(path, length: int, conf) -> int:
    """Rows of unfold(0, duration, step) over the hop-padded file; the reference's unfold fails on a shorter file, this names it."""
    duration, step = example_geometry(conf)
    padded = length + sum(hop_pad(length, conf.hop_length))
    if padded < duration:
        raise ValueError(f"{path}: {padded} samples at {conf.sample_rate} Hz (hop-padded) is shorter than one example of "
                         f"{duration} samples")
    return (padded - duration) // step + 1


def make_examples(y: torch.Tensor, files: torch.Tensor, e0: int, E: int, duration: int, step: int, p: int,
                  enc_in: torch.Tensor | None = None, audio: torch.Tensor | None = None) -> None:
    """ddsp_make_examples: rows e0 .. e0 + E - 1 of the files described by `files` ([F, 4] int64 on the device: start in y,
    length, front hop-pad, first example) into enc_in [E, duration + p] and / or audio [E, duration]."""
    for t, w in ((enc_in, duration + p), (audio, duration)):
        if t is not None and (tuple(t.shape) != (E, w) or not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError(f"make_examples: output {tuple(t.shape)} {t.dtype}, expected contiguous float32 {(E, w)}")
    with torch.cuda.device(y.device):
        rc = _lib.lib().ddsp_make_examples(y.data_ptr(), y.numel(), files.data_ptr(), files.shape[0], e0, E, duration, step, p,
                                           None if enc_in is None else enc_in.data_ptr(),
                                           None if audio is None else audio.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_make_examples")


def _device(device):
    if device is None:
        return torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    return torch.device(device)


def _pinned_empty(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, pin_memory=True)


class DeviceAudio:
    """Every file's conf-rate mono audio, concatenated on the device (y), and its table for ddsp_make_examples (files)."""

    def __init__(self, y: torch.Tensor, files: torch.Tensor, n_examples: int, duration: int, step: int):
        self.y, self.files, self.n_examples, self.duration, self.step = y, files, n_examples, duration, step

    @classmethod
    def from_files(cls, paths, conf, device):
        duration, step = example_geometry(conf)
        resamplers, parts, table, start, n = {}, [], [], 0, 0
        with torch.cuda.device(device):
            for path in paths:
                pcm, sr = load_audio(path)
                length = resampled_length(pcm.shape[0], sr, conf.sample_rate)
                count = count_examples(path, length, conf)
                x = torch.from_numpy(pcm).to(device)
                if sr == conf.sample_rate:
                    y = pcm_to_mono(x)
                else:
                    if sr not in resamplers:
                        resamplers[sr] = Resample(sr, conf.sample_rate).to(device)
                    rs = resamplers[sr]
                    y = rs(pcm_to_mono(x).reshape(1, -1))[0].contiguous()      # ddsp_resample, or the stock ops where its table does not fit
                parts.append(y)
                table.append((start, length, hop_pad(length, conf.hop_length)[0], n))
                start += length
                n += count
            y = torch.cat(parts)
        files = torch.tensor(table, dtype=torch.int64).to(device)
        return cls(y, files, n, duration, step)

    @classmethod
    def from_examples(cls, audios: torch.Tensor, device):
        """The cached examples themselves as "files" of one example each (AudioData loaded from its cache)."""
        E, duration = audios.shape
        y = audios.to(device).reshape(-1)
        rows = torch.arange(E, dtype=torch.int64)
        files = torch.stack([rows * duration, torch.full_like(rows, duration), torch.zeros_like(rows), rows], 1).to(device)
        return cls(y, files, E, duration, duration)


# ------------------------------------------------------------------------------------------------------------- datasets

class AudioData(Dataset):
    """audio_dataset.py:14-68: the examples [E, duration] of every WAV file under conf.data_dir, cached in
    data_dir/audio_dataset.pth (loaded instead of rebuilding unless `clear`)."""

    def __init__(self, conf, clear=False, device=None):
        self.device = _device(device)
        self.source = None             # DeviceAudio when built on the device (PLHDataset encodes from it)
        dataset_path = conf.data_dir + '/' + AUDIO_CACHE
        if os.path.exists(dataset_path) and not clear:
            self.audios = torch.load(dataset_path, weights_only=True)
            return
        files = find_audio_files(conf.data_dir)
        if self.device.type == 'cuda':
            self.audios = self._build_device(files, conf)
        else:
            self.audios = self._build_cpu(files, conf)
        torch.save(self.audios, dataset_path)

    @staticmethod
    def _build_cpu(files, conf):
        duration, step = example_geometry(conf)
        audios = []
        for f in files:
            pcm, sr = load_audio(f)
            y = pcm_to_float(pcm)
            y = y[0] if y.shape[0] == 1 else y.mean(dim=0)
            y = Resample(sr, conf.sample_rate)(y[None])[0]
            count_examples(f, len(y), conf)
            y = F.pad(y, hop_pad(len(y), conf.hop_length))
            audios.append(y.unfold(0, duration, step))
        return torch.cat(audios)

    def _build_device(self, files, conf):
        src = DeviceAudio.from_files(files, conf, self.device)
        self.source = src
        out = _pinned_empty((src.n_examples, src.duration))
        with torch.cuda.device(self.device):
            for e0 in range(0, src.n_examples, _ROWS_PER_COPY):
                E = min(_ROWS_PER_COPY, src.n_examples - e0)
                rows = torch.empty((E, src.duration), device=self.device, dtype=torch.float32)
                make_examples(src.y, src.files, e0, E, src.duration, src.step, 0, audio=rows)
                out[e0:e0 + E].copy_(rows, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return out

    def __getitem__(self, index):
        return self.audios[index]

    def __len__(self):
        return self.audios.shape[0]


class PLHDataset(Dataset):
    """audio_dataset.py:71-113: the Encoder's features of every AudioData example and the example itself,
    {f0, harmonicity, loudness, probabilities, normalized_cents, audio}, cached in data_dir/plh_dataset.pth.

    `weights`: CREPE weights (a path or state dict), else conf.crepe_weights (as F0Encoder takes them).  `encode_batch`: examples
    per encoder call (default conf.batch_size, the reference's DataLoader batch).

    With conf.pitch_voicing set, `f0` and `normalized_cents` are the gated ones (Encoder's `voicing`); `voiced` is not
    stored.  With conf.pitch_tracker = 'yin' the pitch features come from pitch_salience_yin and no weights are needed.  The
    cache file records none of these settings, nor conf.pitch_decoder: pass `clear` after changing one."""

    def __init__(self, conf, clear=False, weights=None, device=None, encode_batch=None):
        self.device = _device(device)
        dataset_path = conf.data_dir + '/' + PLH_CACHE
        if os.path.exists(dataset_path) and not clear:
            self.final = torch.load(dataset_path, weights_only=True)
            return
        audios = AudioData(conf, clear, device=self.device)
        encoder = Encoder(conf, weights).to(self.device).eval()
        padding = conf.n_fft - conf.hop_length
        rows = int(encode_batch or conf.batch_size)
        if rows <= 0:
            raise ValueError(f"encode_batch must be positive, got {rows}")
        if self.device.type == 'cuda':
            self.final = self._build_device(audios, encoder, padding, rows)
        else:
            self.final = self._build_cpu(audios, encoder, padding, rows)
        torch.save(self.final, dataset_path)

    @staticmethod
    def _build_cpu(audios, encoder, padding, rows):
        pls = []
        for e0 in range(0, len(audios), rows):
            batch = audios.audios[e0:e0 + rows]
            data = encoder(F.pad(batch, (padding // 2, padding - padding // 2)))
            pls.append(data)
        final = {key: torch.cat([d[key] for d in pls], dim=0) for key in FEATURES}
        final['audio'] = audios.audios
        return final

    def _build_device(self, audios, encoder, padding, rows):
        src = audios.source if audios.source is not None else DeviceAudio.from_examples(audios.audios, self.device)
        E, duration = src.n_examples, src.duration
        final = {}
        with torch.cuda.device(self.device):
            for e0 in range(0, E, rows):
                n = min(rows, E - e0)
                enc_in = torch.empty((n, duration + padding), device=self.device, dtype=torch.float32)
                make_examples(src.y, src.files, e0, n, duration, src.step, padding, enc_in=enc_in)
                data = encoder(enc_in)
                if not final:
                    final = {k: _pinned_empty((E,) + tuple(data[k].shape[1:])) for k in FEATURES}
                for k in FEATURES:
                    final[k][e0:e0 + n].copy_(data[k], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        final['audio'] = audios.audios
        return final

    def __getitem__(self, index):
        return {key: val[index] for key, val in self.final.items()}

    def __len__(self):
        return len(self.final['f0'])
