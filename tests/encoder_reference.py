"""TEST INFRASTRUCTURE ONLY -- plain fp64 references of the audio encoder's HIP stages (csrc/ddsp_encoder.hip, csrc/ddsp_loudness.hip)
and the seeded inputs the host and the GPU tests share.  No device code; nothing under ddsp-pytorch_amd/ may import this module.

  loudness_ref    per frame: fp64 rfft -> abs -> (20 log10(|X| + 1e-20) + a_weight) / 90 + 1 -> mean over the bins
  resample_ref    the fp64 polyphase sum with the full fp32-stored kernel of sinc_resample_kernel (every tap, torchaudio's padding
                  (width, width + orig'), cut to resampled_length), at every output or at given positions only
  row_stats_ref   fp64 mean and unbiased std of each row
  frames_fp32     (y - mean) / std in numpy float32 from GIVEN fp32 stats, each frame at columns 254 .. 1277 of 1532, zero margins:
                  one subtraction and one correctly rounded division per element, the expression crepe_frames_kernel evaluates
  decode_ref      fp64 sigmoid of the fp32 sum logits + bias

Inputs are broadband (Gaussian noise, or tones plus noise): a spectrum bin that is empty up to rounding has an ill-conditioned
logarithm in any fp32 implementation and says nothing about a kernel.  tests/test_encoder_reference_host.py holds the stock fp32
CPU branch to 1e-6 (loudness) and 5e-7 (resampler) of these references on exactly these inputs, which is what makes the GPU
tolerances (2e-6, 1e-6) fair.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ddsp_pytorch_amd.encoder import a_weighting, resampled_length, sinc_resample_kernel

LOUDNESS_SIZES = (64, 128, 256, 512, 1024, 2048)
LOUDNESS_TOL = 2e-6
RESAMPLE_TOL = 1e-6
STOCK_LOUDNESS_TOL = 1e-6        # the stock fp32 CPU branch against loudness_ref on the inputs below
STOCK_RESAMPLE_TOL = 5e-7
RATES_TO_16K = (44100, 48000, 22050, 32000, 96000, 8000, 11025, 12000)
RATES_TO_44K = (16000, 48000)
RATE_PAIRS = tuple((r, 16000) for r in RATES_TO_16K) + tuple((r, 44100) for r in RATES_TO_44K)
LONG_PAIR, LONG_LENGTH = (8000, 16000), 8_500_001       # 17 000 002 outputs: past the resampler grid's 16384 x 1024
PAD, WIN = 254, 1024


# ---------------------------------------------------------------------------------------------------------------- references

def a_weight_of(n_fft: int, sample_rate: int = 16000) -> np.ndarray:
    """LoudnessEncoder's parameter: float64 [n_fft / 2 + 1]."""
    return a_weighting(np.linspace(0, float(sample_rate) / 2, 1 + n_fft // 2, endpoint=True, dtype='float32'))


def loudness_ref(x, n_fft: int, hop: int, a_weight) -> np.ndarray:
    """x [B, L] -> [B, F] float64, F = 1 + (L - n_fft) // hop.  A frame with a sample that is not finite is NaN (what the stock
    path gives: every bin of its transform is NaN)."""
    x = np.asarray(x, dtype=np.float64)
    B, L = x.shape
    F = 1 + (L - n_fft) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None]
    frames = x[:, idx]                                                           # [B, F, n_fft]
    dead = ~np.isfinite(frames).all(axis=-1)
    mag = np.abs(np.fft.rfft(np.where(dead[..., None], 0.0, frames), axis=-1))
    db = (20.0 * np.log10(mag + 1e-20) + np.asarray(a_weight, dtype=np.float64)) / 90.0 + 1.0
    return np.where(dead, np.nan, db.mean(axis=-1))


def resample_ref(x, orig: int, new: int, positions=None) -> np.ndarray:
    """x [B, L] -> [B, resampled_length] float64, or [B, len(positions)] at the given output positions."""
    kernel, width, o, n = sinc_resample_kernel(orig, new)
    k = kernel[:, 0].numpy().astype(np.float64)                                  # [n, 2 width + o]: the fp32-stored taps
    x = np.asarray(x, dtype=np.float64)
    B, L = x.shape
    target = resampled_length(L, orig, new)
    j = np.arange(target) if positions is None else np.asarray(positions, dtype=np.int64)
    assert j.size == 0 or (j.min() >= 0 and j.max() < target)
    xp = np.pad(x, ((0, 0), (width, width + o)))
    taps = np.arange(k.shape[1])
    out = np.empty((B, j.size))
    for lo in range(0, j.size, 2048):
        jj = j[lo:lo + 2048]
        win = xp[:, (jj // n)[:, None] * o + taps[None]]                         # [B, J, W]
        out[:, lo:lo + 2048] = (win * k[jj % n][None]).sum(axis=-1)
    return out


def row_stats_ref(y) -> np.ndarray:
    """y [B, N] -> [B, 2] float64: mean, unbiased std."""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([y.mean(axis=1), y.std(axis=1, ddof=1)], axis=1)


def frames_fp32(y, stats, hop: int, T: int) -> np.ndarray:
    """y [B, Lr] fp32, stats [B, 2] fp32 (mean, std) -> [B * T, 1532] fp32."""
    y = np.asarray(y, dtype=np.float32)
    stats = np.asarray(stats, dtype=np.float32)
    B = y.shape[0]
    idx = np.arange(T)[:, None] * hop + np.arange(WIN)[None]
    out = np.zeros((B, T, WIN + 2 * PAD), dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, :, PAD:PAD + WIN] = (y[:, idx] - stats[:, 0, None, None]) / stats[:, 1, None, None]
    return out.reshape(B * T, WIN + 2 * PAD)


def decode_ref(logits, bias) -> np.ndarray:
    """[N, 360] fp32, [360] fp32 -> fp64 probabilities."""
    z = (np.asarray(logits, dtype=np.float32) + np.asarray(bias, dtype=np.float32)[None]).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


# ------------------------------------------------------------------------------------------------------- stock fp32 branches

class _Conf:
    def __init__(self, sample_rate, n_fft, hop_length):
        self.sample_rate, self.n_fft, self.hop_length = sample_rate, n_fft, hop_length


def loudness_encoder(n_fft: int, hop: int):
    import ddsp_pytorch_amd as ddsp
    return ddsp.LoudnessEncoder(_Conf(16000, n_fft, hop))


# --------------------------------------------------------------------------------------------------------------------- inputs

QUIET = (1e-2, 1e-4, 1e-6)

# per-frame levels of the three rows (9 frames; the 8-frame form drops the last).  Frames 2q and 2q + 1 share a transform:
# row 0 has its quiet frames in slot a, row 1 in slot b, row 2 has pairs that are quiet in both slots.
_STEP_LEVELS = np.array([
    [1e-2, 1.0, 1e-4, 1.0, 1e-6, 1.0, 1.0, 1.0, 1e-4],
    [1.0, 1e-2, 1.0, 1e-4, 1.0, 1e-6, 1.0, 1.0, 1.0],
    [1e-2, 1e-2, 1e-4, 1e-4, 1e-6, 1e-4, 1.0, 1e-6, 1e-6],
])
_ZERO_LEVELS = np.array([
    [0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0],
    [1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0],
    [0.0, 0.0, 1.0, 1e-4, 0.0, 1e-4, 1e-4, 0.0, 1.0],
])


def pair_ratio(levels: np.ndarray) -> np.ndarray:
    """levels [B, F] -> each frame's level over its pair partner's (frames 2q, 2q + 1 of a row), capped at 1; a row's odd last
    frame has no partner (1), a zero frame beside a louder one is 0."""
    B, F = levels.shape
    ratio = np.ones((B, F))
    for f in range(F):
        partner = f ^ 1
        if partner < F:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(levels[:, partner] > 0, levels[:, f] / levels[:, partner], 1.0)
            ratio[:, f] = np.minimum(r, 1.0)
    return ratio


def _level_rows(n_fft, levels, rng):
    B, F = levels.shape
    x = 0.3 * rng.standard_normal((B, F, n_fft)) * levels[:, :, None]
    return x.reshape(B, F * n_fft).astype(np.float32)


def loudness_cases(n_fft: int, seed: int = 0):
    """-> list of dicts {name, x [3, L] fp32, hop, levels [3, F] or None, nan_frames bool [3, F] or None}."""
    rng = np.random.default_rng([n_fft, seed, 19])
    cases = []
    for F in (9, 8):
        cases.append(dict(name=f"steps{F}", x=_level_rows(n_fft, _STEP_LEVELS[:, :F], rng), hop=n_fft, levels=_STEP_LEVELS[:, :F]))
    cases.append(dict(name="zeros9", x=_level_rows(n_fft, _ZERO_LEVELS, rng), hop=n_fft, levels=_ZERO_LEVELS))
    cases.append(dict(name="zeros8", x=_level_rows(n_fft, _ZERO_LEVELS[:, :8], rng), hop=n_fft, levels=_ZERO_LEVELS[:, :8]))
    one = np.array([[1.0], [1e-4], [0.0]])
    cases.append(dict(name="one_frame", x=_level_rows(n_fft, one, rng), hop=n_fft, levels=one))
    # overlapped frames, and the unaligned loads of the 2048 kernel: an onset after >= n_fft + hop zeros, and a decay into zeros
    hop = n_fft // 4 + 3
    L = n_fft + 8 * hop + 2
    x = 0.3 * rng.standard_normal((3, L))
    x[0, :n_fft + hop + 5] = 0.0
    x[1, :n_fft + 2 * hop + 1] = 0.0
    x[2, 3 * hop:] = 0.0
    cases.append(dict(name="overlap_onset", x=x.astype(np.float32), hop=hop, levels=None))
    # one NaN sample (row 0) and one +Inf sample (row 1); hop n_fft / 2: each lies in two frames that straddle a pair boundary
    # (frames 1, 2 and 5, 6: slot b of one pair and slot a of the next), so both have a live partner (frames 0, 3 and 4, 7)
    hop = n_fft // 2
    L = n_fft + 7 * hop
    x = (0.3 * rng.standard_normal((3, L))).astype(np.float32)
    x[0, 2 * hop + 7] = np.nan
    x[1, 5 * hop + n_fft // 2 + 11] = np.inf
    cases.append(dict(name="non_finite", x=x, hop=hop, levels=None))
    for c in cases:
        F = 1 + (c["x"].shape[1] - n_fft) // c["hop"]
        idx = np.arange(F)[:, None] * c["hop"] + np.arange(n_fft)[None]
        c["nan_frames"] = ~np.isfinite(c["x"][:, idx]).all(axis=-1)
    return cases


def resample_lengths(orig: int, new: int):
    """The lengths of one rate pair: rows shorter than one window, exact multiples, a ragged tail."""
    from ddsp_pytorch_amd.encoder import support_taps
    g = math.gcd(orig, new)
    o = orig // g
    K = support_taps(orig, new)[2]
    return sorted({n for n in (1, K - 1, o - 1, o, o + 1, 4 * o, 9001) if n >= 1})


def resample_input(orig: int, new: int, L: int, seed: int = 0, rows: int = 3) -> np.ndarray:
    """[rows, L] fp32: N(0, 0.3) rows, the last one (of three) three tones plus nothing else."""
    rng = np.random.default_rng([orig, new, L, seed, 20])
    x = 0.3 * rng.standard_normal((rows, L))
    if rows == 3:
        t = np.arange(L)
        x[2] = 0.3 * (np.sin(2 * np.pi * 0.0101 * t) + np.sin(2 * np.pi * 0.0437 * t + 1.0) + np.sin(2 * np.pi * 0.1103 * t + 2.0))
    return x.astype(np.float32)


def long_positions(target: int, seed: int = 0) -> np.ndarray:
    """The first 4096 outputs, the last 4096, and 4096 drawn with a seed."""
    rng = np.random.default_rng([target, seed, 21])
    return np.concatenate([np.arange(4096), np.arange(target - 4096, target), np.sort(rng.integers(4096, target - 4096, 4096))])


def stock_resample(x: np.ndarray, orig: int, new: int) -> np.ndarray:
    """The stock fp32 formulation (F.pad + F.conv1d) on the CPU."""
    from ddsp_pytorch_amd.encoder import Resample
    with torch.no_grad():
        return Resample(orig, new)(torch.from_numpy(x)).numpy()


def sweep_cases(cases: int, seed: int):
    """The randomised cases of fuzz_parity.sweep_encoder_stages: alternately a loudness case {kind, n_fft, hop, x [B, L]} -- random
    size, hop and frame count, every hop-long segment at its own level over six decades (some exactly zero) -- and a resampler
    case {kind, orig, new, x [B, L]} with a rate pair of RATE_PAIRS and L <= 20 000."""
    rng = np.random.default_rng([seed, 22])
    out = []
    for i in range(cases):
        B = int(rng.integers(1, 4))
        if i % 2 == 0:
            n_fft = int(rng.choice(LOUDNESS_SIZES))
            hop = int(rng.choice([n_fft, n_fft // 2, n_fft // 4 + 3, int(rng.integers(n_fft // 8, n_fft + 18))]))
            F = int(rng.integers(1, 13))
            L = n_fft + (F - 1) * hop + int(rng.integers(0, hop))
            nseg = -(-L // hop)
            levels = 10.0 ** -rng.integers(0, 7, (B, nseg)).astype(np.float64)
            levels[rng.random((B, nseg)) < 0.15] = 0.0
            x = 0.3 * rng.standard_normal((B, L)) * np.repeat(levels, hop, axis=1)[:, :L]
            out.append(dict(kind="loudness", n_fft=n_fft, hop=hop, x=x.astype(np.float32)))
        else:
            orig, new = RATE_PAIRS[int(rng.integers(len(RATE_PAIRS)))]
            L = int(rng.integers(1, 20001))
            out.append(dict(kind="resample", orig=orig, new=new, x=(0.3 * rng.standard_normal((B, L))).astype(np.float32)))
    return out
