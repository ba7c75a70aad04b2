"""The definition of the harmonic analysis in numpy fp64, with a plain loop over frames, and the inputs
the tests share.  `analyse_fp32` is the same definition in the arithmetic of the device kernel (fp32 window, products and sums,
32-bit phase words) with exact sines: tests/test_harmonic_analysis_host.py derives the device bound TOL_C from it."""
import numpy as np

# Derived in tests/test_harmonic_analysis_host.py::test_device_bound: 2.39e-6, rounded up to half the audio contract of
# 1e-5 max|audio|.  The margin is for the one figure that is not derived there, EPS_SIN: it admits a hardware error of 4.4e-6.
TOL_C = 5e-6
# Absolute error allowed to the hardware sine / cosine of an argument in [-0.5, 0.5] turns.  No public document states the
# accuracy of v_sin_f32 / v_cos_f32, so this is an assumption, and tests/test_gpu_harmonic_analysis.py puts it to the device
# (test_hardware_sine_is_within_the_figure_the_bound_assumes).
EPS_SIN = 2e-6

# (B, T, hop, W, H, sr) of the device tests
GPU_SHAPES = [(2, 16, 64, 256, 20, 16000), (3, 24, 64, 512, 70, 16000), (1, 20, 128, 1024, 100, 16000), (2, 40, 7, 64, 5, 16000),
              (2, 6, 128, 64, 8, 16000), (1, 8, 512, 2048, 180, 44100), (1, 1, 64, 256, 20, 16000)]
# (hop, W, T, H, m) of the stationary cases: f0 = 16000 m / W
STATIONARY = [(64, 256, 16, 20, 6), (64, 512, 24, 70, 3), (128, 1024, 20, 100, 5)]


def up(x, hop):
    """OscillatorBank.rescale: x [T, ...] -> [T hop, ...]."""
    T = x.shape[0]
    pos = np.clip((np.arange(T * hop) + 0.5) / hop - 0.5, 0.0, T - 1)
    i0 = np.floor(pos).astype(np.int64)
    i1 = np.minimum(i0 + 1, T - 1)
    frac = (pos - i0).reshape((-1,) + (1,) * (x.ndim - 1))
    return x[i0] + (x[i1] - x[i0]) * frac


def clean(f0):
    f0 = np.asarray(f0, dtype=np.float64)
    return np.where(np.isfinite(f0) & (f0 > 0), f0, 0.0)


def theta(f0, hop, sr):
    """f0 [T] -> the phase track in turns [T hop]."""
    return np.cumsum(up(clean(f0), hop) / sr)


def frame_start(t, hop, W):
    return t * hop - (W - hop) // 2


def keep_mask(f0, sr, H, voiced=None):
    """[T, H]: the bank's mask on the fp32 product k f0 (harmonic_oscillator.py:26-31), a usable f0, a voiced frame."""
    f32 = np.asarray(f0, dtype=np.float32)
    k = np.arange(1, H + 1, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        keep = ~(k[None, :] * f32[:, None] > np.float32(sr // 2)) & (np.isfinite(f32) & (f32 > 0))[:, None]
    if voiced is not None:
        keep = keep & np.asarray(voiced, dtype=bool)[:, None]
    return keep


def analyse(audio, f0, hop, sr, H, W, voiced=None, frames=None):
    """One row: audio [T hop], f0 [T] -> C [T, H] complex, a [T], c [T, H].  `frames`: only these (the rest stay 0)."""
    audio = np.asarray(audio, dtype=np.float64)
    T, N = len(f0), len(audio)
    assert N == T * hop and W % 2 == 0
    th = theta(f0, hop, sr)
    j = np.arange(W)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * j / W)
    k = np.arange(1, H + 1)
    C = np.zeros((T, H), dtype=np.complex128)
    for t in (range(T) if frames is None else frames):
        n = frame_start(t, hop, W) + j
        inside = (n >= 0) & (n < N)
        n, wj = n[inside], w[inside]
        turns = (k[None, :] * th[n, None]) % 1.0
        C[t] = (2.0 / wj.sum()) * ((wj * audio[n])[:, None] * np.exp(-2j * np.pi * turns)).sum(axis=0)
    C = np.where(keep_mask(f0, sr, H, voiced), C, 0.0)
    amp = np.abs(C)
    a = amp.sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(a[:, None] == 0, 1.0 / H, amp / a[:, None])
    return C, a, c


def resynth(C, f0, hop, sr):
    """One row: C [T, H] -> harm [T hop]."""
    C = np.asarray(C, dtype=np.complex128)
    H = C.shape[1]
    turns = (np.arange(1, H + 1)[None, :] * theta(f0, hop, sr)[:, None]) % 1.0
    cu = up(C.real, hop) + 1j * up(C.imag, hop)
    return (cu * np.exp(2j * np.pi * turns)).real.sum(axis=-1)


def bank(f0, a, c, hop, sr):
    """OscillatorBank.forward restated in fp64 for one row: f0 [T], a [T], c [T, H] -> [T hop]."""
    H = c.shape[1]
    k = np.arange(1, H + 1)
    amps = np.where(k.astype(np.float32)[None, :] * np.asarray(f0, np.float32)[:, None] > np.float32(sr // 2), 0.0, np.asarray(c, np.float64))
    amps = amps / amps.sum(axis=-1, keepdims=True)
    phases = 2 * np.pi * ((k[None, :] * theta(f0, hop, sr)[:, None]) % 1.0)
    return (up(np.asarray(a, np.float64), hop)[:, None] * up(amps, hop) * np.sin(phases)).sum(axis=-1)


def interior(T, hop, W):
    """The frames whose window lies inside the clip, and the samples between the first and the last one's centres (a centre
    is at t hop + hop / 2 - 1 / 2: these samples interpolate interior frames only)."""
    N = T * hop
    frames = [t for t in range(T) if frame_start(t, hop, W) >= 0 and frame_start(t, hop, W) + W <= N]
    return frames, slice(frames[0] * hop + hop // 2, frames[-1] * hop + hop // 2)


def stationary_controls(hop, W, T, H, m, seed=0, sr=16000):
    rng = np.random.default_rng(seed)
    f0 = np.full(T, sr * m / W, dtype=np.float32)
    assert float(f0[0]) == sr * m / W and H * float(f0[0]) <= sr // 2
    c = rng.uniform(0.2, 1.0, H)
    c = np.tile((c / c.sum()).astype(np.float32), (T, 1))
    a = np.full(T, 0.6, dtype=np.float32)
    return f0, a, c


def vibrato_case(noise=0.0, seed=3, sr=16000, hop=64, W=512, H=20, seconds=2.0):
    """A 220 Hz tone with +-0.5 semitone of vibrato at 5.5 Hz whose amplitudes move at the vibrato's own pace, a by +-50 % at
    6 Hz and every c by +-50 % at 4 Hz with its own phase: (audio, f0, the noise added, the configuration).  The residual
    of this case is the amplitude movement inside a 32 ms window, which the analysis averages; a slower drift (0.7 and
    0.4 Hz at +-30 %) leaves 0.04 % and tests the method far less."""
    rng = np.random.default_rng(seed)
    T = int(seconds * sr) // hop
    tt = (np.arange(T) + 0.5) * hop / sr
    f0 = (220.0 * 2.0 ** (0.5 / 12 * np.sin(2 * np.pi * 5.5 * tt))).astype(np.float32)
    a = 0.5 * (1 + 0.5 * np.sin(2 * np.pi * 6.0 * tt))
    c = (1.0 / np.arange(1, H + 1))[None, :] * (1 + 0.5 * np.sin(2 * np.pi * 4.0 * tt[:, None] + rng.uniform(0, 6.28, H)[None, :]))
    c = c / c.sum(axis=-1, keepdims=True)
    e = noise * rng.standard_normal(T * hop)
    return bank(f0, a, c, hop, sr) + e, f0, e, (hop, sr, H, W)


def gliding_rows(B, T, hop, W, H, sr, seed=0):
    """The device tests' rows: harmonic + noise audio with peak 1 (fp32), and an f0 [B, T] (fp32) that glides across
    sr / (2 H) -- so the top harmonics are masked in some frames and live in others -- with, from four frames on, one frame each
    of 0, a negative value and NaN.  voiced [B, T]: false on the frame before the last, where there are three frames."""
    rng = np.random.default_rng(1000 + seed)
    audio = np.empty((B, T * hop), dtype=np.float32)
    f0 = np.empty((B, T), dtype=np.float32)
    voiced = np.ones((B, T), dtype=bool)
    edge = (sr // 2) / H
    for b in range(B):
        lo, hi = (0.7, 1.4) if b % 2 == 0 else (1.3, 0.8)
        track = edge * lo * (hi / lo) ** ((np.arange(T) + rng.uniform(0, 1)) / max(T, 2))
        track = track.astype(np.float32)
        a = rng.uniform(0.3, 1.0, T)
        c = rng.uniform(0.1, 1.0, (T, H)) / np.arange(1, H + 1)[None, :] ** 0.5
        dead = np.zeros(T, dtype=bool)
        f0[b] = track
        if T >= 4:
            at = rng.choice(T, 3, replace=False)
            dead[at] = True
            f0[b, at] = (0.0, -track[at[1]], np.nan)
        if T >= 3:
            voiced[b, T - 2] = False
        y = bank(track, np.where(dead, 0.0, a), c, hop, sr) + 0.05 * rng.standard_normal(T * hop)
        audio[b] = (y / np.abs(y).max()).astype(np.float32)
        audio[b] /= np.abs(audio[b]).max()
    return audio, f0, voiced


def analyse_fp32(audio, f0, hop, sr, H, W, voiced=None, waves=4):
    """`analyse` in the device kernel's arithmetic, with exact sines: the window rounded to fp32, fl32(w x), phases as 32-bit
    fractions of a turn multiplied by k with wrap-around and converted (signed) to fp32, every term one FMA into an fp32
    accumulator in ascending j over a quarter of the window, the quarters added in order, one fp32 scale.
    -> (C [T, H] complex, sum_j |w x| 2 / norm per frame: what an error of the sine / cosine is multiplied by)."""
    audio = np.asarray(audio, dtype=np.float32)
    T, N = len(f0), len(audio)
    th = theta(f0, hop, sr)
    words = np.floor((th % 1.0) * 2.0 ** 32 + 0.5).astype(np.uint64) % (1 << 32)
    j = np.arange(W)
    w64 = 0.5 - 0.5 * np.cos(2 * np.pi * j / W)
    w32 = w64.astype(np.float32)
    k = np.arange(1, H + 1, dtype=np.uint64)
    chunk = ((W + 15) // 16) * 4
    C = np.zeros((T, H), dtype=np.complex128)
    gain = np.zeros(T)
    for t in range(T):
        n = frame_start(t, hop, W) + j
        inside = (n >= 0) & (n < N)
        wx = np.zeros(waves * chunk, dtype=np.float32)
        ph = np.zeros(waves * chunk, dtype=np.uint64)
        wx[:W][inside] = w32[inside] * audio[n[inside]]
        ph[:W][inside] = words[n[inside]]
        prod = (ph[:, None] * k[None, :]) % (1 << 32)
        ang = ((prod.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.float32) * np.float32(2.0 ** -32)
        cos = np.cos(2 * np.pi * ang.astype(np.float64)).astype(np.float32).astype(np.float64)
        sin = np.sin(2 * np.pi * ang.astype(np.float64)).astype(np.float32).astype(np.float64)
        x = wx.astype(np.float64).reshape(waves, chunk, 1)
        cos, sin = cos.reshape(waves, chunk, H), sin.reshape(waves, chunk, H)
        re = np.zeros((waves, H), dtype=np.float32)
        im = np.zeros((waves, H), dtype=np.float32)
        for q in range(chunk):
            re = (re.astype(np.float64) + x[:, q] * cos[:, q]).astype(np.float32)
            im = (im.astype(np.float64) - x[:, q] * sin[:, q]).astype(np.float32)
        sr_, si_ = re[0], im[0]
        for v in range(1, waves):
            sr_, si_ = sr_ + re[v], si_ + im[v]
        norm = w64[inside].sum()
        scale = np.float32(2.0 / norm)
        C[t] = (sr_ * scale).astype(np.float64) + 1j * (si_ * scale).astype(np.float64)
        gain[t] = 2.0 * np.abs(wx.astype(np.float64)).sum() / norm
    return np.where(keep_mask(f0, sr, H, voiced), C, 0.0), gain
