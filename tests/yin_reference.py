"""The YIN salience of DESIGN.md section 10c in numpy fp64, written as the definition reads, and the inputs the YIN tests
share.  Only the bin frequencies come from the package (`pitch_tables`, as the definition says); nothing else of it is used."""
import numpy as np

from ddsp_pytorch_amd.encoder import pitch_tables

RATE = 16000
WINDOW = 1024
LAGS = 512
BINS = 360
CENTS = 20.0 * np.arange(BINS) + 1997.3794084376191


def bin_constants(octave_cost=0.05):
    """-> (i_b int [360], w_b, cost_b) in fp64."""
    tau = RATE / pitch_tables()[0].numpy().astype(np.float64)
    whole = np.floor(tau)
    return whole.astype(np.int64), tau - whole, octave_cost * np.log2(tau / tau[-1])


def salience(y, hop, octave_cost=0.05, frames=None):
    """y [B, Lr] -> (d' [B, T, 512], salience [B, T, 360]) in fp64; `frames`: only these frame indices of every row."""
    y = np.asarray(y, dtype=np.float64)
    B, Lr = y.shape
    T = 1 + (Lr - WINDOW) // hop
    frames = np.arange(T) if frames is None else np.asarray(frames)
    x = np.stack([y[:, t * hop:t * hop + WINDOW] for t in frames], axis=1)          # [B, T', 1024]
    with np.errstate(all="ignore"):
        d = np.stack([((x[..., :LAGS] - x[..., tau:tau + LAGS]) ** 2).sum(axis=-1) for tau in range(LAGS)], axis=-1)
        c = np.cumsum(d[..., 1:], axis=-1)
        dp = np.ones_like(d)
        dp[..., 1:] = np.where(c > 0, d[..., 1:] * np.arange(1, LAGS) / c, 1.0)
        i, w, cost = bin_constants(octave_cost)
        p0, p1, p2, p3 = dp[..., i - 1], dp[..., i], dp[..., i + 1], dp[..., i + 2]
        v = p1 + 0.5 * w * (p2 - p0 + w * (2 * p0 - 5 * p1 + 4 * p2 - p3 + w * (3 * (p1 - p2) + p3 - p0)))
        s = 1.0 - v - cost
        s = np.where(np.isfinite(s), np.clip(s, 0.0, 1.0), 0.0)
    s[~np.isfinite(x).all(axis=-1)] = 0.0                                           # a frame with a sample that is not finite
    return dp, s


def weighted_cents(s):
    """The nine-bin weighted average around the argmax of s [..., 360] -> cents [...] (fp64)."""
    flat = s.reshape(-1, BINS)
    out = np.empty(flat.shape[0])
    for n, row in enumerate(flat):
        c = int(np.argmax(row))
        lo, hi = max(0, c - 4), min(BINS, c + 5)
        out[n] = np.sum(row[lo:hi] * CENTS[lo:hi]) / np.sum(row[lo:hi])
    return out.reshape(s.shape[:-1])


def cents_of(freq):
    return 1200.0 * np.log2(np.asarray(freq, dtype=np.float64) / 10.0)


def tone(f0, n, rate, rng, noise=0.02, top=None):
    """Harmonics k <= 8 of f0 below `top` (default: Nyquist) with amplitudes 1 / k and random phases, plus white noise."""
    t = np.arange(n)
    top = rate / 2 if top is None else top
    x = np.zeros(n)
    for k in range(1, 9):
        phase = rng.uniform(0, 2 * np.pi)
        if k * f0 < top:
            x += np.sin(2 * np.pi * k * f0 * t / rate + phase) / k
    return x + noise * rng.standard_normal(n)


TONE_F0 = np.exp(np.linspace(np.log(50.0), np.log(900.0), 64))
_CACHE = {}


def tone_frames():
    """The 64 accuracy tones, one 1024-sample frame each at 16 kHz: fp32 [64, 1024] (what the code under test reads)."""
    if "tones" not in _CACHE:
        rng = np.random.default_rng(20240)
        _CACHE["tones"] = np.stack([tone(f, WINDOW, RATE, rng) for f in TONE_F0]).astype(np.float32)
        _CACHE["tones"].setflags(write=False)
    return _CACHE["tones"]


def edge_frames():
    """fp32 [3, 1024]: an all-zero frame, a constant frame, a white-noise frame."""
    if "edges" not in _CACHE:
        rng = np.random.default_rng(20241)
        e = np.zeros((3, WINDOW), dtype=np.float32)
        e[1] = 0.37
        e[2] = rng.standard_normal(WINDOW).astype(np.float32)
        e.setflags(write=False)
        _CACHE["edges"] = e
    return _CACHE["edges"]


def rows(B, Lr, seed):
    """fp32 [B, Lr] at 16 kHz: a tone of its own pitch per row, the last row of three or more white noise."""
    rng = np.random.default_rng(seed)
    y = np.stack([tone(np.exp(rng.uniform(np.log(60.0), np.log(800.0))), Lr, RATE, rng) for _ in range(B)])
    if B >= 3:
        y[-1] = 0.3 * rng.standard_normal(Lr)
    return y.astype(np.float32)
