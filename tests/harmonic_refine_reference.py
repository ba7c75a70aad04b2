"""The definition of the f0 refinement by frequency reassignment in numpy fp64, with a plain loop over
frames, on top of tests/harmonic_analysis_reference.py.  `step_fp32` is one step in the arithmetic of the device kernel (fp32
windows, products and sums, 32-bit phase words, the fp32 store) with exact sines, and `bound` what an error of EPS_SIN in the
hardware sine and cosine can do to num, den and g: tests/test_harmonic_refine_host.py derives the device bound from the two."""
import numpy as np

import harmonic_analysis_reference as ref

GRID_OFFSET = 1997.3794084376191                 # cents of bin 0 of the 360-bin pitch grid (20 cents a bin)
# The device test allows every frame 2 (1 + FP32_SHARE) times its own sine / cosine part (`bound`).  FP32_SHARE is what the
# kernel's fp32 arithmetic adds, as a share of that part: tests/test_harmonic_refine_host.py::test_device_bound measures it with
# `step_fp32` on the device tests' own inputs (at most 0.168 for g, where it is the fp32 store, 0.006 for num and 0.012 for den)
# and asserts it stays below this.  The factor 2 is section 14's, and for the same reason: EPS_SIN is assumed, not documented.
FP32_SHARE = 0.25


def to_grid(f0):
    """The track rounded to the centres of the 360-bin grid: 10 * 2^((20 b + GRID_OFFSET) / 1200)."""
    b = np.round((1200.0 * np.log2(np.asarray(f0, np.float64) / 10.0) - GRID_OFFSET) / 20.0)
    return 10.0 * 2.0 ** ((20.0 * b + GRID_OFFSET) / 1200.0)


def cents(f, g):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / np.asarray(g, np.float64))


def windows(W):
    """The periodic Hann window and its derivative per sample."""
    j = np.arange(W)
    return 0.5 - 0.5 * np.cos(2 * np.pi * j / W), (np.pi / W) * np.sin(2 * np.pi * j / W)


def interior_frames(T, hop, W):
    return [t for t in range(T) if ref.frame_start(t, hop, W) >= 0 and ref.frame_start(t, hop, W) + W <= T * hop]


def alive_frames(f0, voiced=None):
    with np.errstate(invalid="ignore"):
        alive = np.isfinite(f0) & (f0 > 0)
    return alive if voiced is None else alive & np.asarray(voiced, dtype=bool)


def frame_sums(audio, th, t, hop, W, H):
    """C_k and D_k (no scale, no mask) of an interior frame, and sum_j |w x|, sum_j |w' x|."""
    w, wd = windows(W)
    n = ref.frame_start(t, hop, W) + np.arange(W)
    e = np.exp(-2j * np.pi * ((np.arange(1, H + 1)[None, :] * th[n, None]) % 1.0))
    x = audio[n]
    return ((w * x)[:, None] * e).sum(axis=0), ((wd * x)[:, None] * e).sum(axis=0), np.abs(w * x).sum(), np.abs(wd * x).sum()


def _frame_fp64(audio, th, fup, t, hop, sr, H, W, keep):
    C, D, _, _ = frame_sums(audio, th, t, hop, W, H)
    C, D = np.where(keep, C, 0.0), np.where(keep, D, 0.0)
    k = np.arange(1, H + 1)
    w = windows(W)[0]
    n = ref.frame_start(t, hop, W) + np.arange(W)
    return (k * (D * np.conj(C)).imag).sum(), (k * k * np.abs(C) ** 2).sum(), (w * fup[n]).sum() / w.sum()


def step(audio, f0, anchor, hop, sr, H, W, voiced=None, max_cents=50.0, frame=_frame_fp64, frames=None):
    """One refinement step of one row: audio [T hop], f0 [T], the anchor track [T] -> (g [T], num [T], den [T]); num and den are
    0 on the frames that are not measured.  `frames`: only these are measured (the others are not to be read)."""
    audio, f0, anchor = np.asarray(audio, np.float64), np.asarray(f0, np.float64), np.asarray(anchor, np.float64)
    T = len(f0)
    assert len(audio) == T * hop and W % 2 == 0
    alive = alive_frames(f0, voiced)
    inter = interior_frames(T, hop, W)
    th, fup = ref.theta(f0, hop, sr), ref.up(ref.clean(f0), hop)
    keep = ref.keep_mask(f0, sr, H, voiced)
    g, num, den = f0.copy(), np.zeros(T), np.zeros(T)
    for t in inter:
        if not alive[t] or (frames is not None and t not in frames):
            continue
        num[t], den[t], mean = frame(audio, th, fup, t, hop, sr, H, W, keep[t])
        with np.errstate(invalid="ignore", divide="ignore"):
            value = mean - sr / (2 * np.pi) * num[t] / den[t]
        if den[t] != 0 and np.isfinite(value):
            g[t] = value
    if inter:
        lo, hi = inter[0], inter[-1]
        before, after = alive & (np.arange(T) < lo), alive & (np.arange(T) > hi)
        g[before] = f0[before] * (g[lo] / f0[lo] if alive[lo] else 1.0)          # (an unchanged g[lo] is the ratio 1)
        g[after] = f0[after] * (g[hi] / f0[hi] if alive[hi] else 1.0)
    up_, down = 2.0 ** (max_cents / 1200.0), 2.0 ** (-max_cents / 1200.0)
    g[alive] = np.minimum(np.maximum(g[alive], anchor[alive] * down), anchor[alive] * up_)
    return g, num, den


def refine(audio, f0, hop, sr, H, W, voiced=None, iterations=2, max_cents=50.0):
    """`iterations` steps from f0, anchored at f0 -> the track after every step, [iterations + 1, T] (row 0 is f0)."""
    tracks = [np.asarray(f0, np.float64)]
    for _ in range(iterations):
        tracks.append(step(audio, tracks[-1], tracks[0], hop, sr, H, W, voiced, max_cents)[0])
    return np.stack(tracks)


def residual(audio, f0, hop, sr, H, W, voiced=None):
    """harmonic_residual's residual of one row along f0, as a share of the signal's rms over `interior`'s samples."""
    C, _, _ = ref.analyse(audio, f0, hop, sr, H, W, voiced)
    _, samples = ref.interior(len(f0), hop, W)
    r = np.asarray(audio, np.float64) - ref.resynth(C, f0, hop, sr)
    return np.sqrt(np.mean(r[samples] ** 2) / np.mean(np.asarray(audio, np.float64)[samples] ** 2))


def steady_case(f, sr, hop, W, H, T, off_cents):
    """A steady tone with c ~ 1 / k and a = 0.5: (audio, the true track, the track `off_cents` above it)."""
    f0 = np.full(T, f, dtype=np.float64)
    c = np.tile(1.0 / np.arange(1, H + 1), (T, 1))
    return ref.bank(f0, np.full(T, 0.5), c / c.sum(axis=-1, keepdims=True), hop, sr), f0, f0 * 2.0 ** (off_cents / 1200.0)


def glide_case(sr=44100, hop=512, W=2048, H=60, T=24, f=196.0, semitones=2.0):
    """A glide of two semitones over the clip, 60 harmonics ~ 1 / k: (audio, the true track, its grid rounding)."""
    f0 = f * 2.0 ** (semitones / 12.0 * (np.arange(T) + 0.5) / T)
    c = np.tile(1.0 / np.arange(1, H + 1), (T, 1))
    return ref.bank(f0, np.full(T, 0.5), c / c.sum(axis=-1, keepdims=True), hop, sr), f0, to_grid(f0)


# ------------------------------------------------------------------------------------------------- the device's arithmetic

def _wave_butterfly(v):
    """wave_sum of csrc/ddsp_internal.h over each 64 of 256 fp32 values, then the four wavefronts in order."""
    v = v.astype(np.float32).reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ o]).astype(np.float32)
    total = v[0, 0]
    for wv in range(1, 4):
        total = np.float32(total + v[wv, 0])
    return total


def _frame_fp32(audio, th, fup, t, hop, sr, H, W, keep, waves=4):
    w64, wd64 = windows(W)
    w32, wd32 = w64.astype(np.float32), wd64.astype(np.float32)
    x = np.asarray(audio, dtype=np.float32)
    n = ref.frame_start(t, hop, W) + np.arange(W)
    words = np.floor((th[n] % 1.0) * 2.0 ** 32 + 0.5).astype(np.uint64) % (1 << 32)
    chunk = ((W + 15) // 16) * 4
    wx, wdx, ph = (np.zeros(waves * chunk, dtype=dt) for dt in (np.float32, np.float32, np.uint64))
    wx[:W], wdx[:W], ph[:W] = w32 * x[n], wd32 * x[n], words
    prod = (ph[:, None] * np.arange(1, H + 1, dtype=np.uint64)[None, :]) % (1 << 32)
    ang = ((prod.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.float32) * np.float32(2.0 ** -32)
    cos = np.cos(2 * np.pi * ang.astype(np.float64)).astype(np.float32).astype(np.float64).reshape(waves, chunk, H)
    sin = np.sin(2 * np.pi * ang.astype(np.float64)).astype(np.float32).astype(np.float64).reshape(waves, chunk, H)
    xs, ds = wx.astype(np.float64).reshape(waves, chunk, 1), wdx.astype(np.float64).reshape(waves, chunk, 1)
    acc = np.zeros((4, waves, H), dtype=np.float32)              # C re, C im, D re, D im
    for q in range(chunk):
        terms = (xs[:, q] * cos[:, q], -xs[:, q] * sin[:, q], ds[:, q] * cos[:, q], -ds[:, q] * sin[:, q])
        for i in range(4):
            acc[i] = (acc[i].astype(np.float64) + terms[i]).astype(np.float32)
    cr, ci, dr, di = (acc[i, 0] for i in range(4))
    for v in range(1, waves):
        cr, ci, dr, di = cr + acc[0, v], ci + acc[1, v], dr + acc[2, v], di + acc[3, v]
    kf = np.arange(1, H + 1, dtype=np.float32)
    cross = (di.astype(np.float64) * cr - (dr * ci).astype(np.float64)).astype(np.float32)       # fma(di, cr, -fl(dr ci))
    power = (ci.astype(np.float64) * ci + (cr * cr).astype(np.float64)).astype(np.float32)       # fma(ci, ci, fl(cr cr))
    tn, td = np.zeros(256, dtype=np.float32), np.zeros(256, dtype=np.float32)
    tn[:H], td[:H] = np.where(keep, kf * cross, 0), np.where(keep, (kf * kf) * power, 0)
    mean = (w32.astype(np.float64) * fup[n]).sum() / w32.astype(np.float64).sum()
    return float(_wave_butterfly(tn)), float(_wave_butterfly(td)), mean


def step_fp32(audio, f0, anchor, hop, sr, H, W, voiced=None, max_cents=50.0):
    """`step` in the device kernels' arithmetic with exact sines; g, num and den rounded to fp32 as they are stored."""
    f0 = np.asarray(f0, dtype=np.float32)
    g, num, den = step(np.asarray(audio, np.float32), f0, np.asarray(anchor, np.float32), hop, sr, H, W, voiced, max_cents, _frame_fp32)
    return g.astype(np.float32), num.astype(np.float32), den.astype(np.float32)


def bound(audio, f0, hop, sr, H, W, voiced=None, frames=None):
    """What errors of up to EPS_SIN in every sine and cosine, all in the worst direction, do to one step of one row, per frame:
    (|d num|, |d den|, |d g| in Hz, vacuous), 0 on the frames that are not measured.  `vacuous`: den <= 2 |d den| somewhere."""
    audio, f0 = np.asarray(audio, np.float64), np.asarray(f0, np.float64)
    T = len(f0)
    alive = alive_frames(f0, voiced)
    th = ref.theta(f0, hop, sr)
    keep = ref.keep_mask(f0, sr, H, voiced)
    k = np.arange(1, H + 1)
    dnum, dden, dg, vacuous = np.zeros(T), np.zeros(T), np.zeros(T), False
    for t in interior_frames(T, hop, W):
        if not alive[t] or (frames is not None and t not in frames):
            continue
        C, D, sc, sd = frame_sums(audio, th, t, hop, W, H)
        C, D = np.abs(C)[keep[t]], np.abs(D)[keep[t]]
        kk = k[keep[t]]
        ec, ed = np.sqrt(2.0) * ref.EPS_SIN * sc, np.sqrt(2.0) * ref.EPS_SIN * sd
        num, den, _ = _frame_fp64(audio, th, np.zeros(T * hop), t, hop, sr, H, W, keep[t])
        dnum[t] = (kk * (D * ec + C * ed + ec * ed)).sum()
        dden[t] = (kk * kk * (2 * C * ec + ec * ec)).sum()
        if not den > 2 * dden[t]:
            vacuous = True
            continue
        dg[t] = sr / (2 * np.pi) * (dnum[t] + abs(num / den) * dden[t]) / (den - dden[t])
        dg[t] += 2.0 ** -23 * abs(f0[t])                         # the mean (fp32 window weights) and the fp32 store, half an ulp each
    return dnum, dden, dg, vacuous
