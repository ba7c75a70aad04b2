"""The definition of the control transformation in numpy fp64, one row at a time, the same definition in
the kernel's own arithmetic (fp32 combinations, u and v in fp64, the kernel's summation order), and the inputs of the tests.

One row: f0 [T] and a [T] and c [T, H] (fp32 values), optionally noise bands N [T, F]; per output frame t' a source position
pos[t'] in input frames, a pitch ratio r[t'] and an envelope ratio q[t'] (fp32 arrays, as the package hands them to the kernel).

  voiced[i]  f0[i] finite and positive
  A[i, k]    a[i] c[i, k] / S_i where frame i is voiced and fl32(k f0[i]) > sample_rate // 2 is false, S_i the sum of c[i, k] over
             those k; 0 elsewhere, and 0 where S_i = 0: the amplitude the oscillator bank really plays
  E_i(u)     A[i, 1] for u < 1;  (1 - mu) A[i, m] + mu A[i, m + 1] for 1 <= u < H, m = floor(u), mu = u - m;  A[i, H] at u = H;
             0 for u > H
  frame t'   p = pos clamped to [0, T - 1] (NaN -> 0), i0 = floor(p), i1 = min(i0 + 1, T - 1), lam = p - i0
             f0_s = (1 - lam) f0[i0] + lam f0[i1] where both are voiced, the voiced one's f0 where one is
             f0' = fl32(fl32(f0_s) r)
             A'[k'] = (1 - lam) E_i0(u) + lam E_i1(u), u = k' (r / q), k' = 1 .. H'; 0 where fl32(k' f0') > sample_rate // 2
             a' = sum A', c' = A' / a', and 1 / H' where a' = 0
             N'[j] = (1 - lam) X_i0 + lam X_i1, X_i = (1 - nu) N[i, n] + nu N[i, min(n + 1, F - 1)], v = j / q, n = floor(v),
             nu = v - n, for v <= F - 1; 0 for v > F - 1
  silent     neither neighbour voiced: f0' = 0, A' = 0, a' = 0, c' = 1 / H' (N' as above: voicing plays no part in the noise);
             r or q not finite or not positive: that, and N' = 0

TOL_A bounds |A'_device - A'_fp64| relative to the largest A of the frame's two source rows (and the same for N' relative to the
largest N).  tests/test_control_transform_host.py derives it: `transform_fp32` below is the kernel's arithmetic operation by
operation, its difference from fp64 on the device tests' own inputs is measured there, and TOL_A is twice that, rounded up.
"""
import numpy as np

SAMPLE_RATE = 16000
TOL_A = 4e-7
GPU_SHAPES = [(1, 1, 1, 1, 1, 2), (3, 7, 5, 5, 5, 2), (2, 9, 23, 100, 100, 65), (2, 16, 16, 180, 180, 195), (1, 4, 9, 256, 256, 257),
              (2, 12, 12, 64, 37, 65), (1, 8, 8, 65, 130, 65)]                       # (B, T, T', H, H', F)


def voiced_of(f0):
    f = np.asarray(f0, dtype=np.float32)
    return np.isfinite(f) & (f > 0)


def keep_mask(f0, sr, H):
    """[T, H]: the harmonics the bank plays (the product in fp32, strictly >), on voiced frames."""
    f = np.asarray(f0, dtype=np.float32)
    k = np.arange(1, H + 1, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(k[None, :] * f[:, None] > sr // 2) & voiced_of(f)[:, None]


def source_amplitudes(f0, a, c, sr):
    """-> A [T, H] fp64."""
    c64 = np.where(keep_mask(f0, sr, c.shape[-1]), np.asarray(c, np.float64), 0.0)
    S = c64.sum(-1)
    gain = np.where(S == 0, 0.0, np.where(voiced_of(f0), np.asarray(a, np.float64), 0.0) / np.where(S == 0, 1.0, S))
    return c64 * gain[:, None]


def envelope(Ai, u):
    """E_i(u) for the rows Ai [T', H] at u [T', H'], any float dtype (u in fp64; mu rounded to Ai's dtype)."""
    dt = Ai.dtype
    H = Ai.shape[-1]
    m = np.clip(np.floor(np.minimum(u, float(H))), 1, max(1, H - 1)).astype(np.int64)
    mu = (u - m).astype(dt)
    lo, hi = np.take_along_axis(Ai, m - 1, -1), np.take_along_axis(Ai, np.minimum(m, H - 1), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        between = (dt.type(1) - mu) * lo + mu * hi
    return np.where(u < 1, Ai[:, :1], np.where(u < H, between, np.where(u == H, Ai[:, H - 1:], dt.type(0))))


def frame_map(f0, pos, r, q):
    """What both evaluations share, all exact or fp64: i0, i1, lam (fp64; an fp32 value), ok, live, f0' (fp32), r / q."""
    f = np.asarray(f0, dtype=np.float32)
    T = len(f)
    r, q = np.asarray(r, np.float32), np.asarray(q, np.float32)
    p = np.asarray(pos, np.float32).astype(np.float64)
    p = np.clip(np.where(np.isnan(p), 0.0, p), 0.0, float(T - 1))
    i0 = np.floor(p).astype(np.int64)
    i1 = np.minimum(i0 + 1, T - 1)
    lam = p - i0
    ok = np.isfinite(r) & (r > 0) & np.isfinite(q) & (q > 0)
    voiced = voiced_of(f)
    va, vb = voiced[i0], voiced[i1]
    live = ok & (va | vb)
    with np.errstate(invalid="ignore", over="ignore"):
        glide = ((1.0 - lam) * f[i0].astype(np.float64) + lam * f[i1].astype(np.float64)).astype(np.float32)
        f0s = np.where(va & vb, glide, np.where(va, f[i0], f[i1]))
        f0o = np.where(live, f0s * np.where(ok, r, np.float32(1)), np.float32(0)).astype(np.float32)
    rq = np.where(ok, r.astype(np.float64) / np.where(ok, q, np.float32(1)).astype(np.float64), 1.0)
    return dict(i0=i0, i1=i1, lam=lam, ok=ok, va=va, vb=vb, live=live, f0=f0o, rq=rq, q=np.where(ok, q, np.float32(1)).astype(np.float64))


def out_mask(f0o, sr, H_out):
    k = np.arange(1, H_out + 1, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return k[None, :] * f0o[:, None] > sr // 2


def transform(f0, a, c, noise, pos, r, q, sr, H_out):
    """The definition in fp64 -> dict(f0 fp32 [T'], a [T'], c [T', H'], A [T', H'], N [T', F] or None, scale, nscale and the
    frame map); scale [T'] the largest A of the two source rows, nscale the largest N."""
    m = frame_map(f0, pos, r, q)
    A = source_amplitudes(f0, a, c, sr)
    lam = m["lam"][:, None]
    u = np.arange(1, H_out + 1, dtype=np.float64)[None, :] * m["rq"][:, None]
    out = (1.0 - lam) * envelope(A[m["i0"]], u) + lam * envelope(A[m["i1"]], u)
    masked = out_mask(m["f0"], sr, H_out)
    out = np.where(m["live"][:, None] & ~masked, out, 0.0)
    total = out.sum(-1)
    cn = np.where(total[:, None] == 0, 1.0 / H_out, out / np.where(total == 0, 1.0, total)[:, None])
    res = dict(m, u=u, masked=masked, a=total, c=cn, A=out, N=None, scale=np.maximum(A[m["i0"]].max(-1), A[m["i1"]].max(-1)))
    if noise is not None:
        N = np.asarray(noise, np.float64)
        F = N.shape[-1]
        v = np.arange(F, dtype=np.float64)[None, :] / m["q"][:, None]
        n = np.floor(np.minimum(v, float(F - 1))).astype(np.int64)
        nu = v - n
        X = [(1.0 - nu) * np.take_along_axis(N[i], n, -1) + nu * np.take_along_axis(N[i], np.minimum(n + 1, F - 1), -1)
             for i in (m["i0"], m["i1"])]
        res["N"] = np.where(m["ok"][:, None] & (v <= F - 1), (1.0 - lam) * X[0] + lam * X[1], 0.0)
        res["nscale"] = np.maximum(np.abs(N[m["i0"]]).max(-1), np.abs(N[m["i1"]]).max(-1))
    return res


def wave_sum32(x):
    """x [n, K <= 256] fp32 -> [n]: the kernel's sum.  Lane l adds its slots l, l + 64, .. in order from 0, then the xor butterfly
    32, 16, .. 1 over the 64 lanes."""
    n, K = x.shape
    lanes = np.zeros((n, 4, 64), dtype=np.float32)
    lanes.reshape(n, 256)[:, :K] = x
    part = np.zeros((n, 64), dtype=np.float32)
    for sl in range(4):
        part = part + lanes[:, sl]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, idx ^ o]
    return part[:, 0]


def convex32(w, x, y):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float32(1) - w) * x + w * y                  # fp32 arrays: every operation rounds on its own


def transform_fp32(f0, a, c, noise, pos, r, q, sr, H_out):
    """The same in the kernel's arithmetic -> dict(f0, a, c fp32, N fp32 or None)."""
    m = frame_map(f0, pos, r, q)
    c32 = np.where(keep_mask(f0, sr, c.shape[-1]), np.asarray(c, np.float32), np.float32(0))
    S = wave_sum32(c32)
    with np.errstate(invalid="ignore", divide="ignore"):
        gain = np.where(S == 0, np.float32(0), np.asarray(a, np.float32) / np.where(S == 0, np.float32(1), S)).astype(np.float32)
    A = c32 * gain[:, None]
    lam = m["lam"].astype(np.float32)[:, None]
    u = np.arange(1, H_out + 1, dtype=np.float64)[None, :] * m["rq"][:, None]
    out = convex32(lam, envelope(A[m["i0"]], u), envelope(A[m["i1"]], u))
    out = np.where(m["live"][:, None] & ~out_mask(m["f0"], sr, H_out), out, np.float32(0)).astype(np.float32)
    total = wave_sum32(out)
    with np.errstate(invalid="ignore", divide="ignore"):
        cn = np.where(total[:, None] == 0, np.float32(1) / np.float32(H_out), out / np.where(total == 0, np.float32(1), total)[:, None])
    res = dict(f0=m["f0"], a=total, c=cn.astype(np.float32), N=None)
    if noise is not None:
        N = np.asarray(noise, np.float32)
        F = N.shape[-1]
        v = np.arange(F, dtype=np.float64)[None, :] / m["q"][:, None]
        n = np.floor(np.minimum(v, float(F - 1))).astype(np.int64)
        nu = (v - n).astype(np.float32)
        X = [convex32(nu, np.take_along_axis(N[i], n, -1), np.take_along_axis(N[i], np.minimum(n + 1, F - 1), -1)) for i in (m["i0"], m["i1"])]
        res["N"] = np.where(m["ok"][:, None] & (v <= F - 1), convex32(lam, X[0], X[1]), np.float32(0)).astype(np.float32)
    return res


def stretch_positions(T, stretch):
    """-> pos fp32 [T'] of a scalar stretch: T' = max(1, floor(T stretch + 1/2)), pos = (t' + 1/2) T / T' - 1/2 clamped to [0, T - 1]."""
    T_out = max(1, int(np.floor(T * stretch + 0.5)))
    return np.clip((np.arange(T_out, dtype=np.float64) + 0.5) * T / T_out - 0.5, 0.0, float(T - 1)).astype(np.float32)


def ratio_of(semitones):
    """2^(semitones / 12) evaluated in fp64 and rounded to fp32, as the package forms it on the host."""
    return np.exp2(np.asarray(semitones, np.float64) / 12.0).astype(np.float32)


def rows(shape, seed=0):
    """The inputs of one shape (B, T, T', H, H', F) at 16 kHz: f0 [B, T] gliding around the pitch whose top harmonic crosses
    Nyquist, with unvoiced frames (0, NaN, negative) alone and in runs; a [B, T], c [B, T, H] > 0, N [B, T, F] >= 0; transpose
    and formant [B, T'] in +-14 semitones; pos [B, T'] with exact integers, T - 1, values outside [0, T - 1] and a frame halfway
    between a voiced and an unvoiced neighbour."""
    B, T, T_out, H, H_out, F = shape
    rng = np.random.default_rng(1000 * seed + 7 * T + 13 * T_out + H + F)
    t = np.arange(T)[None, :] / max(1, T - 1)
    f0 = ((SAMPLE_RATE / 2 / H) * (0.7 + 0.7 * np.abs(np.sin(np.pi * (t * rng.uniform(0.5, 1.5, (B, 1)) + rng.uniform(0, 1, (B, 1))))))).astype(np.float32)
    if T >= 4:
        f0[:, 2] = 0.0
    if T >= 7:
        f0[:, 4], f0[:, 5] = 0.0, np.nan
    if T >= 9:
        f0[:, 7] = -f0[:, 7]
    a = rng.uniform(0.1, 1.0, (B, T)).astype(np.float32)
    c = (rng.uniform(0.05, 1.0, (B, T, H)) / np.sqrt(np.arange(1, H + 1))).astype(np.float32)
    N = rng.uniform(0.0, 1.0, (B, T, F)).astype(np.float32)
    transpose = rng.uniform(-14.0, 14.0, (B, T_out)).astype(np.float32)
    formant = rng.uniform(-14.0, 14.0, (B, T_out)).astype(np.float32)
    pos = rng.uniform(0.0, T - 1.0, (B, T_out))
    pos[:, ::3] = np.round(pos[:, ::3])
    fixed = [1.0 if T > 1 else 0.0, T - 1.0, -0.75, T + 2.5, 1.5 if T >= 4 else 0.0, 4.5 if T >= 7 else 0.0]
    for i, value in enumerate(fixed[:T_out]):
        pos[:, i] = value
    return dict(f0=f0, a=a, c=c, N=N, transpose=transpose, formant=formant, pos=pos.astype(np.float32))


def formant_tone(T=64, H=40, f0=220.0):
    """A steady tone under three formants (Hz: 600, 1400, 2800) at 16 kHz: controls f0 [T], a [T], c [T, H] fp32."""
    f = f0 * np.arange(1, H + 1)
    env = sum(g * np.exp(-0.5 * ((f - fc) / bw) ** 2) for fc, bw, g in ((600.0, 150.0, 1.0), (1400.0, 200.0, 0.6), (2800.0, 300.0, 0.4))) + 1e-3
    c = np.tile((env / env.sum()).astype(np.float32), (T, 1))
    return np.full(T, f0, dtype=np.float32), np.full(T, 0.5, dtype=np.float32), c
