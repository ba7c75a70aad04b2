"""TEST INFRASTRUCTURE ONLY -- the overlap-add filtered noise (include/ddsp_hip.h: ddsp_noise_ola_*) in numpy
fp64: forward, backward, both yardsticks, and the inputs and statistics the host and device tests share.  `ola_fp32` and
`ola_grad_fp32` are the same definition in the arithmetic of csrc/ddsp_noise_ola.hip (fp32 tables, every sum a chain of fp32
multiply-adds in the kernels' order): tests/test_noise_ola_host.py derives TOL_Y and TOL_DH from them.

With M = 2 (F - 1), P = M / 2, N = T hop:
    x[b, t hop + j] = fl32(2 u - 1)
    h_t[e] = (1/2 + 1/2 cos(2 pi e / M)) (1/M) sum_k c_k H_t[k] cos(2 pi k e / M)        e in (-P, P); the tap e = -P is never evaluated
    y[b, n] = sum_m h_{m // hop}[n - m] x[b, m]                                           over 0 <= m < N with |n - m| < P
    q_t[e]  = sum_{j < hop} x[t hop + j] g[t hop + j + e],   dH_t[k] = (c_k / M) sum_e w(e) cos(2 pi k e / M) q_t[e]
    Yf[b, n] = sum_e w(e) A_{(n - e) // hop} |x[n - e]|,  A_t = (1/M) sum_k c_k |H_t[k]|;   Yb[b, t] = (2/M) sum_e w(e) sum_j |x||g|
Nothing under ddsp-pytorch_amd/ may import this module.
"""
from __future__ import annotations

import numpy as np

import noise_analysis_reference as nar
from noise_grad_reference import draw  # noqa: F401  (x = fp32(2u - 1) of an injected draw or of the in-kernel Philox stream)

# Derived in tests/test_noise_ola_host.py::test_device_bound (figures there and in DESIGN.md section 5a): twice the largest deviation
# of the fp32 emulation from fp64 on GPU_SHAPES, relative to the yardstick, plus the window's definitional term, rounded up to one
# digit.  Both lie below the noise contract of 2e-6.
TOL_Y = 3e-7
TOL_DH = 3e-7

# (B, T, hop, F) of the device tests.  The last one is there for the kernel's other path: with a hop of 2 the responses of a tile's frames
# do not fit in LDS and the convolution reads its taps from the workspace.
GPU_SHAPES = [(2, 5, 128, 65), (1, 7, 50, 33), (1, 9, 16, 33), (3, 6, 64, 65), (2, 3, 512, 195), (1, 1, 64, 17), (1, 4, 7, 5),
              (1, 2, 1024, 257), (1, 40, 2, 65)]


def ck(F):
    c = np.full(F, 2.0)
    c[0] = c[F - 1] = 1.0
    return c


def window(F):
    """w(e) for e in (-P, P), index e + P - 1: 1/2 + 1/2 cos(2 pi e / M) in fp64."""
    P = F - 1
    e = np.arange(-P + 1, P)
    return 0.5 + 0.5 * np.cos(np.pi * e / P)


def responses(H):
    """H [..., F] -> h [..., 2P - 1]: h[e] at index e + P - 1 for e in (-P, P)."""
    H = np.asarray(H, dtype=np.float64)
    F = H.shape[-1]
    P = F - 1
    M = 2 * P
    e = np.arange(-P + 1, P)
    k = np.arange(F)
    C = np.cos(np.pi * ((k[:, None] * e[None, :]) % M) / P) * (ck(F) / M)[:, None]           # [F, 2P - 1]
    with np.errstate(invalid="ignore"):
        raw = np.einsum("...k,ke->...e", H, C)                   # (a non-finite H_t: its whole response, and only its own)
    return raw * window(F)


def ola_fp64(H, hop, uniform=None, seed=0, offset=0, x=None):
    """H [B, T, F] -> (y [B, N], Yf [B, N]) in fp64 for the draw `uniform` [B, T, hop], the in-kernel stream of (seed, offset),
    or the samples x [B, T, hop] themselves."""
    H = np.asarray(H, dtype=np.float64)
    B, T, F = H.shape
    P, N = F - 1, T * hop
    if x is None:
        x = draw(B, T, hop, uniform, seed, offset)
    x = np.asarray(x, dtype=np.float64).reshape(B, N)
    h = responses(H)
    A = (np.abs(H) * ck(F)).sum(-1) / (2 * P)                                                # [B, T]
    w = window(F)
    y = np.zeros((B, N))
    Y = np.zeros((B, N))
    n = np.arange(N)
    with np.errstate(invalid="ignore"):
        for e in range(P - 1, -P, -1):                                                       # m = n - e ascending
            m = n - e
            ok = (m >= 0) & (m < N)
            mo = m[ok]
            y[:, ok] += h[:, mo // hop, e + P - 1] * x[:, mo]
            Y[:, ok] += w[e + P - 1] * A[:, mo // hop] * np.abs(x[:, mo])
    return y, Y


def _lag_windows(g, T, hop, P):
    """g [B, N] -> [B, T, hop + 2P - 2]: g[t hop - (P - 1) + i], zero outside the row."""
    B, N = g.shape
    gp = np.concatenate([np.zeros((B, P - 1), g.dtype), g, np.zeros((B, P - 1), g.dtype)], axis=1)
    idx = (np.arange(T) * hop)[:, None] + np.arange(hop + 2 * P - 2)[None, :]
    return gp[:, idx]


def ola_grad_fp64(grad_y, F, hop, uniform=None, seed=0, offset=0):
    """grad_y [B, N] (taken as fp32) -> (dH [B, T, F], Yb [B, T]) in fp64."""
    g = np.ascontiguousarray(grad_y, dtype=np.float32).astype(np.float64)
    B, N = g.shape
    T, P = N // hop, F - 1
    M = 2 * P
    x = draw(B, T, hop, uniform, seed, offset).astype(np.float64)                            # [B, T, hop]
    gw = _lag_windows(g, T, hop, P)
    q = np.empty((B, T, 2 * P - 1))
    a = np.empty((B, T, 2 * P - 1))
    with np.errstate(invalid="ignore"):
        for i in range(2 * P - 1):                                                           # e = i - (P - 1)
            q[..., i] = (x * gw[..., i:i + hop]).sum(-1)
            a[..., i] = (np.abs(x) * np.abs(gw[..., i:i + hop])).sum(-1)
        e = np.arange(-P + 1, P)
        k = np.arange(F)
        C = np.cos(np.pi * ((k[:, None] * e[None, :]) % M) / P) * (ck(F) / M)[:, None]       # [F, 2P - 1]
        qw = q * window(F)
        dH = np.einsum("bte,ke->btk", qw, C)
        Y = (2.0 / M) * (a * window(F)).sum(-1)
    return dH, Y


def ratio(got, ref, yard):
    """Largest |got - ref| / yard over the entries where ref is finite (an exact match is 0 even against a zero yardstick; a
    non-finite got where ref is finite is inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    yard = np.broadcast_to(np.asarray(yard, np.float64), ref.shape)
    fin = np.isfinite(ref)
    err = np.where(fin, np.abs(got - np.where(fin, ref, 0.0)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / yard)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- inputs

def gpu_H(shape, seed=0):
    """[B, T, F] fp32: smooth and time-varying, one all-zero frame per row (where the row has at least two frames)."""
    B, T, hop, F = shape
    rng = np.random.default_rng(3000 + seed)
    H = np.empty((B, T, F), dtype=np.float32)
    for b in range(B):
        H[b] = nar.smooth_H(F, T, seed=10 * seed + b).astype(np.float32)
        if T >= 2:
            H[b, int(rng.integers(0, T))] = 0.0
    return H


def zero_frames(H):
    return np.argwhere((np.asarray(H) == 0).all(axis=-1))


def gpu_uniform(shape, seed=0):
    B, T, hop, F = shape
    return np.random.default_rng(4000 + seed).random((B, T, hop), dtype=np.float32)


def gpu_grad(shape, seed=0):
    B, T, hop, F = shape
    return np.random.default_rng(5000 + seed).standard_normal((B, T * hop)).astype(np.float32)


def lowpass_H(F):
    """The example of DESIGN.md section 5a: a Gaussian of width 0.15 of the band axis plus a floor of 0.02."""
    b = np.arange(F) / (F - 1)
    return np.exp(-0.5 * (b / 0.15) ** 2) + 0.02


def reach(t, T, hop, F):
    """The samples of a row a non-finite H_t reaches, and equally the samples whose gradient reaches frame t: [lo, hi)."""
    P = F - 1
    return max(0, t * hop - P + 1), min(T * hop, (t + 1) * hop + P - 1)


# ------------------------------------------------------------------------------------------------------------ statistics

def position_variance_ratio(y, hop, skip=8):
    """min / max over the position in the frame of the mean square of y [T hop], `skip` frames ignored at each end."""
    fr = np.asarray(y, dtype=np.float64).reshape(-1, hop)[skip:-skip]
    v = (fr ** 2).mean(axis=0)
    return float(v.min() / v.max())


def welch_distance(y, H, hop, skip=8, seg=128):
    """Relative l2 distance of the Welch spectrum of y (Hann segments of `seg`, half overlapped) from 1/3 |DTFT h|^2 times the
    window's power, for the constant filter H [F]."""
    y = np.asarray(y, dtype=np.float64)[skip * hop:-skip * hop]
    F = len(H)
    P = F - 1
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(seg) / seg)
    starts = np.arange(0, len(y) - seg + 1, seg // 2)
    segs = y[starts[:, None] + np.arange(seg)[None, :]] * win
    S = (np.abs(np.fft.rfft(segs, axis=-1)) ** 2).mean(axis=0)
    h = responses(np.asarray(H, dtype=np.float64))                                           # e in (-P, P)
    e = np.arange(-P + 1, P)
    omega = 2 * np.pi * np.arange(seg // 2 + 1) / seg
    hhat = (h[None, :] * np.cos(omega[:, None] * e[None, :])).sum(-1)                        # (h is even: a real transform)
    want = hhat ** 2 / 3.0 * (win ** 2).sum()
    return float(np.linalg.norm(S - want) / np.linalg.norm(want))


# ------------------------------------------------------------------------------------- the device kernels' arithmetic

def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _tables(F, ulps=0):
    """(ct [M]: fl32 cos(2 pi m / M); win [P]: fma(0.5, ct[d], 0.5)) as fp64 arrays of fp32 values.  `ulps` moves every cosine
    by that many fp32 ulps (the device's cospif is not correctly rounded: test_device_bound measures what one ulp is worth)."""
    P = F - 1
    ct = np.cos(np.pi * np.arange(2 * P) / P).astype(np.float32)
    for _ in range(abs(ulps)):
        ct = np.nextafter(ct, np.float32(np.inf if ulps > 0 else -np.inf))
    ct = ct.astype(np.float64)
    return ct, _f32(0.5 * ct[:P] + 0.5)


def _cos_chain(v, F, outs, ulps=0):
    """sum_{i=1}^{P-1} v[..., i] ct[(o i) mod M] for o in range(outs), ascending i, one fp32 multiply-add per term."""
    P = F - 1
    ct, _ = _tables(F, ulps)
    o = np.arange(outs)
    acc = np.zeros(v.shape[:-1] + (outs,))
    for i in range(1, P):
        acc = _f32(acc + v[..., i:i + 1] * ct[(o * i) % (2 * P)])
    return acc


def responses_fp32(H, ulps=0):
    """H [..., F] (fp32 values) -> hh [..., P]: the half d = |e| of the even response, as cos_sum_kernel<IR> forms it."""
    H = _f32(H)
    F = H.shape[-1]
    P = F - 1
    _, win = _tables(F, ulps)
    acc = _cos_chain(H, F, P, ulps)
    sign = np.where(np.arange(P) % 2 == 1, -1.0, 1.0)
    edge = _f32(H[..., 0:1] + sign * H[..., P:P + 1])
    return _f32(_f32(_f32(2.0 * acc + edge) * _f32(1.0 / (2 * P))) * win)


def ola_fp32(H, hop, uniform=None, seed=0, offset=0, ulps=0):
    """The forward in the kernels' arithmetic: y [B, N] as fp64 values of fp32 numbers."""
    H = np.asarray(H, dtype=np.float32)
    B, T, F = H.shape
    P, N = F - 1, T * hop
    x = draw(B, T, hop, uniform, seed, offset).astype(np.float64).reshape(B, N)
    hh = responses_fp32(H, ulps)
    y = np.zeros((B, N))
    n = np.arange(N)
    for e in range(P - 1, -P, -1):
        m = n - e
        ok = (m >= 0) & (m < N)
        mo = m[ok]
        y[:, ok] = _f32(y[:, ok] + hh[:, mo // hop, abs(e)] * x[:, mo])
    return y


def ola_grad_fp32(grad_y, F, hop, uniform=None, seed=0, offset=0, ulps=0):
    """The backward in the kernels' arithmetic: dH [B, T, F]."""
    g = np.ascontiguousarray(grad_y, dtype=np.float32).astype(np.float64)
    B, N = g.shape
    T, P = N // hop, F - 1
    x = draw(B, T, hop, uniform, seed, offset).astype(np.float64)
    gw = _lag_windows(g, T, hop, P)
    lags = np.arange(2 * P - 1)
    q = np.zeros((B, T, 2 * P - 1))
    for j in range(hop):
        q = _f32(q + x[..., j:j + 1] * gw[..., j + lags])
    _, win = _tables(F, ulps)
    Gs = np.empty((B, T, P))
    Gs[..., 0] = q[..., P - 1]
    if P > 1:
        Gs[..., 1:] = _f32(q[..., P:] + q[..., P - 2::-1])
    Gs = _f32(win * Gs)
    acc = _cos_chain(Gs, F, F, ulps)
    return _f32(_f32(ck(F) * _f32(1.0 / (2 * P))) * _f32(Gs[..., 0:1] + acc))
