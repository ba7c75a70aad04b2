"""TEST INFRASTRUCTURE ONLY -- the definition of the noise analysis for the overlap-add noise (include/ddsp_hip.h:
ddsp_noise_analysis_ola) in numpy fp64, and the inputs the tests share.  `analyse_ola_fp32` is the same
definition in the arithmetic of the device kernels (fp32 tables, every sum a chain of fp32 FMAs in the kernels' order):
tests/test_noise_analysis_ola_host.py derives the device bound TOL_H_OLA from it.

With M = 2 (F - 1), P = L = F - 1, N = T hop and x[n] = 0 for n >= N:
    h[e]        the even response of noise_ola_reference.responses, |e| <= P - 1
    R_ola(H)[l] = (hop / 3) sum_e h[e] h[e + l]                                              l in [0, L)
    r_t[l]      = (hop / c_t[l]) sum_{n < hop, t hop + n + l < N} x[t hop + n] x[t hop + n + l],  c_t[l] = clamp(N - t hop - l, 0, hop)
    p = max(P(rbar), 0),  H^0 = sqrt(3 p / hop),  H^{i+1} = H^i sqrt(p / max(P(R_ola(H^i)), tiny))
the frame average and P being section 15's (noise_analysis_reference).  Nothing under ddsp-pytorch_amd/ may import this module.
"""
from __future__ import annotations

import numpy as np

import noise_analysis_reference as nar
import noise_ola_reference as olar
from noise_analysis_reference import P, average_frames, rel, smooth_H, tiny  # noqa: F401  (section 15's, unchanged)

# Derived in tests/test_noise_analysis_ola_host.py::test_device_bound: the largest deviation of `analyse_ola_fp32` from fp64 over
# the device tests' inputs is 8.36e-5 of the frame's max_b H, at (2, 4, 512, 257, 1, 2), and 4.93e-7 of max_b p.  Each bound is
# twice its figure, rounded up to one digit, because any other summation order is as valid as the emulated one.  H's figure is
# p's seen through the square root: the sine rows have bands at 1e-7 of the frame's largest p and below, where an error of
# d = 5e-7 max_b p in p is d / (2 sqrt(p / max_b p)) of max_b H in H.
TOL_H_OLA = 2e-4
TOL_P_OLA = 1e-6

ITERATIONS = 8                                                   # the default of this model

# (B, T, hop, F, average, iterations) of the device tests
GPU_SHAPES = [(2, 12, 128, 65, 1, 8), (1, 9, 100, 33, 3, 8), (1, 5, 512, 195, 5, 4), (2, 4, 512, 257, 1, 2), (1, 1, 128, 65, 1, 8),
              (1, 40, 16, 65, 3, 8), (1, 30, 2, 33, 5, 4), (1, 3, 1024, 257, 1, 1), (2, 6, 128, 33, 3, 0)]


# ------------------------------------------------------------------------------------------------------- steps 1 and 2

def rho(H):
    """H [..., F] -> [..., L]: sum_e h[e] h[e + l] over the taps |e|, |e + l| <= P - 1."""
    h = olar.responses(H)                                         # [..., 2P - 1], h[e] at e + P - 1
    L, n = h.shape[-1] // 2 + 1, h.shape[-1]
    out = np.empty(h.shape[:-1] + (L,))
    for lag in range(L):
        out[..., lag] = (h[..., :n - lag] * h[..., lag:]).sum(-1)
    return out


def model_R(H, hop):
    """H [..., F] -> R_ola(H) [..., L]: the expected autocorrelation of the overlap-add noise of a constant H, times hop."""
    return rho(H) * (hop / 3.0)


# -------------------------------------------------------------------------------------------------------------- step 3

def counts(T, hop, L):
    """[T, L]: c_t[l] = clamp(N - t hop - l, 0, hop), the number of products of lag l that start in frame t and end inside the row."""
    return np.clip(T * hop - np.arange(T)[:, None] * hop - np.arange(L)[None, :], 0, hop)


def measure(x, hop, F):
    """x [..., T hop] -> r [..., T, L]."""
    x = np.asarray(x, dtype=np.float64)
    N, L = x.shape[-1], F - 1
    T = N // hop
    s = np.zeros(x.shape[:-1] + (T, L))
    for lag in range(min(L, N)):
        prod = np.concatenate([x[..., :N - lag] * x[..., lag:], np.zeros(x.shape[:-1] + (lag,))], axis=-1)
        s[..., lag] = prod.reshape(x.shape[:-1] + (T, hop)).sum(-1)
    c = counts(T, hop, L)
    return s * np.where(c > 0, hop / np.maximum(c, 1), 0.0)


# -------------------------------------------------------------------------------------------------------------- step 5

def fixed_point(rbar, hop, F, iterations=ITERATIONS):
    """rbar [..., L] -> (H [..., F], p [..., F])."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.maximum(P(rbar, F), 0.0)                          # (np.maximum keeps a NaN)
        H = np.sqrt(3.0 * p / hop)
        for _ in range(iterations):
            H = H * np.sqrt(p / np.maximum(P(model_R(H, hop), F), tiny(np.float64)))
    return H, p


def check_args(hop, F, average, iterations):
    if F < 2:
        raise ValueError(f"n_filters must be at least 2, got {F}")
    if hop < 1:
        raise ValueError(f"hop must be positive, got {hop}")
    if average < 1 or average % 2 == 0:
        raise ValueError(f"average must be an odd count of frames, got {average}")
    if iterations < 0:
        raise ValueError(f"iterations must be at least 0, got {iterations}")


def noise_analysis(x, hop, F, average=1, iterations=ITERATIONS):
    """x [..., T hop] -> (H [..., T, F], p [..., T, F])."""
    check_args(hop, F, average, iterations)
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] == 0 or x.shape[-1] % hop:
        raise ValueError(f"{x.shape[-1]} samples are no positive whole number of frames of hop {hop}")
    with np.errstate(invalid="ignore", over="ignore"):
        return fixed_point(average_frames(measure(x, hop, F), average), hop, F, iterations)


def reach(n, T, hop, F, average=1):
    """[T] bool: the frames a sample at n that is not finite reaches: t hop <= n < t hop + hop + L - 1, widened by the averaging
    window."""
    t = np.arange(T)
    own = (t * hop <= n) & (n < t * hop + hop + F - 2)
    s = (average - 1) // 2
    return np.array([own[max(0, u - s):u + s + 1].any() for u in range(T)])


# ---------------------------------------------------------------------------------------------------------------- inputs

def ola_noise(H, hop, seed):
    """H [T, F] -> x [T hop] fp64: the fp64 overlap-add noise of a seeded injected uniform draw."""
    H = np.asarray(H, dtype=np.float64)
    u = np.random.default_rng(seed).random((1, H.shape[0], hop), dtype=np.float32)
    return olar.ola_fp64(H[None], hop, uniform=u)[0][0]


def gpu_rows(shape, seed=0):
    """The device tests' rows [B, T hop] (fp32): fp64 overlap-add noise of a smooth, time-varying H with one frame's samples zeroed
    (where there are at least three frames); the last row of a batch is a sine instead, and a batch of one row has the sine added
    to the second half of its frames."""
    B, T, hop, F, _, _ = shape
    rng = np.random.default_rng(6000 + seed)
    x = np.empty((B, T * hop), dtype=np.float32)
    n = np.arange(T * hop)
    for b in range(B):
        row = ola_noise(smooth_H(F, T, seed=10 * seed + b), hop, seed=100 * seed + b + 1)
        sine = 0.5 * np.sin(2 * np.pi * rng.uniform(0.05, 0.2) * n + rng.uniform(0, 6.28))
        if B > 1 and b == B - 1:
            row = sine
        elif B == 1 and T >= 2:
            row = row + np.where(n >= (T // 2) * hop, sine, 0.0)
        if T >= 3:
            quiet = int(rng.integers(0, T))
            row[quiet * hop:(quiet + 1) * hop] = 0.0
        x[b] = row.astype(np.float32)
    return x


def zeroed_frames(x, hop):
    """x [B, T hop] -> [B, T] bool: the frames whose own samples are all zero."""
    return (np.asarray(x).reshape(x.shape[0], -1, hop) == 0).all(axis=-1)


# ------------------------------------------------------------------------------------- the device kernels' arithmetic

_f32 = nar._f32


def half_table(F):
    """[P, F]: hh[d] = h[+-d] of unit vector b, (1/2 + 1/2 cos(pi d / P)) (c_b / M) cos(2 pi b d / M)."""
    Pn, M = F - 1, 2 * (F - 1)
    d, b = np.arange(Pn), np.arange(F)
    return ((0.5 + 0.5 * np.cos(np.pi * d / Pn))[:, None] * (olar.ck(F) / M)[None, :]
            * np.cos(np.pi * ((b[None, :] * d[:, None]) % M) / Pn))


def analyse_ola_fp32(x, hop, F, average=1, iterations=ITERATIONS):
    """`noise_analysis` of finite fp32 rows x [B, T hop] in the arithmetic of the overlap-add kernels of
    csrc/ddsp_noise_analysis.hip: the tables rounded once to fp32; r an FMA chain over n, then fl(r fl(hop / c)); the frame average
    summed in ascending t' and divided once; q an FMA chain over l; hh an FMA chain over b; rho an FMA chain over e ascending, then
    fl(rho fl(hop / 3)); H0 = sqrt(fl(p fl(3 / hop))); H <- fl(H sqrt(fl(p / max(P, tiny)))).  (Products with a sample or a tap
    beyond the end are exact zeros here and absent in the kernels: the same chain.)"""
    check_args(hop, F, average, iterations)
    x = _f32(x)
    B, N = x.shape
    T, L = N // hop, F - 1
    HT = _f32(half_table(F))                                      # [P, F]
    CT = _f32(nar.cos_matrix(F))                                  # [F, L]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xp = np.concatenate([x, np.zeros((B, L))], axis=-1)
        w = xp[:, (np.arange(T) * hop)[:, None] + np.arange(hop + L - 1)[None, :]]            # [B, T, hop + L - 1]
        acc = np.zeros((B, T, L))
        for n in range(hop):
            acc = _f32(acc + w[..., n:n + 1] * w[..., n:n + L])
        c = counts(T, hop, L)
        r = np.where(c > 0, _f32(acc * _f32(_f32(hop) / np.maximum(c, 1))), 0.0)
        s = (average - 1) // 2
        rbar = np.empty_like(r)
        for t in range(T):
            lo, hi = max(0, t - s), min(T, t + s + 1)
            a = np.zeros((B, L))
            for u in range(lo, hi):
                a = _f32(a + r[:, u])
            rbar[:, t] = _f32(a / (hi - lo))
        Pm = nar._P_fp32(rbar, CT)
        p = np.where(Pm < 0, 0.0, Pm)
        H = _f32(np.sqrt(_f32(p * _f32(3.0 / hop))))
        small = float(tiny(np.float32))
        scale = _f32(hop / 3.0)
        for _ in range(iterations):
            hh = nar._fma_chain(HT, H[..., None, :])              # [B, T, P]
            h = np.concatenate([hh[..., :0:-1], hh, np.zeros((B, T, L))], axis=-1)            # h[e] at e + P - 1, zeros behind
            a = np.zeros((B, T, L))
            for i in range(2 * L - 1):
                a = _f32(a + h[..., i:i + 1] * h[..., i:i + L])
            Pm = nar._P_fp32(_f32(a * scale), CT)
            den = np.where(Pm < small, small, Pm)
            H = _f32(H * _f32(np.sqrt(_f32(p / den))))
    return H, p
