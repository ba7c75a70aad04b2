"""TEST INFRASTRUCTURE ONLY -- fp64 definition of the filtered noise's forward (the truncated per-frame convolution of
ddsp_noise_forward_ws; reference: model/ddsp/filtered_noise.py:7-53) and its yardsticks, in numpy.

Per frame f, with R = hop, S = 2(F-1), half = S/2:

    x[d]    = fp32(u[d] * 2 - 1), widened                      (the injected draw, or oracle.philox_uniform at seed / offset)
    z[n]    = (1/S) sum_k c_k H[k] cos(2 pi ((k n) mod S) / S)   c_k = 1 for k in {0, F-1}, else 2
    kern[j] = z[(src - half) mod S] * hann32[src]   where src = (j + half) mod R < S, else 0
    y[n]    = sum_{m <= n} x[m] kern[n - m]                      n in [0, R)
    A       = (1/S) sum_k c_k |H[k]|;   kabs[j] = A * hann32[src] (same support)
    Y[n]    = sum_{m <= n} |x[m]| kabs[n - m]                    the per-sample yardstick
    Yframe  = max_n Y[n];   peak = max_n |y[n]|

hann32 is the fp32 periodic Hann value of oracle/ddsp_oracle.c: frame_impulse (noise_grad_reference.hann32).  |z[n]| <= A, so
|y[n]| <= Y[n], and Y[n] bounds every rounding term an fp32 evaluation incurs on the way to y[n] up to a factor of epsilon times the
depth.  y and Y are direct sums, lag by lag (no FFT, whose rounding leaves a residue where every term is 0): Y is exactly 0 where y
is -- at the first sample of a frame cropped to a divisor of S/2 (its tap at lag 0 is hann32[0] == 0) a correct kernel returns an
exact zero and any other value fails.  A non-finite H[f, k] makes z, and with kern[0] every y[n], of frame f non-finite, and
touches no other frame.

Two fp32 evaluations of the same definition, from which tests/test_noise_fwd_reference_host.py derives TOL_SAMPLE and TOL_FRAME:
`direct_fp32` (z a chain of fp32 multiply-adds over k, the convolution a chain over m: the arithmetic class of the Batched, Frame and
Wave kernels) and `fft_fp32` (the reference module's own fp32 FFT pipeline in torch on the CPU: the class of the Fft forms).

Memory stays bounded: at most CHUNK_ELEMS samples of frames are convolved at a time (chunks run on a few threads; numpy releases
the GIL inside its loops).  Nothing under ddsp-pytorch_amd/ may import this module.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from noise_grad_reference import draw, hann32, ratio  # noqa: F401  (ratio: re-exported for the tests)

CHUNK_ELEMS = 1 << 15          # frames x hop per chunk: three fp64 arrays of it stay in a core's cache
THREADS = max(1, min(8, os.cpu_count() or 1))

# Derived in tests/test_noise_fwd_reference_host.py::test_device_bounds (figures there and in DESIGN.md section 5): twice the largest
# deviation of the fp32 evaluations from fp64 on GPU_SHAPES relative to the yardstick, rounded up to one digit -- TOL_SAMPLE from
# direct_fp32 per sample against Y[n], plus the cosines' definitional term at the one shape whose kernel still rounds an fp32 cosine
# (the wavefront form, hop 128 / 65 bands); TOL_FRAME from fft_fp32 per frame against Yframe.
TOL_SAMPLE = 3e-6             # of Y[n]: the Batched, Frame and Wave kernels
TOL_FRAME = 5e-7              # of Yframe: every form
FRAME_REL = 2e-6               # the project's noise contract, relative to each frame's own fp64 peak
FRAME_FLOOR = 1e-3             # ... exempt: frames with peak < FRAME_FLOOR * Yframe

# (B, T, hop, F, family) of tests/test_gpu_noise_forward.py: every (hop, F) it runs, at its own (B, T) -- but at most DERIVE_FRAMES
# frames (the figures are per frame: more frames of a shape add draws, not arithmetic).  family: "direct" or "fft".
DERIVE_FRAMES = 48
GPU_SHAPES = [
    (3, 7, 512, 257, "fft"), (3, 21, 512, 195, "fft"), (3, 7, 512, 129, "fft"), (3, 7, 512, 256, "fft"), (3, 7, 512, 3, "fft"),
    (1, 1, 512, 257, "fft"), (3, 7, 256, 129, "fft"), (3, 7, 256, 100, "fft"), (3, 7, 256, 65, "fft"),
    (1, 48, 512, 193, "fft"), (1, 48, 512, 195, "fft"), (1, 48, 512, 224, "fft"),
    (2, 24, 128, 65, "direct"),
    (1, 67, 8, 2, "direct"), (2, 33, 16, 9, "direct"), (3, 29, 8, 65, "direct"), (1, 100, 40, 33, "direct"), (2, 35, 128, 64, "direct"),
    (1, 47, 64, 129, "direct"), (2, 9, 160, 65, "direct"), (1, 17, 256, 129, "direct"), (3, 7, 256, 128, "direct"),
    (2, 13, 512, 101, "direct"), (3, 5, 512, 257, "direct"), (2, 9, 512, 195, "direct"), (1, 9, 1024, 1025, "direct"),
    (2, 4, 1, 9, "direct"), (2, 4, 3, 5, "direct"), (3, 2, 7, 33, "direct"), (2, 3, 12, 65, "direct"), (3, 2, 100, 33, "direct"),
    (2, 2, 441, 129, "direct"), (1, 2, 2048, 1025, "direct"), (1, 2, 8192, 129, "direct"),
]


def ck(F: int) -> np.ndarray:
    c = np.full(F, 2.0)
    c[0] = c[F - 1] = 1.0
    return c


def tap_map(F: int, R: int):
    """Taps that reach the impulse response: (j [M], z index n [M], window [M]) for every j in [0, R) with src < S."""
    S = 2 * (F - 1)
    half = S // 2
    j = np.arange(R)
    src = (j + half) % R
    keep = src < S
    src = src[keep]
    return j[keep], (src - half) % S, hann32(S)[src]


def impulse_fp64(H, R: int):
    """H [N, F] -> (kern [N, R], kabs [N, R]) in fp64."""
    H = np.asarray(H, dtype=np.float64)
    N, F = H.shape
    S = 2 * (F - 1)
    table = np.cos(2.0 * np.pi * np.arange(S) / S)
    C = table[(np.arange(F)[:, None] * np.arange(S)[None, :]) % S] * (ck(F) / S)[:, None]        # [F, S]
    kern = np.zeros((N, R))
    kabs = np.zeros((N, R))
    jm, nm, wm = tap_map(F, R)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(H).all(axis=1)
        z = np.full((N, S), np.nan)
        z[fin] = H[fin] @ C                                       # (a non-finite H: its whole frame, and only its own)
        A = (np.abs(H) * ck(F)).sum(axis=1) / S
        A[~fin] = np.nan
        kern[:, jm] = z[:, nm] * wm
        kabs[:, jm] = A[:, None] * wm
    return kern, kabs


def _convolve_chunk(args):
    x, kern, kabs = args
    R = x.shape[1]
    y = np.zeros_like(x)
    Y = np.zeros_like(x)
    ax = np.abs(x)
    lags = np.flatnonzero((kabs != 0.0).any(axis=0) | (kern != 0.0).any(axis=0))     # (NaN != 0: a non-finite frame keeps its lags)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in lags:
            y[:, j:] += kern[:, j:j + 1] * x[:, :R - j]
            Y[:, j:] += kabs[:, j:j + 1] * ax[:, :R - j]
    return y, Y


def noise_fwd_fp64(H, hop: int, uniform=None, seed: int = 0, offset: int = 0):
    """H [B,T,F] (taken as fp32) -> (y [B,T,hop], Y [B,T,hop]) in fp64 for the draw `uniform` [B,T,hop], or the in-kernel stream of
    (seed, offset) when `uniform` is None (the offset including the value of a device counter where one is used)."""
    H = np.ascontiguousarray(H, dtype=np.float32)
    B, T, F = H.shape
    assert F >= 2 and hop >= 1
    R = hop
    x = draw(B, T, hop, uniform, seed, offset).reshape(B * T, R).astype(np.float64)
    Hf = H.reshape(B * T, F)
    step = max(1, CHUNK_ELEMS // R)
    jobs = []
    for f0 in range(0, B * T, step):
        kern, kabs = impulse_fp64(Hf[f0:f0 + step], R)
        jobs.append((x[f0:f0 + step], kern, kabs))
    if len(jobs) > 1 and THREADS > 1:
        with ThreadPoolExecutor(THREADS) as pool:
            parts = list(pool.map(_convolve_chunk, jobs))
    else:
        parts = [_convolve_chunk(j) for j in jobs]
    y = np.concatenate([p[0] for p in parts]).reshape(B, T, R)
    Y = np.concatenate([p[1] for p in parts]).reshape(B, T, R)
    return y, Y


def frame_figures(y, Y):
    """(Yframe [B,T], peak [B,T]); NaN for a non-finite frame."""
    return Y.max(axis=-1), np.abs(y).max(axis=-1)


# ---------------------------------------------------------------------------------------------------- the fp32 evaluations

def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _cos_table(S: int, ulps: int = 0):
    """fl32 cos(2 pi m / S), m in [0, S), as fp64 values; `ulps` moves every entry by that many fp32 ulps (the kernels' cospif is not
    a correctly rounded fp64 cosine: test_device_bounds measures what one ulp on every cosine is worth)."""
    ct = np.cos(2.0 * np.pi * np.arange(S) / S).astype(np.float32)
    exact = np.abs(ct) == 1.0                                     # cos(0), cos(pi): exact in any implementation, cospif included
    for _ in range(abs(ulps)):
        ct = np.where(exact, ct, np.nextafter(ct, np.float32(np.inf if ulps > 0 else -np.inf)))
    return ct.astype(np.float64)


def direct_fp32(H, hop: int, uniform=None, seed: int = 0, offset: int = 0, ulps: int = 0):
    """The definition as noise_frame_kernel (csrc/ddsp_noise.hip) evaluates it: an fp32 cosine table, z a chain of fp32 multiply-adds
    over k = 1 .. F-2 added to H[0] +- H[F-1], the window 0.5 - 0.5 ct[src] in fp32, the convolution a chain of fp32 multiply-adds over
    m ascending.  -> y [B,T,hop], fp64 values of fp32 numbers.  (Each multiply-add is an exact product added and rounded once to fp32
    through fp64: a double rounding that differs from a fused multiply-add in about one case in 2^29.)"""
    H = np.ascontiguousarray(H, dtype=np.float32)
    B, T, F = H.shape
    R, S = hop, 2 * (F - 1)
    half = S // 2
    N = B * T
    x = draw(B, T, hop, uniform, seed, offset).reshape(N, R).astype(np.float64)
    Hf = H.reshape(N, F).astype(np.float64)
    ct = _cos_table(S, ulps)
    jm, nm, _ = tap_map(F, R)
    src = (jm + half) % R
    acc = np.zeros((N, len(nm)))
    for k in range(1, F - 1):
        acc = _f32(acc + Hf[:, k:k + 1] * ct[(k * nm) % S])
    sign = np.where(nm % 2 == 1, -1.0, 1.0)
    v = _f32(_f32(2.0 * acc + _f32(Hf[:, 0:1] + sign * Hf[:, F - 1:F])) * _f32(1.0 / S))
    win = _f32(0.5 - _f32(0.5 * ct[src]))
    kern = np.zeros((N, R))
    kern[:, jm] = _f32(v * win)
    y = np.zeros((N, R))
    for m in range(R):
        y[:, m:] = _f32(y[:, m:] + x[:, m:m + 1] * kern[:, :R - m])
    return y.reshape(B, T, R)


def fft_fp32(H, hop: int, uniform=None, seed: int = 0, offset: int = 0):
    """The reference module's own pipeline in fp32 torch on the CPU (oracle/torch_restatement.py: irfft -> roll -> hann_window ->
    pad or crop -> roll, then rfft / irfft of the padded pair), on the same draw.  -> y [B,T,hop] as fp64 values."""
    import torch
    from oracle import oracle, torch_restatement
    H = np.ascontiguousarray(H, dtype=np.float32)
    B, T, F = H.shape
    if uniform is None:
        uniform = oracle.philox_uniform(seed, offset, B, T, hop)
    u = torch.from_numpy(np.ascontiguousarray(uniform, dtype=np.float32))
    y = torch_restatement.filtered_noise(torch.from_numpy(H), hop, uniform=u)
    return y.numpy().astype(np.float64).reshape(B, T, hop)


# ------------------------------------------------------------------------------------------------------------------ inputs

def gpu_H(B, T, F, seed, zero=True):
    """H [B,T,F] of the device tests: the controller heads' value range on N(0,1) at per-frame levels over seven decades, one
    exactly-zero frame wherever there is more than one frame."""
    from ddsp_pytorch_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    H = syn.controller_range(rng.standard_normal((B, T, F), dtype=np.float32))
    H *= (10.0 ** rng.uniform(-4, 3, size=(B, T, 1))).astype(np.float32)          # (fuzz_parity.frame_levels)
    if zero and B * T > 1:
        H.reshape(B * T, F)[(B * T) // 2] = 0.0
    return H


def gpu_uniform(B, T, hop, seed):
    return np.random.default_rng(seed + 1).random((B, T, hop), dtype=np.float32)


def derive_shape(shape):
    """(B, T, hop, F, family) -> the same with at most DERIVE_FRAMES frames."""
    B, T, hop, F, fam = shape
    if B * T > DERIVE_FRAMES:
        B, T = 1, DERIVE_FRAMES
    return B, T, hop, F, fam
