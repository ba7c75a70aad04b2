"""The definition of the noise analysis in numpy fp64, and the inputs the tests share.  `analyse_fp32` is
the same definition in the arithmetic of the device kernels (fp32 tables, every sum a chain of fp32 FMAs in the kernels' order):
tests/test_noise_analysis_host.py derives the device bound TOL_H from it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Derived in tests/test_noise_analysis_host.py::test_device_bound: the largest deviation of `analyse_fp32` from fp64 over the
# device tests' inputs, relative to each frame's max_b H, is 1.45e-6 (in p: 6.3e-7 of max_b p); TOL_H is twice that, rounded up
# to one digit, because any other summation order is as valid as the emulated one.
TOL_H = 3e-6

# (B, T, hop, F, average, iterations) of the device tests; the last one is the shape with iterations = 0
GPU_SHAPES = [(2, 12, 128, 65, 1, 16), (1, 9, 100, 33, 3, 8), (1, 5, 512, 195, 5, 4), (2, 4, 512, 257, 1, 2), (1, 1, 128, 65, 1, 16),
              (3, 40, 64, 17, 7, 16), (2, 6, 128, 33, 3, 0)]


def tiny(dtype):
    return np.finfo(dtype).tiny


# ------------------------------------------------------------------------------------------------------------ step 1: Amat

def amat(F, hop):
    """[hop, F]: the reference's amp_to_impulse_response(., hop) on unit vectors, op by op (irfft, roll by M / 2, periodic Hann
    of size M, pad to hop, roll by -M / 2).  Requires hop >= M."""
    M = 2 * (F - 1)
    if hop < M:
        raise ValueError(f"hop {hop} < 2 (F - 1) = {M}: the reference crops the impulse response, H is not identifiable")
    ir = np.fft.irfft(np.eye(F), n=M, axis=-1)                                    # [F, M]
    ir = np.roll(ir, M // 2, axis=-1) * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(M) / M))
    ir = np.concatenate([ir, np.zeros((F, hop - M))], axis=-1)
    return np.roll(ir, -(M // 2), axis=-1).T.copy()


def support(F, hop):
    """(d [M], e [M]): the non-zero rows of Amat in the order the kernels store them and their signed offsets: d = e = j for
    j < M / 2, e = j - M and d = hop + e otherwise."""
    M = 2 * (F - 1)
    j = np.arange(M)
    e = np.where(j < M // 2, j, j - M)
    return np.where(e >= 0, e, hop + e), e


def amat_rows(F, hop):
    """[M, F]: the rows `support` names, in closed form: (1/2 + 1/2 cos(2 pi e / M)) (c_b / M) cos(2 pi b e / M), c_b = 1 at
    b = 0 and F - 1, 2 otherwise."""
    M = 2 * (F - 1)
    _, e = support(F, hop)
    b = np.arange(F)
    cb = np.where((b == 0) | (b == F - 1), 1.0, 2.0)
    arg = ((b[None, :] * e[:, None]) % M) / (F - 1)
    return (0.5 + 0.5 * np.cos(2 * np.pi * e / M))[:, None] * (cb / M)[None, :] * np.cos(np.pi * arg)


# ------------------------------------------------------------------------------------------------------- steps 2 and 3

def model_R(H, hop, truncated=True):
    """H [..., F] -> R(H) [..., L]: the expected in-frame autocorrelation of a frame of FilteredNoise.  truncated=False is the
    model without the truncation weights, (hop / 3) sum_d k[d] k[d + l], which host test 2 shows to be wrong."""
    H = np.asarray(H, dtype=np.float64)
    F = H.shape[-1]
    L = F - 1
    k = H @ amat(F, hop).T                                                        # [..., hop]
    d = np.arange(hop)
    R = np.empty(H.shape[:-1] + (L,))
    for l in range(L):
        w = (hop - l - d[:hop - l]) if truncated else hop
        R[..., l] = (w * k[..., :hop - l] * k[..., l:]).sum(-1) / 3.0
    return R


def measure(x, hop, F):
    """x [..., T hop] -> r [..., T, L]: r_t[l] = sum_{n < hop - l} x[t hop + n] x[t hop + n + l]."""
    x = np.asarray(x, dtype=np.float64)
    fr = x.reshape(x.shape[:-1] + (-1, hop))
    L = F - 1
    r = np.empty(fr.shape[:-1] + (L,))
    for l in range(L):
        r[..., l] = (fr[..., :hop - l] * fr[..., l:]).sum(-1)
    return r


def average_frames(r, average):
    """r [..., T, L] -> the mean over t' in [t - s, t + s] inside [0, T), s = (average - 1) / 2."""
    if average < 1 or average % 2 == 0:
        raise ValueError(f"average must be an odd count of frames, got {average}")
    T = r.shape[-2]
    s = (average - 1) // 2
    out = np.empty_like(r)
    for t in range(T):
        out[..., t, :] = r[..., max(0, t - s):min(T, t + s + 1), :].mean(axis=-2)
    return out


# -------------------------------------------------------------------------------------------------------------- step 4

def cos_matrix(F):
    """[F, L]: c_l g[l] cos(pi b l / (F - 1)), c_0 = 1, c_l = 2, g[l] = 1/2 + 1/2 cos(pi l / L)."""
    L = F - 1
    b, l = np.arange(F), np.arange(L)
    cl = np.where(l == 0, 1.0, 2.0)
    g = 0.5 + 0.5 * np.cos(np.pi * l / L)
    return (cl * g)[None, :] * np.cos(np.pi * ((b[:, None] * l[None, :]) % (2 * L)) / L)


def smooth(q):
    """(1/4, 1/2, 1/4) with mirrored ends over the last axis."""
    ext = np.concatenate([q[..., 1:2], q, q[..., -2:-1]], axis=-1)
    return 0.25 * ext[..., :-2] + 0.5 * ext[..., 1:-1] + 0.25 * ext[..., 2:]


def P(r, F):
    return smooth(np.asarray(r, dtype=np.float64) @ cos_matrix(F).T)


# -------------------------------------------------------------------------------------------------------------- step 5

def fixed_point(rbar, hop, F, iterations):
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
    if hop < 2 * (F - 1):
        raise ValueError(f"hop {hop} < 2 (n_filters - 1) = {2 * (F - 1)}: H is not identifiable")
    if average < 1 or average % 2 == 0:
        raise ValueError(f"average must be an odd count of frames, got {average}")
    if iterations < 0:
        raise ValueError(f"iterations must be at least 0, got {iterations}")


def noise_analysis(x, hop, F, average=1, iterations=16):
    """x [..., T hop] -> (H [..., T, F], p [..., T, F])."""
    check_args(hop, F, average, iterations)
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] % hop:
        raise ValueError(f"{x.shape[-1]} samples are no whole number of frames of hop {hop}")
    with np.errstate(invalid="ignore", over="ignore"):
        return fixed_point(average_frames(measure(x, hop, F), average), hop, F, iterations)


def rel(a, b):
    """Relative l2 distance of a from b."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------------------------------------- inputs

def smooth_H(F, T=None, seed=0):
    """A smooth H: a Gaussian bump plus a slope plus a floor of 0.02; [F], or [T, F] with the bump moving and breathing."""
    b = np.arange(F) / (F - 1)
    if T is None:
        return 0.02 + 0.15 * (1 - b) + 0.8 * np.exp(-0.5 * ((b - 0.3) / 0.08) ** 2)
    rng = np.random.default_rng(seed)
    t = (np.arange(T)[:, None] + rng.uniform(0, 1)) / max(T, 2)
    centre = 0.3 + 0.25 * np.sin(2 * np.pi * (t + rng.uniform(0, 1)))
    gain = 0.5 + 0.4 * np.cos(2 * np.pi * (0.7 * t + rng.uniform(0, 1)))
    return 0.02 + 0.15 * (1 - b)[None, :] + gain * np.exp(-0.5 * ((b[None, :] - centre) / 0.08) ** 2)


def oracle_noise(H, hop, seed):
    """H [T, F] -> (x [T hop] fp64, the draws s [T, hop] in (-1, 1)): the oracle's filtered noise (oracle/torch_restatement.py)
    in fp64 with seeded injected uniform draws."""
    import torch
    from oracle import torch_restatement as oracle
    H = np.asarray(H, dtype=np.float64)
    u = np.random.default_rng(seed).random((H.shape[0], hop))
    y = oracle.filtered_noise(torch.from_numpy(H)[None], hop, uniform=torch.from_numpy(u)[None])
    return y[0].numpy().astype(np.float64), 2 * u - 1


def gpu_rows(shape, seed=0):
    """The device tests' rows [B, T hop] (fp32): oracle-filtered noise of a smooth, time-varying H with one silent frame per
    row (where there are at least three frames); the last row of a batch is a sine instead, and a batch of one row has the sine
    added to the second half of its frames."""
    B, T, hop, F, _, _ = shape
    rng = np.random.default_rng(2000 + seed)
    x = np.empty((B, T * hop), dtype=np.float32)
    n = np.arange(T * hop)
    for b in range(B):
        row, _ = oracle_noise(smooth_H(F, T, seed=10 * seed + b), hop, seed=100 * seed + b + 1)
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


# ------------------------------------------------------------------------------------- the device kernels' arithmetic

def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _fma_chain(a, b):
    """sum over the LAST axis of a * b as the kernels do it: one fp32 FMA per term, ascending.  fp64 arrays holding fp32 values
    (a product of two is exact in fp64)."""
    acc = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape)
    for i in range(a.shape[-1]):
        acc = _f32(acc + a[..., i] * b[..., i])
    return acc


def _P_fp32(r, CT):
    """r [..., L], CT [F, L] (fp32 values) -> fl(0.25 fl(q[b - 1] + q[b + 1]) + 0.5 q[b]) of the fp32 FMA chains q."""
    q = _fma_chain(CT, r[..., None, :])
    ext = np.concatenate([q[..., 1:2], q, q[..., -2:-1]], axis=-1)
    return _f32(0.25 * _f32(ext[..., :-2] + ext[..., 2:]) + 0.5 * ext[..., 1:-1])


def analyse_fp32(x, hop, F, average=1, iterations=16):
    """`noise_analysis` of fp32 rows x [B, T hop] in the arithmetic of csrc/ddsp_noise_analysis.hip: the tables rounded once to
    fp32; r an FMA chain over n; the frame average summed in ascending t' and divided once; q an FMA chain over l; k an FMA
    chain over b; R an FMA chain of (hop - l - d) fl(k[d] k[d + l]) over the stored rows in their order, then fl(R / 3 as
    fl(1/3)); H0 = sqrt(fl(p fl(3 / hop))); H <- fl(H sqrt(fl(p / max(P, tiny))))."""
    check_args(hop, F, average, iterations)
    x = _f32(x)
    B = x.shape[0]
    fr = x.reshape(B, -1, hop)
    T, L, M = fr.shape[1], F - 1, 2 * (F - 1)
    A = _f32(amat_rows(F, hop))                                   # [M, F]
    CT = _f32(cos_matrix(F))                                      # [F, L]
    dpos, _ = support(F, hop)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.zeros((B, T, L))
        for l in range(L):
            r[..., l] = _fma_chain(fr[..., :hop - l], fr[..., l:])
        s = (average - 1) // 2
        rbar = np.empty_like(r)
        for t in range(T):
            lo, hi = max(0, t - s), min(T, t + s + 1)
            acc = np.zeros((B, L))
            for u in range(lo, hi):
                acc = _f32(acc + r[:, u])
            rbar[:, t] = _f32(acc / (hi - lo))
        Pm = _P_fp32(rbar, CT)
        p = np.where(Pm < 0, 0.0, Pm)
        H = _f32(np.sqrt(_f32(p * _f32(3.0 / hop))))
        small = float(tiny(np.float32))
        third = _f32(1.0 / 3.0)
        ls = np.arange(L)
        for _ in range(iterations):
            kc = _fma_chain(A, H[..., None, :])                   # [B, T, M]
            k = np.zeros((B, T, hop + L))                         # (the tail is never read with a non-zero weight)
            k[..., dpos] = kc
            acc = np.zeros((B, T, L))
            for j in range(M):
                d = int(dpos[j])
                w = np.maximum(hop - ls - d, 0)                   # lanes past their last d add nothing
                acc = np.where(w > 0, _f32(acc + w * _f32(k[..., d:d + 1] * k[..., d:d + L])), acc)
            R = _f32(acc * third)
            Pm = _P_fp32(R, CT)
            den = np.where(Pm < small, small, Pm)
            H = _f32(H * _f32(np.sqrt(_f32(p / den))))
    return H, p
