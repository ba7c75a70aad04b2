"""The MFCC front end (ddsp_pytorch_amd.encoder.mfcc) restated in fp64 as plain numpy loops, with a forward
error bound for every element, and the inputs the MFCC tests share.

Definition (x [B, L] fp32 -> mfcc [B, F, n_mfcc], logmel [B, F, n_mels], F = (L - n_fft) // hop + 1):
    y_f[n]    = x[f hop + n] w[n],  w[n] = fl32(0.5 - 0.5 cos(2 pi n / n_fft))              (frames are not centred)
    A[k]      = |DFT(y_f)[k]| s,    s = fl32(2 / sum w)
    mel[m]    = sum_k W[m, k] A[k]                                                           (W: fl32 of the fp64 HTK-mel triangles)
    logmel[m] = log(mel[m] + floor)
    mfcc[j]   = sum_m D[j, m] logmel[m],  D[j, m] = fl32(sqrt(2 / n_mels) cos(pi j (m + 1/2) / n_mels))
A frame with a NaN or an infinite sample is NaN in both outputs.

Error bound of an fp32 evaluation, per element (E = ||y_f||_2 in fp64, eps = 2^-24):
    d_mel[m]    <= c eps (log2(n_fft) E s sum_k W[m, k] + mel[m])
    d_logmel[m] <= d_mel[m] / (mel[m] + floor) + c eps |logmel[m]|
    d_mfcc[j]   <= sum_m |D[j, m]| d_logmel[m] + c eps sum_m |D[j, m] logmel[m]|
`reference` returns the bounds for c = 1; a caller multiplies.

The constant: C_CPU is the smallest c (rounded up to two digits) at which the CPU fp32 torch evaluation of the definition
(encoder.mfcc on CPU tensors: torch.fft.rfft and two matmuls) passes on every input of `cases()` and `big_case()`; the kernel
does the same arithmetic in another order and gets KERNEL_FACTOR times that.  Neither number comes from the kernel.
Re-measure with `python tests/mfcc_reference.py` (prints the worst ratio over all cases; no GPU needed).
"""
import functools
import itertools
import math

import numpy as np

C_CPU = 8.1                  # measured 8.0891 (an all-zero frame's coefficients at n_fft 64, 128 bands: the 128-term sum of the DCT)
KERNEL_FACTOR = 3.0
EPS = 2.0 ** -24
SAMPLE_RATE = 16000
FLOOR = 1e-5


# ---------------------------------------------------------------------------------------------------------------- tables
@functools.lru_cache(maxsize=None)
def hann(n_fft):
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * n / n_fft) for n in range(n_fft)], dtype=np.float64).astype(np.float32)


def hz_to_mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


@functools.lru_cache(maxsize=None)
def filterbank(n_fft, sample_rate, n_mels, fmin, fmax):
    """dense [n_mels, n_fft / 2 + 1] fp32, element by element (cached: treat the tables as read-only)"""
    bins = n_fft // 2 + 1
    lo, hi = hz_to_mel(fmin), hz_to_mel(min(fmax, sample_rate / 2.0))
    edges = [lo + (hi - lo) * i / (n_mels + 1) for i in range(n_mels + 2)]
    W = np.zeros((n_mels, bins), dtype=np.float64)
    for m in range(n_mels):
        l, c, r = edges[m], edges[m + 1], edges[m + 2]
        for k in range(1, bins):                           # bin 0 has weight 0
            mk = hz_to_mel(k * sample_rate / n_fft)
            W[m, k] = max(0.0, min((mk - l) / (c - l), (r - mk) / (r - c)))
    return W.astype(np.float32)


@functools.lru_cache(maxsize=None)
def dct(n_mels, n_mfcc):
    D = np.zeros((n_mfcc, n_mels), dtype=np.float64)
    for j in range(n_mfcc):
        for m in range(n_mels):
            D[j, m] = math.sqrt(2.0 / n_mels) * math.cos(math.pi * j * (m + 0.5) / n_mels)
    return D.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- reference
def spectrum(x, n_fft, hop):
    """x [B, L] -> (A [B, F, bins] fp64, E [B, F], dead [B, F]).  The DFT is numpy's fp64 transform of every frame alone."""
    x = np.asarray(x, dtype=np.float32)
    B, L = x.shape
    F = (L - n_fft) // hop + 1
    w = hann(n_fft).astype(np.float64)
    s = float(np.float32(2.0 / w.sum()))
    A = np.zeros((B, F, n_fft // 2 + 1))
    E = np.zeros((B, F))
    dead = np.zeros((B, F), dtype=bool)
    for b in range(B):
        for f in range(F):
            frame = x[b, f * hop:f * hop + n_fft].astype(np.float64)
            if not np.all(np.isfinite(frame)):
                dead[b, f] = True
                continue
            y = frame * w
            A[b, f] = np.abs(np.fft.rfft(y)) * s
            E[b, f] = math.sqrt(float(np.dot(y, y)))
    return A, E, dead, s


def from_spectrum(spec, n_fft, sample_rate, n_mels, n_mfcc, fmin=20.0, fmax=8000.0, floor=FLOOR):
    """-> dict(mfcc, logmel: fp64 values, NaN in dead frames; bound_mfcc, bound_logmel: the bounds for c = 1; dead)"""
    A, E, dead, s = spec
    B, F, bins = A.shape
    W = filterbank(n_fft, sample_rate, n_mels, fmin, fmax).astype(np.float64)
    D = dct(n_mels, n_mfcc).astype(np.float64)
    floor = float(np.float32(floor))
    mel = np.zeros((B, F, n_mels))
    for m in range(n_mels):
        for k in np.nonzero(W[m])[0]:                      # ascending k
            mel[..., m] += W[m, k] * A[..., k]
    d_mel = EPS * (math.log2(n_fft) * E[..., None] * s * W.sum(axis=1)[None, None] + mel)
    logmel = np.log(mel + floor)
    d_logmel = d_mel / (mel + floor) + EPS * np.abs(logmel)
    mfcc = np.zeros((B, F, n_mfcc))
    d_mfcc = np.zeros((B, F, n_mfcc))
    for m in range(n_mels):                                # ascending m, every coefficient j at once
        mfcc += D[:, m] * logmel[..., m, None]
        d_mfcc += np.abs(D[:, m]) * d_logmel[..., m, None] + EPS * np.abs(D[:, m] * logmel[..., m, None])
    mfcc[dead] = np.nan
    logmel[dead] = np.nan
    return dict(mfcc=mfcc, logmel=logmel, bound_mfcc=d_mfcc, bound_logmel=d_logmel, dead=dead)


def reference(x, n_fft, hop, sample_rate, n_mels=128, n_mfcc=30, fmin=20.0, fmax=8000.0, floor=FLOOR):
    return from_spectrum(spectrum(x, n_fft, hop), n_fft, sample_rate, n_mels, n_mfcc, fmin, fmax, floor)


def worst_ratio(got_mfcc, got_logmel, ref):
    """max |got - ref| / bound(c = 1) over the live frames of both outputs (logmel may be None); dead frames must be NaN
    everywhere, live frames nowhere.  -> (ratio, where)"""
    dead = ref["dead"]
    worst, where = 0.0, None
    for name, got in (("mfcc", got_mfcc), ("logmel", got_logmel)):
        if got is None:
            continue
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == ref[name].shape, (name, got.shape, ref[name].shape)
        assert np.all(np.isnan(got[dead])), f"{name}: a frame with a non-finite sample must be NaN everywhere"
        assert not np.any(np.isnan(got[~dead])), f"{name}: NaN in a frame whose samples are finite"
        ratio = np.abs(got[~dead] - ref[name][~dead]) / ref["bound_" + name][~dead]
        if ratio.size and float(ratio.max()) > worst:
            worst, where = float(ratio.max()), (name, tuple(int(i) for i in np.argwhere(~dead)[int(ratio.argmax()) // got.shape[-1]]))
    return worst, where


# ------------------------------------------------------------------------------------------------------------------ inputs
N_FFTS = (64, 128, 256, 512, 1024, 2048)
FRAMES = (1, 2, 3, 5)
MEL_PAIRS = ((8, 1), (40, 1), (40, 13), (40, 30), (128, 1), (128, 13), (128, 30), (128, 64))    # (n_mels, n_mfcc <= n_mels)


def hops(n_fft):
    return (n_fft // 4, n_fft, 3)


def noise_input(n_fft, F, hop, seed=0):
    """[2, L] noise at full scale; L leaves a few samples after the last frame (they belong to no frame)"""
    rng = np.random.default_rng([n_fft, F, hop, seed])
    L = n_fft + (F - 1) * hop + min(hop - 1, 2)
    return rng.uniform(-1.0, 1.0, (2, L)).astype(np.float32)


def content_inputs(n_fft):
    """name -> x [2, F n_fft] for hop = n_fft (frames do not overlap, so each has a level of its own)"""
    rng = np.random.default_rng([n_fft, 77])
    n = np.arange(n_fft)
    out = {}
    # a full-scale sine on a bin centre, 3 frames; the second row on another bin and quieter
    sine = np.stack([np.tile(np.sin(2 * np.pi * (n_fft // 8) * n / n_fft), 3), 0.25 * np.tile(np.cos(2 * np.pi * 5 * n / n_fft), 3)])
    out["sine"] = sine.astype(np.float32)
    # a frame at 1e-6 beside a frame at 1 (both orders; 4 frames and 3: the last quiet frame is paired with zeros)
    loud = rng.uniform(-1.0, 1.0, (2, 4, n_fft))
    loud[0, 0] *= 1e-6
    loud[0, 3] *= 1e-6
    loud[1, 1] *= 1e-6
    loud[1, 2] *= 1e-6
    out["quiet_beside_loud"] = loud.reshape(2, -1).astype(np.float32)
    # an all-zero frame beside a loud one
    zero = rng.uniform(-1.0, 1.0, (2, 3, n_fft))
    zero[0, 1] = 0.0
    zero[1, 0] = 0.0
    zero[1, 2] = 0.0
    out["zero_beside_loud"] = zero.reshape(2, -1).astype(np.float32)
    # a NaN and an infinite sample in one frame: row 0's frame 0 (its partner is frame 1), row 1's frame 2 (paired with zeros)
    bad = rng.uniform(-1.0, 1.0, (2, 3, n_fft))
    bad[0, 0, 3] = np.nan
    bad[0, 0, n_fft // 2] = np.inf
    bad[1, 2, 0] = -np.inf
    bad[1, 2, n_fft - 1] = np.nan
    out["non_finite"] = bad.reshape(2, -1).astype(np.float32)
    return out


def cases():
    """(name, x, n_fft, hop, [(n_mels, n_mfcc), ...]) for every input of tests/test_mfcc_host.py and tests/test_gpu_mfcc.py but
    the long one (big_case)."""
    for n_fft in N_FFTS:
        for F, hop in itertools.product(FRAMES, hops(n_fft)):
            yield f"noise-{n_fft}-{F}-{hop}", noise_input(n_fft, F, hop), n_fft, hop, MEL_PAIRS
        for name, x in content_inputs(n_fft).items():
            yield f"{name}-{n_fft}", x, n_fft, n_fft, ((128, 30), (40, 13))


BIG = dict(n_fft=64, hop=16, samples=2_100_000, n_mels=40, n_mfcc=13)      # 65 623 frame pairs: 8 203 units, over the cap of 8 192 blocks


def big_case():
    rng = np.random.default_rng(2100)
    x = rng.uniform(-1.0, 1.0, (1, BIG["samples"])).astype(np.float32)
    x[0, 1_000_000:1_000_400] = 0.0                       # some all-zero frames on the way
    return x


def big_reference(x):
    """`reference` for the long row without its per-frame Python loops"""
    n_fft, hop = BIG["n_fft"], BIG["hop"]
    w = hann(n_fft).astype(np.float64)
    s = float(np.float32(2.0 / w.sum()))
    F = (x.shape[1] - n_fft) // hop + 1
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None]
    y = x[0].astype(np.float64)[idx] * w
    spec = (np.abs(np.fft.rfft(y, axis=-1))[None] * s, np.sqrt((y * y).sum(-1))[None], np.zeros((1, F), dtype=bool), s)
    return from_spectrum(spec, n_fft, SAMPLE_RATE, BIG["n_mels"], BIG["n_mfcc"])


if __name__ == "__main__":
    import os
    import sys

    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ddsp_pytorch_amd as ddsp

    worst = (0.0, None)
    for name, x, n_fft, hop, pairs in cases():
        spec = spectrum(x, n_fft, hop)
        for n_mels, n_mfcc in pairs:
            ref = from_spectrum(spec, n_fft, SAMPLE_RATE, n_mels, n_mfcc)
            got, lm = ddsp.mfcc(torch.from_numpy(x), n_fft, hop, SAMPLE_RATE, n_mels=n_mels, n_mfcc=n_mfcc, return_logmel=True)
            r, where = worst_ratio(got.numpy(), lm.numpy(), ref)
            if r > worst[0]:
                worst = (r, (name, n_mels, n_mfcc, where))
    x = big_case()
    got, lm = ddsp.mfcc(torch.from_numpy(x), BIG["n_fft"], BIG["hop"], SAMPLE_RATE, n_mels=BIG["n_mels"], n_mfcc=BIG["n_mfcc"], return_logmel=True)
    r, where = worst_ratio(got.numpy(), lm.numpy(), big_reference(x))
    if r > worst[0]:
        worst = (r, ("big", where))
    print(f"CPU fp32 evaluation: worst |error| / bound(c = 1) = {worst[0]:.4f} at {worst[1]}; C_CPU in this file: {C_CPU}")
