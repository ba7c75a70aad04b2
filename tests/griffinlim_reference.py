"""fp64 reference, designed inputs, shapes and error bounds for the three launches of a Griffin-Lim iteration
(csrc/ddsp_griffinlim.hip: synthesis, overlap-add, analysis), as the test hook ddsp_griffinlim_stage (include/ddsp_hip.h) runs them
one at a time.  Used by tests/test_gpu_griffinlim_stages.py and tests/fuzz_parity.py (on the device) and
tests/test_griffinlim_reference_host.py (the reference and the bounds themselves, without a device).

The reference is numpy in float64 / complex128, in the kernels' frame-major layout: S [B, T, F], spectra [B, T, F] complex,
frames [B, T, n_fft], y [B, L].  Every bound is a function whose docstring holds its derivation from the unit roundoff
U = 2^-24 and counted operations; the transforms' own bounds are those of tests/wave_fft_reference.py.  The last section is the
stock fp32 formulation on the CPU (torch.fft / torch.stft in fp32, spectral._stock_loop's normalisation): the yardstick the
sharp criterion measures -- at most CPU_FACTOR times its error on the same inputs -- and the proof, on the host, that the
bounds are attainable without the code under test."""
import math

import numpy as np

from wave_fft_reference import CPU_FACTOR, U, fft_ceiling, real2048_ceiling  # noqa: F401  (re-exported)

SYNTH, OVERLAP, ANALYSIS = 0, 1, 2          # DDSP_GL_STAGE_*
EINVAL, ERANGE, EPERM = -1, -2, -3
SIZES = (64, 128, 256, 512, 1024, 2048)
PAIR_BT = {64: 8, 128: 4, 256: 2, 512: 1, 1024: 1}      # pairs of frames per wavefront (ddsp_wave_fft.h: PairUnit<N>::BT)
MAX_UNITS = 16384                                        # kMaxBlocks: the transform kernels stride beyond this many units
MAX_OVERLAP_THREADS = 65536 * 256                        # the overlap kernel strides beyond this many samples

G27 = ("n2048_h256", "n1024_h128_p2", "n512_h64", "n512_w400_h100")


def frames_per_unit(n_fft):
    return 1 if n_fft == 2048 else 2 * PAIR_BT[n_fft]


# ---- windows, envelope, shapes ----------------------------------------------------------------------------------------------
def hann(win_length):
    """torch.hann_window(win_length) (periodic), in float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)


def padded(window, n_fft):
    """`window` zero-padded and centred to n_fft, as torch.stft pads a win_length window."""
    window = np.asarray(window, dtype=np.float64)
    left = (n_fft - window.shape[0]) // 2
    return np.concatenate([np.zeros(left), window, np.zeros(n_fft - window.shape[0] - left)])


def natural_length(n_fft, hop, T):
    """Retained samples the overlap-added signal covers: istft keeps [n_fft/2, n_fft/2 + L) of n_fft + hop (T - 1) samples."""
    return n_fft // 2 + hop * (T - 1)


def envelope(window, hop, T, L):
    """istft's window envelope at the retained samples j < min(L, natural length): sum over the covering frames of window^2;
    1 past the natural length (never read; what spectral.py pads with)."""
    n = window.shape[0]
    full = np.zeros(n + hop * (T - 1))
    for t in range(T):
        full[t * hop:t * hop + n] += np.asarray(window, dtype=np.float64) ** 2
    env = np.ones(L)
    m = min(L, natural_length(n, hop, T))
    env[:m] = full[n // 2:n // 2 + m]
    return env


# (name, n_fft, hop, win_length or 0: rectangular n_fft window, B, T, L - hop (T - 1)).  B T = 21 frames: a last unit with fewer
# than BT pairs (16, 8, 4, 2, 2 frames a unit), a last pair with one frame, and (T odd) a pair whose frames lie in two rows.
def _shapes():
    out = []
    for n in SIZES:
        out.append((f"n{n}_hann", n, n // 4, n, 3, 7, 0))
        out.append((f"n{n}_w{3 * n // 4 + 2}_ragged", n, n // 4, 3 * n // 4 + 2, 3, 7, n // 4 - 1))      # L = hop (T - 1) + hop - 1
        # L = n_fft / 2 + 1 and a hop that does not divide n_fft / 2: every frame starts before 0, all but the first end behind L
        out.append((f"n{n}_shortest", n, 3 * n // 16, n, 2, 3, n // 2 + 1 - 2 * (3 * n // 16)))
    out.append(("n2048_h512_L3072", 2048, 512, 2048, 2, 7, 0))       # frame 4 ends exactly at L: the in-row path with equality
    out.append(("n2048_h512_L3071", 2048, 512, 2048, 2, 6, 511))     # the same frame takes the reflected path
    out.append(("n64_rect_zero_tail", 64, 64, 0, 3, 5, 50))          # L = 4 * 64 + 50: 18 samples past the natural length
    out.append(("n256_rect_hop_n", 256, 256, 0, 2, 4, 0))
    return tuple(out)


GPU_SHAPES = _shapes()
SHAPE_BY_NAME = {s[0]: s for s in GPU_SHAPES}


def shape_setup(shape):
    """-> dict(n_fft, hop, win_length, B, T, L, window [n_fft] float64 as rounded to fp32, env [L] float64 as rounded to fp32)."""
    _, n, hop, wl, B, T, extra = shape
    L = hop * (T - 1) + extra
    assert 1 + L // hop == T and L > n // 2, shape
    w = np.ones(n) if wl == 0 else padded(hann(wl), n)
    w = w.astype(np.float32).astype(np.float64)
    env = envelope(w, hop, T, L).astype(np.float32).astype(np.float64)
    return dict(n_fft=n, hop=hop, win_length=wl or n, B=B, T=T, L=L, window=w, env=env)


def f32(x):
    """x rounded to what the device is given, back in float64 / complex128."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return x.astype(np.complex64).astype(np.complex128)
    return x.astype(np.float32).astype(np.float64)


def random_state(seed, B, T, n_fft, c):
    """S, ang0, R, Rprev [B, T, F] as rounded to fp32: magnitudes of very different sizes, unit angles, two unrelated spectra."""
    rng = np.random.default_rng(seed)
    F = n_fft // 2 + 1
    S = f32(rng.random((B, T, F)) ** 2 + 0.01)
    ang0 = f32(np.exp(2j * np.pi * rng.random((B, T, F))))
    R = f32(rng.standard_normal((B, T, F)) + 1j * rng.standard_normal((B, T, F)))
    Rprev = f32(rng.standard_normal((B, T, F)) + 1j * rng.standard_normal((B, T, F)))
    return S, ang0, R, Rprev


def designed_state(seed, B, T, n_fft):
    """The inputs of the conditioning test: |R| in [0.5, 2] with random phases; Rprev = R rho e^(i phi), rho in [0.25, 1],
    phi in [pi/2, 3 pi/2] (c Rprev points away from R: |a| >= |R|, kappa <= 2) -- except every 16th bin, where
    Rprev = (R / c)(1 + eps e^(i psi)), eps = 2^-6 .. 2^-14 by turns: a = -R eps e^(i psi), kappa about 2 / eps, up to 3e4.
    c = fl32(0.99 / 1.99).  Returns (S, R, Rprev, c, ill) with `ill` the mask [F] of the designed bins."""
    rng = np.random.default_rng(seed)
    F = n_fft // 2 + 1
    c = float(np.float32(0.99 / 1.99))
    R = (0.5 + 1.5 * rng.random((B, T, F))) * np.exp(2j * np.pi * rng.random((B, T, F)))
    Rprev = R * (0.25 + 0.75 * rng.random((B, T, F))) * np.exp(1j * np.pi * (0.5 + rng.random((B, T, F))))
    ill = np.arange(F) % 16 == 7
    eps = 2.0 ** -(6 + (np.arange(F) // 16) % 9)
    near = (R / c) * (1.0 + eps * np.exp(2j * np.pi * rng.random((B, T, F))))
    Rprev = np.where(ill, near, Rprev)
    S = 0.5 + rng.random((B, T, F))
    return f32(S), f32(R), f32(Rprev), c, ill


# ---- the reference stages ---------------------------------------------------------------------------------------------------
def angles(R, Rprev=None, c=0.0):
    """torchaudio 0.8.1: a = R - c Rprev (no subtraction without Rprev); a / (|a| + 1e-16)."""
    a = np.asarray(R, dtype=np.complex128)
    if Rprev is not None:
        a = a - float(c) * np.asarray(Rprev, dtype=np.complex128)
    return a / (np.abs(a) + 1e-16)


def spectrum(S, ang0=None, R=None, Rprev=None, c=0.0):
    """S * angles as the inverse transform takes it: the initial angles (all 1 without ang0) when there is no R; the imaginary
    parts of bins 0 and n_fft / 2 dropped, as a complex-to-real transform drops them."""
    S = np.asarray(S, dtype=np.float64)
    if R is None:
        a = np.ones(S.shape, np.complex128) if ang0 is None else np.asarray(ang0, dtype=np.complex128)
    else:
        a = angles(R, Rprev, c)
    X = S * a
    X[..., 0] = X[..., 0].real
    X[..., -1] = X[..., -1].real
    return X


def synth(S, window, ang0=None, R=None, Rprev=None, c=0.0):
    """frames [..., n_fft] = irfft(S angles) * window."""
    n = window.shape[0]
    return np.fft.irfft(spectrum(S, ang0, R, Rprev, c), n=n, axis=-1) * np.asarray(window, dtype=np.float64)


def overlap_sum(frames, hop, L):
    """[B, L]: the overlap-added frames at the retained samples, zero past the natural length (before the envelope)."""
    B, T, n = frames.shape
    full = np.zeros((B, n + hop * (T - 1) + max(0, L)), dtype=frames.dtype)
    for t in range(T):                                   # ascending t: with float32 frames this is the kernel's own order
        full[:, t * hop:t * hop + n] += frames[:, t]
    m = min(L, natural_length(n, hop, T))
    y = np.zeros((B, L), dtype=frames.dtype)
    y[:, :m] = full[:, n // 2:n // 2 + m]
    return y


def overlap(frames, env, hop, L):
    """y [B, L] = overlap-add / envelope inside the natural length, 0 past it (torch.istft with `length`)."""
    n = frames.shape[-1]
    m = min(L, natural_length(n, hop, frames.shape[1]))
    y = overlap_sum(np.asarray(frames, dtype=np.float64), hop, L)
    y[:, :m] /= np.asarray(env, dtype=np.float64)[:m]
    return y


def overlap_fp32(frames, env, hop, L):
    """The overlap kernel restated in fp32: per sample the sum over the covering frames in ascending order starting from +0,
    then ONE division by the envelope, each operation correctly rounded (the library is built with contraction off and
    correctly rounded division) -- so the device must give these bits."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    n = frames.shape[-1]
    m = min(L, natural_length(n, hop, frames.shape[1]))
    y = overlap_sum(frames, hop, L)
    assert y.dtype == np.float32
    y[:, :m] = y[:, :m] / np.asarray(env, dtype=np.float32)[:m]
    return y


def reflect_rows(y, pad):
    return np.pad(y, ((0, 0), (pad, pad)), mode="reflect")


def analysis(y, window, hop, T):
    """R [B, T, F] = rfft(window * frame t of the reflect-padded y) (torch.stft, center=True, pad_mode='reflect', onesided)."""
    n = window.shape[0]
    yp = reflect_rows(np.asarray(y, dtype=np.float64), n // 2)
    idx = hop * np.arange(T)[:, None] + np.arange(n)[None, :]
    return np.fft.rfft(yp[:, idx] * np.asarray(window, dtype=np.float64), axis=-1)


def step(S, window, env, hop, L, ang0=None, R=None, Rprev=None, c=0.0):
    """One iteration: (frames, y, R_next)."""
    fr = synth(S, window, ang0, R, Rprev, c)
    y = overlap(fr, env, hop, L)
    return fr, y, analysis(y, window, hop, S.shape[1])


def trajectory(S, ang0, window, env, hop, L, c, n_iter):
    """The fp64 loop: [R_0 .. R_(n_iter - 1)], R_k the spectrum rebuilt in iteration k (R_-1: the initial angles)."""
    out = []
    for k in range(n_iter):
        R = out[k - 1] if k >= 1 else None
        Rprev = out[k - 2] if (k >= 2 and c != 0.0) else None
        out.append(step(S, window, env, hop, L, ang0, R, Rprev, c)[2])
    return out


# ---- norms ------------------------------------------------------------------------------------------------------------------
def norm2s(X):
    """Per frame, the 2-norm of the Hermitian-extended (two-sided) spectrum of a one-sided X [..., F] (n_fft even)."""
    p = np.abs(X) ** 2
    return np.sqrt(2.0 * p.sum(axis=-1) - p[..., 0] - p[..., -1])


def pair_norm(v, n_fft):
    """v [NF] per frame (flat frame order) -> per frame the 2-norm over the frames transformed TOGETHER with it: frames 2i and
    2i + 1 of the flat order share one complex transform below 2048 points (a missing partner counts as zero)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if n_fft == 2048:
        return v
    w = np.concatenate([v, np.zeros(v.size % 2)]).reshape(-1, 2)
    return np.repeat(np.sqrt((w ** 2).sum(axis=1)), 2)[:v.size]


def transform_ceiling(n_fft):
    """Relative 2-norm error of one transform of the stage, input to output.  Below 2048: the n_fft-point complex transform
    (fft_ceiling) plus the packing (A + i B, conj A + i conj B) or the split (Z[k] +- conj Z[n - k]) / 2: one rounded addition
    per component of magnitude <= |A_k| + |B_k| resp. |Z_k| + |Z_(n-k)|, in the 2-norm over k at most sqrt(2) U times the pair's
    norm -- 2 U covers it (the halving is exact).  2048: real2048_ceiling(), which counts pack2048 / split2048 as its stage."""
    return real2048_ceiling() if n_fft == 2048 else fft_ceiling(n_fft) + 2.0 * U


# ---- the conditioned bound of spec_at ---------------------------------------------------------------------------------------
def kappa(R, Rprev=None, c=0.0):
    """kappa = (|R| + c |Rprev|) / |R - c Rprev| >= 1 per bin: how much a relative perturbation of R and c Rprev grows in
    a = R - c Rprev.  1 without a momentum term.  (inf where a == 0 and R != 0.)"""
    R = np.asarray(R, dtype=np.complex128)
    if Rprev is None:
        return np.ones(R.shape)
    q = float(c) * np.asarray(Rprev, dtype=np.complex128)
    num, den = np.abs(R) + np.abs(q), np.abs(R - q)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num == 0.0, 1.0, num / den)


def spec_bound(S, R=None, Rprev=None, c=0.0):
    """|fl32(spec_at) - S a / (|a| + 1e-16)| per bin, a = R - c Rprev from the SAME fp32 inputs: S (2 kappa U + 3 U).

    The count behind the two terms: two rounded operations per component of a, each at most kappa U |a| -- 2 kappa U; the
    norm's squares and sum (2 U on the radicand, halved by the root), the root, and the division and the product with S --
    3 U when the last two are taken as one.  The derivation, to first order, with u = a / |a|, t = c |q| / |a| <= kappa,
    q = Rprev, and every error split into its part ALONG u and its part ACROSS u:

      1. fl(c q) is off by at most U c |q| = t U |a|.  The result is normalised, so only the part across u counts: t U.
      2. fl(R - .) puts a relative error d_x, d_y (|d| <= U) on each component of a: (a_x d_x, a_y d_y).  Its part along u is
         normalised away; across u it is |a| sin th cos th (d_y - d_x), th the angle of a: at most U.
      3. n^ = fl(sqrt(fl(fl(a_x^2) + fl(a_y^2)))) + 1e-16: 2 U on the radicand, halved by the root, plus the root's own U:
         2 U on the norm, along u.  The addition returns its first operand for |a| >= 2^-28 (1e-16 is below half an ulp
         there) and is then within 2^-25 |a| of the exact sum.
      4. The division and the product with S put a relative error of at most 2 U on each component: up to 2 U along u when
         both components err alike, up to 2 U across u (and then nothing along) when they err oppositely at th = 45 degrees.

    Along u: at most 2 U + 2 U; across u: at most t U + U + 2 U; and what 4. spends across it cannot spend along.  With 4.'s two
    errors as mu + eta and mu - eta (|mu| + |eta| <= 2 U) the squared length is (2 + mu + eta cos 2th)^2 +
    (t + sin 2th (1 + eta))^2 in units of U^2, whose largest value over mu, eta and th is below (t + sqrt(17))^2 (t = 0: 17 at
    eta = 0, th = 45 degrees; 16.2 at eta = 2; the derivative in t is at most 1).  So the sharp first-order bound is
    (t + sqrt(17)) U = (t + 4.13) U, and
        (2 kappa + 3) - (t + sqrt(17)) = (2 |R| + c |q|) / |a| - 1.13 >= (2 |R| + c |q|) / (|R| + c |q|) - 1.13 >= 0
    whenever |R| >= 0.15 c |Rprev| (without Rprev: t = 0, kappa = 1, 4.13 <= 5).  Elsewhere 2 kappa - t >= kappa >= 1 still
    holds, so the stated bound can be short of the sharp one by 0.13 U S at most.  The second-order term of the turn is
    (2 kappa U)^2 / 2, 1e-3 of the first at kappa = 3e4.  The designed inputs assert both premises (|R| >= 0.15 c |Rprev|,
    |a| >= 2^-28).

    The stock fp32 formulation (mul, sub, pow, sum, pow, add, div, mul on real views) has the same operation count, so this is
    its bound as well; on the CPU it reaches 0.65 of it on the G27 states (tests/test_griffinlim_reference_host.py)."""
    k = kappa(R, Rprev, c) if R is not None else np.ones(np.shape(S))
    return np.asarray(S, dtype=np.float64) * (2.0 * k * U + 3.0 * U)


# ---- the bounds of the three stages -----------------------------------------------------------------------------------------
def synth_ceiling(S, window, ang0=None, R=None, Rprev=None, c=0.0):
    """Per frame [B, T], ||frames^ - frames||_2 in absolute terms (divide by ||frames||_2 for the relative figure).

    The unwindowed frame x = irfft(X) has ||x||_2 = ||X||_2s / sqrt(n) (Parseval, X two-sided).  Its errors:
      * the transform's: transform_ceiling(n) times the norm of what is transformed together, the frame and its pair partner
        (below 2048 points two frames are the real and imaginary part of one complex sequence; |da| <= |dz| elementwise);
      * spec_at's: linear in the spectrum's error, whose two-sided 2-norm is at most that of spec_bound (the partner's
        spectrum error stays in the partner's part of the sequence, to first order).
    The window (times 1 / n, a power of two: exact) multiplies both by at most max |w|, and its product rounds once: U ||frames||."""
    n = window.shape[0]
    X = spectrum(S, ang0, R, Rprev, c)
    xn = norm2s(X) / math.sqrt(n)
    sb = norm2s(spec_bound(S, R, Rprev, c)) / math.sqrt(n)
    wmax = float(np.abs(window).max())
    ref = np.linalg.norm(np.fft.irfft(X, n=n, axis=-1) * window, axis=-1)
    return wmax * (transform_ceiling(n) * pair_norm(xn, n).reshape(xn.shape) + sb) + U * ref


def analysis_ceiling(Rref, n_fft):
    """Per frame [B, T], ||R^ - R||_2 (one-sided, which the two-sided norm bounds) in absolute terms: the window product rounds
    once (U, relative, on every input sample), then the transform: (1 + U)(1 + transform_ceiling) - 1, times the two-sided norm
    of what is transformed together (the frame and its pair partner)."""
    rel = (1.0 + U) * (1.0 + transform_ceiling(n_fft)) - 1.0
    n2 = norm2s(Rref)
    return rel * pair_norm(n2, n_fft).reshape(n2.shape)


def covering(n_fft, hop):
    """The most frames that cover one sample."""
    return -(-n_fft // hop)


def overlap_bound(frames, env, hop, L):
    """|y^ - y| per sample [B, L] of the fp32 overlap kernel against the fp64 sum of the SAME fp32 frames: m frames summed one
    after the other carry gamma_(m-1) sum |f_t| (gamma_k = k U / (1 - k U); Higham, Accuracy and Stability, 2nd ed., eq. 4.4),
    the division one more factor (1 + U):  ((1 + gamma_(m-1))(1 + U) - 1) sum_t |f_t| / env.  m <= ceil(n_fft / hop)."""
    m = covering(frames.shape[-1], hop)
    g = (m - 1) * U / (1.0 - (m - 1) * U)
    return ((1.0 + g) * (1.0 + U) - 1.0) * overlap(np.abs(np.asarray(frames, dtype=np.float64)), env, hop, L)


def step_bounds(S, window, env, hop, L, ang0=None, R=None, Rprev=None, c=0.0, ceilings=True):
    """The conditioned bound of spec_at carried through one iteration whose stages are fed one another's outputs: (frames: per
    frame 2-norm [B, T]; y: per row 2-norm [B]; R_next: per frame 2-norm [B, T]), all absolute.

      frames  max |w| ||spec_bound||_2s / sqrt(n): the inverse transform is linear and ||irfft(dX)||_2 = ||dX||_2s / sqrt(n).
      y       dy[j] = sum over the m <= ceil(n / hop) covering frames of df_t[j - t hop] / env[j], so |dy[j]|^2 <=
              m sum_t df_t[..]^2 / min env^2, and every element of every frame is used once:
              ||dy||_2 <= sqrt(m) sqrt(sum_t ||df_t||_2^2) / min env.
      R_next  frame t of dy, reflect-padded and windowed, holds a sample at most three times (itself and a reflection at either
              end): ||w dy_t||_2 <= max |w| sqrt(3) ||dy||_2, and the transform's two-sided norm is sqrt(n) times that.

    With `ceilings` the stages' own rounding is added -- synth_ceiling instead of the first line, the 2-norm of overlap_bound,
    analysis_ceiling -- which makes the three figures rigorous bounds of an fp32 step (the stock one is held to them on the
    host).  Without, they are the share of the error that conditioning explains, the yardstick beside CPU_FACTOR times the
    CPU's error in the teacher-forced test; the transforms' share (a few U, against ceilings of 100 U) is that clause's."""
    n = window.shape[0]
    wmax = float(np.abs(window).max())
    fr, _, Rn = step(S, window, env, hop, L, ang0, R, Rprev, c)
    fb = synth_ceiling(S, window, ang0, R, Rprev, c) if ceilings else wmax * norm2s(spec_bound(S, R, Rprev, c)) / math.sqrt(n)
    m = min(L, natural_length(n, hop, S.shape[1]))
    yb = math.sqrt(covering(n, hop)) * np.sqrt((fb ** 2).sum(axis=1)) / float(np.asarray(env)[:m].min())
    if ceilings:
        yb = yb + np.linalg.norm(overlap_bound(fr, env, hop, L), axis=1)
    rb = math.sqrt(3.0 * n) * wmax * yb[:, None] + (analysis_ceiling(Rn, n) if ceilings else np.zeros(Rn.shape[:2]))
    return fb, yb, rb


# ---- error measures ---------------------------------------------------------------------------------------------------------
def frame_err(got, ref):
    """||got - ref||_2 per frame (last axis), absolute."""
    return np.linalg.norm(np.asarray(got) - ref, axis=-1)


def rel(err, ref):
    """err / ||ref||_2 per frame; a frame whose reference is all zero must have no error (reported as 0, or inf)."""
    nr = np.linalg.norm(ref, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(nr == 0.0, np.where(err == 0.0, 0.0, np.inf), err / nr)


# ---- the stock fp32 formulation on the CPU ----------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def stock_spectrum(S, ang0=None, R=None, Rprev=None, c=0.0):
    """S * angles in fp32 as spectral._stock_loop forms them (real views: mul by c, sub, pow, sum, pow, add, div, mul),
    -> complex64 tensor [B, T, F]."""
    torch = _torch()
    spec = torch.from_numpy(np.asarray(S, dtype=np.float32))
    if R is None:
        a = np.ones(np.shape(S), np.complex64) if ang0 is None else np.asarray(ang0, dtype=np.complex64)
        ang = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a)))
    else:
        ang = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(np.asarray(R, dtype=np.complex64))))
        if Rprev is not None:
            prev = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(np.asarray(Rprev, dtype=np.complex64)))).clone()
            ang = ang - prev.mul_(float(c))
        ang = ang.div(ang.pow(2.).sum(-1).pow(0.5).add(1e-16).unsqueeze(-1).expand_as(ang))
    return torch.view_as_complex((spec.unsqueeze(-1).expand_as(ang) * ang).contiguous())


def stock_synth(S, window, ang0=None, R=None, Rprev=None, c=0.0):
    """fp32: irfft of the stock spectrum, times the window (istft's first two steps) -> float64 array of the fp32 values."""
    torch = _torch()
    n = window.shape[0]
    x = torch.fft.irfft(stock_spectrum(S, ang0, R, Rprev, c), n=n, dim=-1) * torch.from_numpy(np.asarray(window, dtype=np.float32))
    return x.numpy().astype(np.float64)


def stock_analysis(y, window, hop):
    """torch.stft in fp32 (center, reflect, onesided) -> complex128 array [B, T, F] of the fp32 values."""
    torch = _torch()
    n = window.shape[0]
    R = torch.stft(torch.from_numpy(np.asarray(y, dtype=np.float32)), n_fft=n, hop_length=hop, win_length=n,
                   window=torch.from_numpy(np.asarray(window, dtype=np.float32)), center=True, pad_mode="reflect", normalized=False,
                   onesided=True, return_complex=True)
    return R.transpose(1, 2).numpy().astype(np.complex128)


def stock_step(S, window, hop, L, ang0=None, R=None, Rprev=None, c=0.0):
    """One stock fp32 iteration on the CPU: (frames, y, R_next) as float64 / complex128 arrays of the fp32 values.  y is
    torch.istft's (its own overlap-add and envelope), `window` the padded n_fft window."""
    torch = _torch()
    n = window.shape[0]
    w = torch.from_numpy(np.asarray(window, dtype=np.float32))
    X = stock_spectrum(S, ang0, R, Rprev, c)
    y = torch.istft(X.transpose(1, 2), n_fft=n, hop_length=hop, win_length=n, window=w, length=L).float()
    return stock_synth(S, window, ang0, R, Rprev, c), y.numpy().astype(np.float64), stock_analysis(y.numpy(), window, hop)


def g27_setup(g):
    """A G27 fixture (tests/golden/g27_*.npz) in this module's terms: dict(S, ang0 [B, T, F] as rounded to fp32, window, env,
    n_fft, hop, B, T, L, c)."""
    n, hop, wl, length = (int(v) for v in g["params"])
    spec = g["spec"].reshape(-1, *g["spec"].shape[-2:]).astype(np.float64)
    S = f32(np.transpose(spec ** (1.0 / float(g["power"])), (0, 2, 1)))
    ang0 = f32(np.transpose(g["angles"].reshape(spec.shape), (0, 2, 1)))
    B, T = S.shape[:2]
    L = hop * (T - 1) if length < 0 else length
    w = f32(padded(g["window"].astype(np.float64), n))
    m = float(g["momentum"])
    c = float(np.float32(m / (1.0 + m))) if m else 0.0
    return dict(S=S, ang0=ang0, window=w, env=f32(envelope(w, hop, T, L)), n_fft=n, hop=hop, B=B, T=T, L=L, c=c)


def teacher_forced_states(p, n_iter=16):
    """[(k, R_(k-1), R_(k-2))] for k = 1 .. n_iter along the fp64 trajectory of the G27 setup `p`, rounded to fp32: the inputs
    of iteration k (R_(k-2) is None for k = 1 and when c == 0, as the loop runs it)."""
    tr = trajectory(p["S"], p["ang0"], p["window"], p["env"], p["hop"], p["L"], p["c"], n_iter)
    return [(k, f32(tr[k - 1]), f32(tr[k - 2]) if (k >= 2 and p["c"] != 0.0) else None) for k in range(1, n_iter + 1)]


# ---- running the hook (needs a device) --------------------------------------------------------------------------------------
GUARD = 256                                                  # floats behind `out` that no kernel may touch


def to_device(a, complex_=False):
    """numpy (rounded to float32 / complex64) or an already resident CUDA tensor -> CUDA tensor; None stays None."""
    torch = _torch()
    if a is None or isinstance(a, torch.Tensor):
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex64 if complex_ else np.float32)).cuda()


def device_stage(stage, out_floats, B, T, n_fft, hop, L, c=0.0, S=None, ang0=None, R=None, Rprev=None, inp=None, window=None, env=None):
    """One call of ddsp_griffinlim_stage -> float32 array [out_floats]; asserts the return code and an untouched guard zone."""
    import ddsp_pytorch_amd as ddsp
    torch = _torch()
    lib = ddsp._lib.lib()
    t = [to_device(S), to_device(ang0, True), to_device(R, True), to_device(Rprev, True), to_device(inp), to_device(window), to_device(env)]
    out = torch.full((out_floats + GUARD,), float("nan"), device="cuda")
    out[out_floats:] = 12345.0
    rc = lib.ddsp_griffinlim_stage(stage, *[None if v is None else v.data_ptr() for v in t], out.data_ptr(), B, T, n_fft, hop, L, float(c),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((out[out_floats:] == 12345.0).all()), "the stage wrote behind its output"
    return out[:out_floats].cpu().numpy()


def device_synth(S, window, hop, L, ang0=None, R=None, Rprev=None, c=0.0):
    """-> frames float32 [B, T, n_fft]"""
    B, T = S.shape[:2]
    n = window.shape[0]
    return device_stage(SYNTH, B * T * n, B, T, n, hop, L, c, S=S, ang0=ang0, R=R, Rprev=Rprev, window=window).reshape(B, T, n)


def device_overlap(frames, env, hop, L):
    """-> y float32 [B, L]"""
    B, T, n = frames.shape
    return device_stage(OVERLAP, B * L, B, T, n, hop, L, inp=frames, env=env).reshape(B, L)


def device_analysis(y, window, hop, T):
    """-> R complex64 [B, T, F]"""
    B, L = y.shape
    n = window.shape[0]
    F = n // 2 + 1
    out = device_stage(ANALYSIS, 2 * B * T * F, B, T, n, hop, L, inp=y, window=window)
    return out.view(np.complex64).reshape(B, T, F)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the criteria of a stage on its own -------------------------------------------------------------------------------------
def sharp(tag, err, ref_norm_of, cpu_err, ceiling, lines):
    """The sharp criterion on per-frame figures: the worst relative error at most CPU_FACTOR times the CPU fp32 formulation's
    worst on the same data, and every frame under its derived ceiling.  Appends the figures to `lines`; -> passed."""
    g, c = rel(err, ref_norm_of), rel(cpu_err, ref_norm_of)
    with np.errstate(divide="ignore", invalid="ignore"):
        over = float(np.max(np.where(ceiling > 0, err / ceiling, np.where(err == 0, 0.0, np.inf))))
    lines.append(f"GLS {tag}: gpu {g.max() / U:.2f}U cpu {c.max() / U:.2f}U ratio {g.max() / c.max() if c.max() else float('inf'):.2f} "
                 f"worst error / ceiling {over:.3f}")
    return bool(g.max() <= CPU_FACTOR * c.max() and over <= 1.0)


def check_synth(tag, got, S, window, ang0=None, R=None, Rprev=None, c=0.0, lines=None):
    lines = [] if lines is None else lines
    ref = synth(S, window, ang0, R, Rprev, c)
    cpu = stock_synth(S, window, ang0, R, Rprev, c)
    got = np.asarray(got, dtype=np.float64)
    ok = bool(np.isfinite(got).all()) and sharp(tag + " synth", frame_err(got, ref), ref, frame_err(cpu, ref),
                                                synth_ceiling(S, window, ang0, R, Rprev, c), lines)
    return ok, lines


def check_analysis(tag, got, y, window, hop, lines=None):
    lines = [] if lines is None else lines
    T = got.shape[1]
    ref = analysis(y, window, hop, T)
    cpu = stock_analysis(y, window, hop)
    got = np.asarray(got, dtype=np.complex128)
    ok = bool(np.isfinite(got.view(np.float64)).all()) and sharp(tag + " analysis", frame_err(got, ref), ref, frame_err(cpu, ref),
                                                                  analysis_ceiling(ref, window.shape[0]), lines)
    return ok, lines


def check_overlap(tag, got, frames, env, hop, L, lines=None):
    """Bit for bit the fp32 restatement; within the summation bound of the fp64 sum; exactly 0 past the natural length."""
    lines = [] if lines is None else lines
    want = overlap_fp32(frames, env, hop, L)
    same = bool(np.array_equal(bits(got), bits(want)))
    bound = overlap_bound(frames, env, hop, L)
    err = np.abs(got.astype(np.float64) - overlap(frames, env, hop, L))
    with np.errstate(divide="ignore", invalid="ignore"):
        over = float(np.max(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))))
    nat = natural_length(frames.shape[-1], hop, frames.shape[1])
    tail = bool(np.all(bits(got[:, nat:]) == 0))
    lines.append(f"GLS {tag} overlap: bits equal {same}, differing {int((bits(got) != bits(want)).sum())}, worst error / summation bound "
                 f"{over:.3f}, {max(0, L - nat)} tail samples zero {tail}")
    return same and over <= 1.0 and tail, lines


def random_case(rng):
    """One random case of the stage sweep: dict(n_fft, hop, win_length (0: rectangular), B, T, L, c, ang0, rprev: presence flags)."""
    n = int(rng.choice(SIZES))
    rect = rng.random() < 0.25
    hop = int(rng.integers(max(1, n // 16), n + 1)) if rect else int(rng.integers(max(1, n // 16), n // 2 + 1))
    wl = 0 if rect else int(rng.integers(max(2 * hop, n // 2), n + 1))
    T = int(rng.integers(max(2, n // 2 // hop + 2), 41))
    extra = int(rng.integers(0, hop))
    L = hop * (T - 1) + extra                                    # (extra > n_fft / 2, rectangular window only: a zero tail)
    assert L > n // 2 and 1 + L // hop == T
    mode = int(rng.integers(0, 4))                               # 0: no R, no ang0; 1: ang0; 2: R alone; 3: R and Rprev
    return dict(n_fft=n, hop=hop, win_length=wl, B=int(rng.integers(1, 5)), T=T, L=L, mode=mode,
                c=0.0 if rng.random() < 0.2 else float(np.float32(rng.random() * 0.6)))


def run_case(case, seed, lines=None):
    """The three stages, each on its own random inputs, under check_synth / check_overlap / check_analysis -> passed."""
    lines = [] if lines is None else lines
    n, hop, B, T, L, c = (case[k] for k in ("n_fft", "hop", "B", "T", "L", "c"))
    w = f32(np.ones(n) if case["win_length"] == 0 else padded(hann(case["win_length"]), n))
    env = f32(np.maximum(envelope(w, hop, T, L), 1e-3))          # (a positive divisor is all the overlap stage asks for)
    tag = f"n{n} hop {hop} wl {case['win_length']} [{B}, {T}] L {L} mode {case['mode']} c {c:.3f}"
    S, ang0, R, Rprev = random_state(seed, B, T, n, c)
    state = [dict(), dict(ang0=ang0), dict(R=R, c=c), dict(R=R, Rprev=Rprev, c=c)][case["mode"]]
    ok1, _ = check_synth(tag, device_synth(S, w, hop, L, **state), S, w, lines=lines, **state)
    rng = np.random.default_rng(seed + 1)
    fr = f32(rng.standard_normal((B, T, n)))
    ok2, _ = check_overlap(tag, device_overlap(fr, env, hop, L), fr, env, hop, L, lines=lines)
    y = f32(rng.standard_normal((B, L)))
    ok3, _ = check_analysis(tag, device_analysis(y, w, hop, T), y, w, hop, lines=lines)
    return ok1 and ok2 and ok3, lines
