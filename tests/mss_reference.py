"""fp64 reference, inputs, shapes and error bounds for ONE scale of the multi-scale spectral loss as csrc/ddsp_mss_fft.hip
computes it in one kernel (ddsp_mss_scale: reflect framing, two transforms of packed frame pairs, the Hermitian split, both L1
terms, the gradient spectrum, the inverse transform, the scatter to grad_frames), for the gather that follows it
(ddsp_stft_frames_backward) and for the per-bin pass of the library-FFT path (ddsp_spectral_loss).  Used by
tests/test_gpu_mss_stages.py and tests/fuzz_parity.py (on the device) and tests/test_mss_reference_host.py (the reference and the
bounds themselves, without a device).

The reference is numpy in float64 / complex128 and imports neither torch nor the package: x [B, L], frames [B, F, n_fft],
spectra [B, F, n_fft / 2 + 1].  Every bound is a function whose docstring holds its derivation from the unit roundoff U = 2^-24
and counted operations; the transforms' own bounds are those of tests/wave_fft_reference.py.  The last sections are the stock
fp32 formulation on the CPU (torch, imported only there) -- the yardstick of the sharp criterion, at most CPU_FACTOR times its
error on the same inputs, and the proof on the host that the bounds are attainable without the code under test -- and the
ctypes calls themselves."""
import math

import numpy as np

from griffinlim_reference import GUARD, bits, f32, hann, norm2s, pair_norm, transform_ceiling  # noqa: F401  (re-exported)
from wave_fft_reference import CPU_FACTOR, PAIR_BT, U  # noqa: F401  (re-exported)

SIZES = (64, 128, 256, 512, 1024, 2048)
MAX_UNITS = 4096                 # kMaxBlocks of ddsp_mss_fft.hip: the kernels stride over the units beyond this many
EINVAL, ERANGE = -1, -2
LN2 = math.log(2.0)
UNDECIDED_CAP = 0.005            # at most this share of a case's bins may be undecided (checked from the reference alone)
TERM_TOL = 2e-5                  # each of the two terms, relative (the project's figure for their sum)
SIGNS = (-1.0, 0.0, 1.0)
SWEEP_SEEDS, SWEEP_CASES = (31, 32), 30     # what tests/test_gpu_fuzz.py runs of fuzz_parity.sweep_mss_stages


def window_of(n_fft):
    """The periodic Hann window as the device is given it: rounded to fp32."""
    return f32(hann(n_fft))


def units(n_fft, B, F):
    """Units (what one wavefront takes at a time) of a call: B ceil(F / 2) pairs in groups of BT below 2048, B F frames at 2048."""
    return B * F if n_fft == 2048 else -(-(B * ((F + 1) // 2)) // PAIR_BT[n_fft])


# ---- the reference scale ----------------------------------------------------------------------------------------------------
def frames_of(x, window, hop):
    """[B, F, n_fft]: frame f of the reflect-padded rows (torch.stft, center=True, pad_mode='reflect'), times the window."""
    n = window.shape[0]
    x = np.asarray(x, dtype=np.float64)
    F = 1 + x.shape[1] // hop
    xp = np.pad(x, ((0, 0), (n // 2, n // 2)), mode="reflect")
    idx = hop * np.arange(F)[:, None] + np.arange(n)[None, :]
    return xp[:, idx] * np.asarray(window, dtype=np.float64)


def coefficient(P, Q, alpha, eps, sd=None, se=None):
    """c' = count * c = sd - alpha se / (ln 2 (P + eps)); sd = sign(P - Q) and se = sign(log2(Q + eps) - log2(P + eps)) unless given."""
    if sd is None:
        sd = np.sign(P - Q)
    if se is None:
        se = np.sign(np.log2(Q + eps) - np.log2(P + eps))
    return sd - alpha * se / (LN2 * (P + eps))


def grad_frames_of(G, n_fft):
    """[.., n_fft]: Re sum_k h_k G_k e^(+2 pi i k n / n_fft) over the one-sided bins, h = 1 at bins 0 and n_fft / 2 and interior
    bins counted once: n_fft * irfft of G with its interior bins halved (irfft extends Hermitian-ly and so counts them twice)."""
    Y = np.array(G, dtype=np.complex128)
    Y[..., 1:-1] *= 0.5
    return n_fft * np.fft.irfft(Y, n=n_fft, axis=-1)


def scale(x_pred, x_true, n_fft, hop, alpha, eps, window=None):
    """One scale in fp64 -> dict:
      S, T         spectra of the prediction's and the target's windowed frames [B, F, n_fft / 2 + 1], F = 1 + L // hop
      P, Q         their powers
      lin, log, loss   mean |P - Q|, mean |log2(Q + eps) - log2(P + eps)| over count = B F (n_fft / 2 + 1) bins, lin + alpha log
      c1           c' = count c_k, c_k = (sign(P - Q) - alpha sign(e) / (ln 2 (P + eps))) / count, e = log2(Q+eps) - log2(P+eps)
      G            the one-sided gradient spectrum 2 c_k S_k
      grad_frames  [B, F, n_fft] = Re sum_k h_k G_k e^(+2 pi i k n / n_fft): d loss / d windowed frame
      frames_p, frames_t, window, count, and the arguments.
    The spectrum of a real frame is real at bins 0 and n_fft / 2, so G is real there; the kernel keeps only the real part at
    those two bins (its packed inverse transform has no place for another), which is what a complex-to-real transform does and
    what `grad_frames_of` does here (irfft drops those imaginary parts): a device whose end bins carried an imaginary residue of
    rounding would lose it, not spread it."""
    w = window_of(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    fp, ft = frames_of(x_pred, w, hop), frames_of(x_true, w, hop)
    S, T = np.fft.rfft(fp, axis=-1), np.fft.rfft(ft, axis=-1)
    P, Q = S.real ** 2 + S.imag ** 2, T.real ** 2 + T.imag ** 2
    count = float(P.size)
    lin = float(np.abs(P - Q).sum() / count)
    log = float(np.abs(np.log2(Q + eps) - np.log2(P + eps)).sum() / count)
    c1 = coefficient(P, Q, alpha, eps)
    G = (2.0 / count) * c1 * S
    return dict(S=S, T=T, P=P, Q=Q, lin=lin, log=log, loss=lin + alpha * log, c1=c1, G=G, grad_frames=grad_frames_of(G, n_fft),
                frames_p=fp, frames_t=ft, window=w, count=count, n_fft=n_fft, hop=hop, alpha=float(alpha), eps=float(eps))


def recover(frames):
    """The one-sided G of a set of gradient frames [.., n_fft], by an fp64 rfft: a frame Re sum_k G_k e^(+i theta k n) transforms
    to n_fft / 2 * G_k at interior bins and to n_fft * G_k at the two (real) end bins."""
    frames = np.asarray(frames, dtype=np.float64)
    n = frames.shape[-1]
    X = np.fft.rfft(frames, axis=-1) * (2.0 / n)
    X[..., 0] *= 0.5
    X[..., -1] *= 0.5
    return X


def gather(grad_frames, window, hop, L):
    """[B, L]: the adjoint of the framing in fp64 -- window, overlap-add at the padded positions, and the reflect padding's adjoint
    (a padded position left of the row adds to its mirror about sample 0, one right of it to its mirror about sample L - 1)."""
    g = np.asarray(grad_frames, dtype=np.float64) * np.asarray(window, dtype=np.float64)
    B, F, n = g.shape
    half = n // 2
    full = np.zeros((B, max(L + n, hop * (F - 1) + n)), dtype=np.float64)
    for f in range(F):
        full[:, f * hop:f * hop + n] += g[:, f]
    out = full[:, half:half + L].copy()
    m = np.arange(1, half + 1)
    out[:, m] += full[:, half - m]
    m = np.arange(L - 1 - half, L - 1)
    out[:, m] += full[:, half + 2 * (L - 1) - m]
    return out


# ---- the bounds -------------------------------------------------------------------------------------------------------------
def spectrum_error(S, n_fft):
    """dS [B, F]: the ceiling on |S^_k - S_k| of every bin k of a frame.  The window product rounds once per sample (U, relative),
    then the transform and its split: (1 + U)(1 + transform_ceiling(n_fft)) - 1 in the relative 2-norm, and a single bin's error
    is at most the 2-norm of all of them.  The norm is the two-sided spectrum's (sqrt(n_fft) times the windowed frame's, Parseval)
    of what is transformed TOGETHER: the packed pair of frames 2q, 2q + 1 of a row below 2048 points, the frame itself at 2048
    (griffinlim_reference.pair_norm, per row: a row with an odd frame count ends in a pair with an empty partner)."""
    rel = (1.0 + U) * (1.0 + transform_ceiling(n_fft)) - 1.0
    n2 = norm2s(S)
    return rel * np.stack([pair_norm(r, n_fft) for r in n2])


def power_error(absS, dS):
    """dP = 2 |S| dS + dS^2: |S + d|^2 - |S|^2 for |d| <= dS."""
    return 2.0 * absS * dS + dS ** 2


def log_slack(P, Q, eps):
    """How far apart P and Q must be for an fp32 evaluation of sign(log2(Q + eps) - log2(P + eps)) to be the true one, beyond what
    the powers' own errors decide: each sum x + eps rounds once (U x) and the hardware log2 is within 1 ulp of a value of
    magnitude |log2 x|, 2 U |log2 x| absolute, which is what a relative change of 2 U ln 2 |log2 x| of x does.  Both sides:
    (P + eps)(U + 2 U ln 2 |log2(P + eps)|) + the same of Q."""
    a, b = P + eps, Q + eps
    return a * (U + 2.0 * U * LN2 * np.abs(np.log2(a))) + b * (U + 2.0 * U * LN2 * np.abs(np.log2(b)))


def undecided(r, dS=None, dT=None):
    """Mask [B, F, bins] of the bins whose signs an fp32 evaluation may legitimately take otherwise: |P - Q| <= 2 (dP + dQ) with
    the dS of `spectrum_error` (the prediction's and the target's, each relative to its own pair), plus `log_slack`, without
    which the rule would not cover the second sign function where both powers vanish beside eps.  A bin with P == Q exactly and
    both spectra exactly equal (an identical row) is decided: sign 0, on the device bit for bit."""
    dS = spectrum_error(r["S"], r["n_fft"]) if dS is None else dS
    dT = spectrum_error(r["T"], r["n_fft"]) if dT is None else dT
    dP = power_error(np.abs(r["S"]), dS[..., None])
    dQ = power_error(np.abs(r["T"]), dT[..., None])
    und = np.abs(r["P"] - r["Q"]) <= 2.0 * (dP + dQ) + log_slack(r["P"], r["Q"], r["eps"])
    return und & ~np.all(r["S"] == r["T"], axis=-1, keepdims=True)


def coefficient_bound(absS, P, c1, dS, alpha, eps, rcp_ulps=1.0):
    """|c'^ S^ - c' S| per bin for an fp32 evaluation that took the reference's signs, given |S^ - S| <= dS.

    With t = alpha / (ln 2 (P + eps)) the coefficient is c' = sd - se t.  The kernel's steps and their roundings:
      1. P^ = fma(x, x, y y): the spectrum's error moves it by dP = 2 |S| dS + dS^2, the product and the fma round once each:
         2 U (P + dP).  P^ + eps rounds once: U (P + dP + eps).  Together dPt, an absolute perturbation of the argument P + eps.
      2. the reciprocal: `rcp_ulps` ulps (the kernel's comment claims 1 for v_rcp_f32; an IEEE division: half an ulp), an ulp at
         most 2 U relative.  alpha sign / ln 2 is one rounded product with a constant that is itself rounded (2 U), the product
         with the reciprocal one more (U): r = (1 + 2 U rcp_ulps)(1 + U)^3 - 1.
         The argument is at least eps whatever P^ >= 0 is, so  |t^ - t| <= t dPt / max(P + eps - dPt, eps) = dt0  (exact, not
         first order: 1 / a^ - 1 / a = (a - a^) / (a a^)), and with the roundings  dt = dt0 + r (t + dt0).
      3. sd - se t^ rounds once: dc = dt + U (|c'| + dt).
      4. 2 inv_n (the rounded reciprocal of the count: U) times c'^ (U), times each component of S^ (U): r3 = (1 + U)^3 - 1 on
         the product.  (The half weight h of the 2048 path is a power of two.)
    So  |c'^ S^ - c' S| <= (|c'| + dc) dS + dc |S| + r3 (|c'| + dc)(|S| + dS).
    To first order in dS and without the roundings this is the |c'| dS + (alpha / ln 2) |S| dP / (P + eps)^2 of the issue."""
    dP = power_error(absS, dS)
    dPt = dP + 2.0 * U * (P + dP) + U * (P + dP + eps)
    t = alpha / (LN2 * (P + eps))
    dt0 = t * dPt / np.maximum(P + eps - dPt, eps)
    r = (1.0 + 2.0 * U * rcp_ulps) * (1.0 + U) ** 3 - 1.0
    dt = dt0 + r * (t + dt0)
    ac = np.abs(c1)
    dc = dt + U * (ac + dt)
    r3 = (1.0 + U) ** 3 - 1.0
    return (ac + dc) * dS + dc * absS + r3 * (ac + dc) * (absS + dS)


def inverse_norm(G, n_fft):
    """Per frame, the 2-norm of the two-sided spectrum the inverse transform takes: h G with h = 1 at the end bins and 1/2 inside,
    extended Hermitian-ly (every interior bin twice)."""
    p = np.abs(G) ** 2
    return np.sqrt(p[..., 0] + p[..., -1] + 0.5 * p[..., 1:-1].sum(axis=-1))


def bin_bound(r, G=None, c1=None, dS=None):
    """The ceiling on |recover(device grad_frames) - G| per bin [B, F, bins], for a device that took the signs behind `c1`
    (default: the reference's own, r["c1"], with G = r["G"]).

      * the spectrum of the gradient: (2 / count) coefficient_bound(...) with dS = spectrum_error(S): the transform's ceiling
        (wave_fft_reference.fft_ceiling / real2048_ceiling through griffinlim_reference.transform_ceiling, which counts the
        Hermitian split or split2048 as its stage) times the 2-norm of the packed pair (the frame at 2048);
      * the inverse transform: its frames g = n-point unnormalised inverse of the two-sided Y = h G have ||g||_2 = sqrt(n) ||Y||_2
        and come back within transform_ceiling ||g||_2 (pair) in the 2-norm (the packing G'_a + i G'_b is the stage that
        ceiling counts); `recover` multiplies an rfft bin, at most sqrt(n) ||dg||_2 (Cauchy-Schwarz), by 2 / n inside and 1 / n at
        the ends:  w_k transform_ceiling ||Y||_2 (pair), w_k = 2 inside, 1 at the ends, ||Y||_2 = inverse_norm, taken of
        |G| + the first term so that the device's own (perturbed) spectrum is what the ceiling multiplies.
    Nothing here is measured on a device."""
    n = r["n_fft"]
    G = r["G"] if G is None else G
    c1 = r["c1"] if c1 is None else c1
    dS = spectrum_error(r["S"], n) if dS is None else dS
    spec = (2.0 / r["count"]) * coefficient_bound(np.abs(r["S"]), r["P"], c1, dS[..., None], r["alpha"], r["eps"])
    yn = inverse_norm(np.abs(G) + spec, n)
    yn = np.stack([pair_norm(row, n) for row in yn])
    w = np.full(G.shape[-1], 2.0)
    w[0] = w[-1] = 1.0
    return spec + transform_ceiling(n) * yn[..., None] * w


def check_bins(r, G_dev, stock=None, lines=None, tag=""):
    """The per-bin criterion.  Every decided bin: |G_dev - G| <= max(bin_bound, CPU_FACTOR * the stock fp32 formulation's worst
    per-bin error over the decided bins of that frame).  Every undecided bin: the same against the reference evaluated with one
    of the signs {-1, 0, +1} at that bin, for each of the two sign functions (an fp32 evaluation can round P + eps and Q + eps
    to one number while P^ != Q^: the two signs need not agree), with the bound of that evaluation.  `stock` is a callable
    -> G of the stock formulation, called only if some bin exceeds its derived bound (error <= bound implies the criterion).
    -> (passed, worst error / limit, share of undecided bins); appends one line of figures to `lines`."""
    n = r["n_fft"]
    G_dev = np.asarray(G_dev, dtype=np.complex128)
    dS = spectrum_error(r["S"], n)
    und = undecided(r, dS=dS)
    limit = bin_bound(r, dS=dS)
    err = np.abs(G_dev - r["G"])
    finite = bool(np.isfinite(err).all())
    err = np.where(np.isfinite(err), err, np.inf)

    def ratio_of(e, lim):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(lim > 0, e / lim, np.where(e == 0, 0.0, np.inf))

    ratio = ratio_of(err, limit)
    idx = np.nonzero(und)
    if idx[0].size:
        # the candidates at the undecided bins only; the inverse transform's share of the bound is taken from the reference's own
        # frame norm (a flipped bin or two move that norm by their share of it; with the cap that is below 1 % here)
        S_u, P_u, Q_u = r["S"][idx], r["P"][idx], r["Q"][idx]
        inv_u = (limit - (2.0 / r["count"]) * coefficient_bound(np.abs(r["S"]), r["P"], r["c1"], dS[..., None], r["alpha"], r["eps"]))[idx]
        best = np.full(idx[0].size, np.inf)
        for sd in SIGNS:
            for se in SIGNS:
                c_u = coefficient(P_u, Q_u, r["alpha"], r["eps"], sd, se)
                G_u = (2.0 / r["count"]) * c_u * S_u
                lim_u = (2.0 / r["count"]) * coefficient_bound(np.abs(S_u), P_u, c_u, dS[idx[0], idx[1]], r["alpha"], r["eps"]) + inv_u
                best = np.minimum(best, ratio_of(np.where(np.isfinite(G_dev[idx]), np.abs(G_dev[idx] - G_u), np.inf), lim_u))
        ratio[idx] = best
    worst_bound = float(ratio.max())
    stock_used = False
    if worst_bound > 1.0 and stock is not None and finite:
        stock_used = True
        es = np.where(und, 0.0, np.abs(np.asarray(stock(), dtype=np.complex128) - r["G"]))
        floor = CPU_FACTOR * es.max(axis=-1, keepdims=True)
        over = ratio > 1.0
        alt = ratio_of(np.where(und, np.inf, err), np.broadcast_to(floor, err.shape))
        ratio = np.where(over, np.minimum(ratio, alt), ratio)
    worst = float(ratio.max())
    share = float(und.mean())
    if lines is not None:
        lines.append(f"MSS {tag}: worst error / bound {worst_bound:.4f}{f' (with the stock floor {worst:.4f})' if stock_used else ''}, "
                     f"undecided {int(und.sum())} of {und.size} bins ({100.0 * share:.3f} %)")
    return finite and worst <= 1.0, worst, share


def check_terms(r, out3, stock_terms=None, lines=None, tag=""):
    """out3 = (loss, lin, log) of the device: lin and log each within TERM_TOL of the reference, relative (a term that is exactly
    zero in the reference must be exactly zero) -- or, for a term that misses it, within CPU_FACTOR times the stock fp32
    formulation's error of that term (`stock_terms`: callable -> (lin, log)); out3[0] == fl32(out3[1] + alpha out3[2]) to one
    fp32 rounding of the sum's size.  -> (passed, worst relative error of a term / TERM_TOL)"""
    o = [float(v) for v in out3]
    ok, worst = True, 0.0
    for name, got, want in (("lin", o[1], r["lin"]), ("log", o[2], r["log"])):
        e = abs(got - want)
        rel = 0.0 if e == 0.0 else (e / abs(want) if want != 0.0 else math.inf)
        good = rel <= TERM_TOL
        if not good and stock_terms is not None and want != 0.0:
            s = dict(zip(("lin", "log"), stock_terms()))[name]
            good = e <= CPU_FACTOR * abs(s - want)
            if lines is not None:
                lines.append(f"MSS {tag}: {name} misses {TERM_TOL:g}: device {rel:.2e}, stock fp32 {abs(s - want) / abs(want):.2e}")
        ok &= good
        worst = max(worst, rel / TERM_TOL)
    total = o[1] + r["alpha"] * o[2]
    # alpha is given to the device as fp32; the finish kernel adds in fp64 and rounds once, after l and g were rounded on their own
    a32 = float(np.float32(r["alpha"]))
    slack = 2.0 * U * (abs(o[1]) + abs(a32 * o[2])) + 2.0 ** -149
    ok &= abs(o[0] - (o[1] + a32 * o[2])) <= slack and math.isfinite(total)
    if lines is not None:
        lines.append(f"MSS {tag}: lin {o[1]:.7g} (ref {r['lin']:.7g}) log {o[2]:.7g} (ref {r['log']:.7g}), worst term error / {TERM_TOL:g}: {worst:.3f}")
    return bool(ok), worst


def gather_bound(grad_frames, window, hop, L):
    """|grad_x^ - gather| per sample [B, L] of the fp32 gather kernel against the fp64 gather of the SAME fp32 frames and window:
    every contribution is one rounded product g w and then passes through at most k = ceil(n_fft / hop) + 2 rounded additions
    (the at most ceil(n_fft / hop) covering frames of a padded position one after the other, and the sums of the at most three
    padded positions of a sample):  gamma_(k+1) sum |g w|, gamma_m = m U / (1 - m U) (Higham, Accuracy and Stability, 2nd ed.,
    eq. 4.4 and lemma 3.1), the sum of the magnitudes being the same gather of |g| and |w|."""
    n = np.shape(window)[0]
    k = -(-n // hop) + 2
    g = (k + 1) * U / (1.0 - (k + 1) * U)
    return g * gather(np.abs(np.asarray(grad_frames, dtype=np.float64)), np.abs(np.asarray(window, dtype=np.float64)), hop, L)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def signals(seed, B, L, amp=0.3, zero_row=None, same_row=None):
    """(x_pred, x_true) [B, L] as rounded to fp32: amp * N(0, 1); optionally a row of zeros in the target and a row where the
    prediction IS the target."""
    rng = np.random.default_rng(seed)
    xt, xp = f32(amp * rng.standard_normal((B, L))), f32(amp * rng.standard_normal((B, L)))
    if zero_row is not None:
        xt[zero_row] = 0.0
    if same_row is not None:
        xp[same_row] = xt[same_row]
    return xp, xt


def segment_levels(rng, B, L, seg, lo=-4.0):
    """[B, L]: every seg-long segment at its own level 10^U(lo, 0)."""
    nseg = -(-L // seg)
    return np.repeat(10.0 ** rng.uniform(lo, 0.0, (B, nseg)), seg, axis=1)[:, :L]


def levelled_signals(seed, B, L, seg, onset=None):
    """Normalised audio (|x| <= 1) whose seg-long segments sit at levels 10^U(-4, 0), the prediction's and the target's drawn
    independently; row 0 of both holds a segment at 1e-4, [onset - seg, onset), directly followed by a full-scale sine onset
    (default onset: 2 seg).  With seg = hop = n_fft and onset = 5 n_fft / 2, frame 2 of row 0 is exactly the quiet segment and
    its pair partner, frame 3, starts at the onset: a quiet and a loud disjoint frame in one transform.
    -> (x_pred, x_true, levels of x_pred [B, L])"""
    rng = np.random.default_rng(seed)
    s0 = 2 * seg if onset is None else onset
    assert seg <= s0 < L - 1
    out = []
    for which in range(2):
        lev = segment_levels(rng, B, L, seg)
        x = np.clip(0.3 * rng.standard_normal((B, L)), -1.0, 1.0) * lev
        x[0, s0 - seg:s0] = 1e-4 * np.clip(0.3 * rng.standard_normal(seg), -1.0, 1.0)
        lev[0, s0 - seg:s0] = 1e-4
        m = np.arange(L - s0)
        x[0, s0:] = np.sin(2.0 * np.pi * (0.03 + 0.002 * which) * m + 0.4 * which) * (1.0 if which == 0 else 0.8)
        lev[0, s0:] = 1.0
        out.append((f32(x), lev))
    assert max(np.abs(out[0][0]).max(), np.abs(out[1][0]).max()) <= 1.0
    return out[0][0], out[1][0], out[0][1]


def level_inputs(shape):
    """(x_pred, x_true) of a LEVEL_SHAPES entry; at hop = n_fft the onset is placed so that frames 2 and 3 of row 0 are the quiet
    segment and the onset."""
    name, n, hop, B, L = shape
    xp, xt, _ = levelled_signals(n + hop, B, L, hop, onset=5 * n // 2 if hop == n else None)
    return xp, xt


# (name, n_fft, hop, B, L): the smallest shapes that reach each branch -- L = n_fft / 2 + 1 (both mirrors overlap; every frame takes
# the reflect load), an even frame count at hop 1, F = 6 and F = 7 (a last pair with one frame; with B = 1 a stray second-of-pair
# store lands in the guard), hops n_fft / 4, n_fft (overlap 0: a pair is two disjoint frames) and 3, B = 1 and 3, frames wholly
# inside the row (the unpadded fast load) and at each edge
def _shapes():
    out = []
    for n in SIZES:
        h = n // 4
        out += [(f"n{n}_shortest_h{h}", n, h, 3, n // 2 + 1), (f"n{n}_shortest_h1", n, 1, 1, n // 2 + 1),
                (f"n{n}_h{h}_F6", n, h, 3, 5 * h + 3), (f"n{n}_h{h}_F7", n, h, 1, 6 * h + 1),
                (f"n{n}_h{n}_F6", n, n, 3, 5 * n + 3), (f"n{n}_h{n}_F7", n, n, 1, 6 * n + 1),
                (f"n{n}_h3_shortest", n, 3, 3, n // 2 + 1), (f"n{n}_h3", n, 3, 1, n + 10)]
    return tuple(out)


GPU_SHAPES = _shapes()
ALPHA_EPS = ((1.0, 1e-7), (1.0, 1e-2), (0.3, 1e-7), (0.3, 1e-2))


def shape_inputs(shape):
    """(x_pred, x_true) of a GPU_SHAPES entry: B = 3 has a row of zeros in the target (row 1) and an identical row (row 2)."""
    name, n, hop, B, L = shape
    assert L > n // 2
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    return signals(seed, B, L, zero_row=1 if B == 3 else None, same_row=2 if B == 3 else None)


# more units than the grid of MAX_UNITS blocks, with small signals: (name, n_fft, hop, B, L)
BEYOND = (("n64_2turns", 64, 1, 32, 2100), ("n128_2turns", 128, 1, 17, 2000), ("n256_2turns", 256, 2, 17, 2000),
          ("n512_2turns", 512, 4, 17, 2000), ("n1024_2turns", 1024, 4, 17, 2000), ("n2048_2turns", 2048, 4, 6, 3000),
          ("n64_3turns", 64, 1, 63, 2100), ("n2048_3turns", 2048, 4, 11, 3000))

# levels inside normalised audio: (name, n_fft, hop, B, L)
def _level_shapes():
    out = []
    for n in SIZES:
        out += [(f"n{n}_levels_h{n // 4}", n, n // 4, 2, 12 * (n // 4) + 5), (f"n{n}_levels_h{n}", n, n, 2, 9 * n + 5)]
    return tuple(out)


LEVEL_SHAPES = _level_shapes()


def padded_positions(p, n_fft, L):
    """The positions of the reflect-padded row that hold sample p."""
    half = n_fft // 2
    out = [p + half]
    if 1 <= p <= half:
        out.append(half - p)
    if L - 1 - half <= p <= L - 2:
        out.append(half + 2 * (L - 1) - p)
    return out


def frames_holding(p, n_fft, hop, L, partners=True):
    """The frames of a row whose reflect-padded window holds sample p, with their pair partners (frame f ^ 1) below 2048."""
    F = 1 + L // hop
    hit = {f for q in padded_positions(p, n_fft, L) for f in range(F) if f * hop <= q < f * hop + n_fft}
    if partners and n_fft != 2048:
        hit |= {f ^ 1 for f in hit if (f ^ 1) < F}
    return sorted(hit)


def random_case(rng):
    """One random case of the sweep: dict(n_fft, hop (1 .. n_fft), B, L, alpha, eps, levels: whether hop-long segments get their
    own levels 10^U(-2, 0), seed)."""
    n = int(rng.choice(SIZES))
    hop = int(rng.choice([int(rng.integers(1, n + 1)), n // 4, n // 2, n, int(rng.integers(1, 8))]))
    B = int(rng.integers(1, 5))
    L = n // 2 + 1 + int(rng.choice([0, int(rng.integers(0, 8)), int(rng.integers(0, 4 * n))]))
    L = min(L, n // 2 + 1 + 60 * hop)                             # at most some 60 frames a row
    return dict(n_fft=n, hop=hop, B=B, L=L, alpha=float(rng.choice([1.0, 0.3, 0.0])), eps=float(10.0 ** rng.uniform(-9.0, -1.0)),
                levels=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30)))


def case_inputs(case):
    """(x_pred, x_true) of a `random_case`."""
    xp, xt = signals(case["seed"], case["B"], case["L"])
    if case["levels"]:
        rng = np.random.default_rng(case["seed"] + 1)
        xp = f32(xp * segment_levels(rng, case["B"], case["L"], case["hop"], -2.0))
        xt = f32(xt * segment_levels(rng, case["B"], case["L"], case["hop"], -2.0))
    return xp, xt


# ---- the stock fp32 formulation on the CPU ----------------------------------------------------------------------------------
def stock(x_pred, x_true, n_fft, hop, alpha, eps, window=None):
    """The same scale in torch fp32 on the CPU with the windowed frames as the leaf (rfft, powers, both L1 means, autograd)
    -> (G recovered from its gradient frames by `recover`, lin, log), all as float64 values of the fp32 results."""
    import torch
    w = window_of(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    fp = torch.from_numpy((frames_of(x_pred, np.ones(n_fft), hop).astype(np.float32) * w.astype(np.float32))).requires_grad_(True)
    ft = torch.from_numpy((frames_of(x_true, np.ones(n_fft), hop).astype(np.float32) * w.astype(np.float32)))
    S, T = torch.fft.rfft(fp, dim=-1), torch.fft.rfft(ft, dim=-1)
    P, Q = S.real.square() + S.imag.square(), T.real.square() + T.imag.square()
    lin = (P - Q).abs().mean()
    log = (torch.log2(Q + eps) - torch.log2(P + eps)).abs().mean()
    (lin + alpha * log).backward()
    return recover(fp.grad.numpy().astype(np.float64)), float(lin.detach()), float(log.detach())


# ---- the calls themselves (need a device) -----------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def device_scale(x_pred, x_true, n_fft, hop, alpha, eps, window=None, want_frames=True, expect=0):
    """One call of ddsp_mss_scale -> (grad_frames float32 [B, F, n_fft] or None, out3 float32 [3]).  grad_frames is allocated
    NaN-prefilled with GUARD floats behind it; asserts the return code and an untouched guard."""
    import ddsp_pytorch_amd as ddsp
    torch = _torch()
    lib = ddsp._lib.lib()
    xp = torch.from_numpy(np.ascontiguousarray(x_pred, dtype=np.float32)).cuda()
    xt = torch.from_numpy(np.ascontiguousarray(x_true, dtype=np.float32)).cuda()
    w = torch.from_numpy(np.ascontiguousarray(window_of(n_fft) if window is None else window, dtype=np.float32)).cuda()
    B, L = xp.shape
    F = 1 + L // hop
    nfl = B * F * n_fft
    out3 = torch.full((3 + GUARD,), 777.0, device="cuda")
    scratch = torch.empty(lib.ddsp_mss_scale_scratch_bytes(), device="cuda", dtype=torch.uint8)
    frames = None
    if want_frames:
        frames = torch.full((nfl + GUARD,), float("nan"), device="cuda")
        frames[nfl:] = 12345.0
    rc = lib.ddsp_mss_scale(xp.data_ptr(), xt.data_ptr(), w.data_ptr(), None if frames is None else frames.data_ptr(), scratch.data_ptr(),
                            out3.data_ptr(), B, L, n_fft, hop, float(alpha), float(eps), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, rc
    if rc != 0:
        return None, None
    assert bool((out3[3:] == 777.0).all()), "the finish kernel wrote behind out3"
    if frames is not None:
        assert bool((frames[nfl:] == 12345.0).all()), "the scale kernel wrote behind grad_frames"
        frames = frames[:nfl].cpu().numpy().reshape(B, F, n_fft)
    return frames, out3[:3].cpu().numpy()


def device_gather(grad_frames, window, hop, L, into=None):
    """ddsp_stft_frames_backward -> grad_x float32 [B, L]; `into` [B, L]: accumulate = 1 onto a copy of it."""
    import ddsp_pytorch_amd as ddsp
    torch = _torch()
    lib = ddsp._lib.lib()
    g = torch.from_numpy(np.ascontiguousarray(grad_frames, dtype=np.float32)).cuda()
    w = torch.from_numpy(np.ascontiguousarray(window, dtype=np.float32)).cuda()
    B, F, n = g.shape
    assert F == 1 + L // hop
    out = torch.full((B * L + GUARD,), float("nan"), device="cuda")
    out[B * L:] = 12345.0
    if into is not None:
        out[:B * L] = torch.from_numpy(np.ascontiguousarray(into, dtype=np.float32)).cuda().reshape(-1)
    rc = lib.ddsp_stft_frames_backward(g.data_ptr(), w.data_ptr(), out.data_ptr(), B, L, n, hop, 0 if into is None else 1,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((out[B * L:] == 12345.0).all()), "the gather wrote behind grad_x"
    return out[:B * L].cpu().numpy().reshape(B, L)


def device_spectral_loss(pred, truth, alpha, eps, want_grad=True, expect=0):
    """ddsp_spectral_loss on complex64 arrays [n_bins] -> (grad complex64 [n_bins] or None, out3 float32 [3])."""
    import ddsp_pytorch_amd as ddsp
    torch = _torch()
    lib = ddsp._lib.lib()
    nb = int(np.shape(pred)[0])
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.complex64).view(np.float32).copy()).cuda() if nb else torch.zeros(2, device="cuda")
    t = torch.from_numpy(np.ascontiguousarray(truth, dtype=np.complex64).view(np.float32).copy()).cuda() if nb else torch.zeros(2, device="cuda")
    out3 = torch.full((3 + GUARD,), 777.0, device="cuda")
    scratch = torch.empty(lib.ddsp_spectral_loss_scratch_bytes(), device="cuda", dtype=torch.uint8)
    grad = torch.full((2 * nb + GUARD,), float("nan"), device="cuda")
    grad[2 * nb:] = 12345.0
    rc = lib.ddsp_spectral_loss(p.data_ptr(), t.data_ptr(), grad.data_ptr() if want_grad else None, scratch.data_ptr(), out3.data_ptr(), nb,
                                float(alpha), float(eps), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, rc
    if rc != 0:
        return None, None
    assert bool((out3[3:] == 777.0).all()) and bool((grad[2 * nb:] == 12345.0).all()), "the pass wrote behind an output"
    g = grad[:2 * nb].cpu().numpy().view(np.complex64) if want_grad else None
    return g, out3[:3].cpu().numpy()


def run_case(x_pred, x_true, n_fft, hop, alpha, eps, tag, lines=None, cap=True):
    """Criteria (a) and (b) of one call: every bin (`check_bins`), the three outputs (`check_terms`), no NaN left, the same three
    floats in bits without grad_frames, and (`cap`) the share of undecided bins.  -> (passed, worst error / bound, reference, frames)"""
    lines = [] if lines is None else lines
    alpha, eps = float(np.float32(alpha)), float(np.float32(eps))          # what the entry is given
    r = scale(x_pred, x_true, n_fft, hop, alpha, eps)
    fr, o3 = device_scale(x_pred, x_true, n_fft, hop, alpha, eps)
    _, o3n = device_scale(x_pred, x_true, n_fft, hop, alpha, eps, want_frames=False)
    st = {}

    def stock_all():
        if not st:
            st["v"] = stock(x_pred, x_true, n_fft, hop, alpha, eps)
        return st["v"]

    ok1, worst, share = check_bins(r, recover(fr), stock=lambda: stock_all()[0], lines=lines, tag=tag)
    ok2, _ = check_terms(r, o3, stock_terms=lambda: stock_all()[1:], lines=lines, tag=tag)
    ok3 = bool(np.isfinite(fr).all()) and np.array_equal(bits(o3), bits(o3n))
    ok4 = share <= UNDECIDED_CAP or not cap
    if not (ok3 and ok4):
        lines.append(f"MSS {tag}: finite and out3 bits without grad_frames {ok3}, undecided share within the cap {ok4}")
    return ok1 and ok2 and ok3 and ok4, worst, r, fr
