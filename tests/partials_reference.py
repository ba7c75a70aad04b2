"""The definition of the inharmonic analysis (include/ddsp_hip.h: ddsp_partials_*) in numpy fp64, one row at a
time with a plain loop over frames, the per-element error bounds of the device kernels with their roundings counted, and the
inputs the tests share.  The phase is tests/sinusoids_reference.phases_closed_form: the bank's own.

Bound of C (and, with the second window, of D), per element.  Both parts of an element are sums over the window's samples inside
the clip of x_j cos / sin(2 pi P_j), x_j = fl32(fl32(w_j) audio_j), a wavefront accumulating J = 4 ceil(W / 16) of them in fp32:
  the sine and cosine: e_sin = EPS_SIN + 2 pi (2^-25 + E_P) on every term in the worst direction -- the hardware's v_sin_f32 /
      v_cos_f32, the reduced phase rounded to fp32 and section 5d's phase bound E_P = (T + 8) 2^-53 (|P| + 1) --
      sum_j |x_j| e_sin[j]
  fp32, in units of 2^-24 sum_j |x_j|: the window rounded to fp32 (1), the product w x (1), the J fused multiply-adds of a
      wavefront (each rounds a partial sum that is at most sum_j |x_j|) (J), the four-way sum of the wavefronts (3), the scale
      2 / norm rounded to fp32 and its product (2): J + 7, and 1 more for the second-order terms of these compounded
and sqrt(2) for the modulus of the two parts: bound = sqrt(2) (2 / norm) sum_j |x_j| (e_sin[j] + (J + 8) 2^-24).
f_re: with the unscaled sums and their bounds bC, bD, num = Im(D conj C) and den = |C|^2 move by at most
  dnum = |D| bC + |C| bD + bC bD + 3 2^-24 |D| |C|   and   dden = 2 |C| bC + bC^2 + 3 2^-24 |C|^2
(the last terms: the product, the fused multiply-add and the conversion of the fp32 expressions), so q = num / den by at most
(dnum + |q| dden) / (den - dden) to first order, and f_re by sr / (2 pi) of that plus 2^-23 |f| for the window mean (fp32 window
weights) and the fp32 store.  It is asserted only where |C| >= 10^-3 of the row's largest.
a is held to the sum of its C bounds.  c = amp / a moves by at most (bound_k + c_k sum_k' bound_k') / (a - sum_k' bound_k'), which
is asserted where a is well above the bound (100 times); it is never more than (K + 1) max_k bound / a, and at K = 256 far less.
The resynthesis of a given C is held to sum_k |up C| e_sin + (K + 8) 2^-24 sum_k |up C|.
"""
import numpy as np

import harmonic_analysis_reference as ref
import sinusoids_reference as sref
from harmonic_analysis_reference import EPS_SIN
from sinusoids_reference import EPS, EPS64, phases_closed_form

# (B, T, hop, W, K, sr) of the device tests
GPU_SHAPES = [(2, 16, 64, 256, 20, 16000), (3, 24, 64, 512, 70, 16000), (1, 20, 128, 1024, 100, 16000), (2, 40, 7, 64, 5, 16000),
              (2, 6, 128, 64, 8, 16000), (1, 1, 64, 256, 20, 16000), (1, 8, 512, 2048, 256, 44100)]
R_C = 8                     # the counted fp32 roundings of an element of C beside a wavefront's J accumulations (header)


def usable(f):
    with np.errstate(invalid="ignore"):
        return np.isfinite(f) & (f > 0)


def as_given(f, cast=True):
    """The tracks as the path under test sees them: fp32 values for the kernels, the fp64 values themselves otherwise."""
    return np.asarray(f, np.float32 if cast else np.float64)


def increments(f, sr, cast=True):
    """f [T, K] -> g = (double) f / sr where f is usable, else 0."""
    fv = as_given(f, cast)
    return np.where(usable(fv), np.where(usable(fv), fv, 0).astype(np.float64) / np.float64(sr), 0.0)


def phases(f, hop, sr, cast=True):
    """f [T, K] -> P [T hop, K] in turns: the bank's phase with P0 = 0."""
    return phases_closed_form(increments(f, sr, cast)[None], hop)[0]


def keep_mask(f, sr, voiced=None, cast=True):
    """[T, K]: a usable entry that is not above the bank's mask, on a voiced frame."""
    fv = as_given(f, cast)
    with np.errstate(invalid="ignore"):
        keep = usable(fv) & ~(fv > fv.dtype.type(sr // 2))
    if voiced is not None:
        keep = keep & np.asarray(voiced, dtype=bool)[:, None]
    return keep


def windows(W):
    """The periodic Hann window and its derivative per sample."""
    j = np.arange(W)
    return 0.5 - 0.5 * np.cos(2 * np.pi * j / W), (np.pi / W) * np.sin(2 * np.pi * j / W)


def interior_frames(T, hop, W):
    return [t for t in range(T) if ref.frame_start(t, hop, W) >= 0 and ref.frame_start(t, hop, W) + W <= T * hop]


def sine_allowance(P, T):
    """e_sin per (sample, partial): EPS_SIN + 2 pi (2^-25 + E_P)."""
    return EPS_SIN + 2.0 * np.pi * (2.0 ** -25 + (T + 8) * EPS64 * (np.abs(P) + 1.0))


def analyse(audio, f, hop, sr, W, voiced=None, frames=None, cast=True):
    """One row: audio [T hop], f [T, K] -> dict of
      C [T, K] complex, a [T], c [T, K], f_re [T, K] (f where it is not defined), measured [T, K] (where f_re is defined),
      Cu, Du [T, K]: the unscaled sums under w and w' (masked like C),
      bound_C, bound_Cu, bound_Du, bound_a [T], bound_c [T, K] (inf where a is not well above its bound), bound_f [T, K] (inf where
      it is not asserted: |C| below 10^-3 of the row's largest), and `vacuous`: the number of entries at or above that level whose
      den is within twice its own bound, where the first-order bound says nothing -- the tests assert that there is none.
    `frames`: only these are computed (the rest stay 0 / f)."""
    audio = np.asarray(audio, dtype=np.float64)
    fv = as_given(f, cast).astype(np.float64)
    T, K = fv.shape
    N = len(audio)
    assert N == T * hop and W % 2 == 0
    P = phases(f, hop, sr, cast)
    turns = P - np.floor(P)
    e_sin = sine_allowance(P, T)
    fup = ref.up(np.where(usable(fv), fv, 0.0), hop)
    keep = keep_mask(f, sr, voiced, cast)
    inter = set(interior_frames(T, hop, W))
    w, wd = windows(W)
    j = np.arange(W)
    J = ((W + 15) // 16) * 4
    out = {k: np.zeros((T, K), dtype=np.complex128) for k in ("C", "Cu", "Du")}
    out.update({k: np.zeros((T, K)) for k in ("bound_C", "bound_Cu", "bound_Du")})
    f_re, measured, bound_f = fv.copy(), np.zeros((T, K), dtype=bool), np.full((T, K), np.inf)
    vacuous = np.zeros((T, K), dtype=bool)
    for t in (range(T) if frames is None else frames):
        n = ref.frame_start(t, hop, W) + j
        inside = (n >= 0) & (n < N)
        n, wj, wdj = n[inside], w[inside], wd[inside]
        x = audio[n]
        with np.errstate(invalid="ignore"):
            e = np.exp(-2j * np.pi * turns[n])
            Cu, Du = ((wj * x)[:, None] * e).sum(axis=0), ((wdj * x)[:, None] * e).sum(axis=0)
            ax, ad = np.abs(wj * x), np.abs(wdj * x)
            bCu = np.sqrt(2.0) * ((ax[:, None] * e_sin[n]).sum(axis=0) + (J + R_C) * EPS * ax.sum())
            bDu = np.sqrt(2.0) * ((ad[:, None] * e_sin[n]).sum(axis=0) + (J + R_C) * EPS * ad.sum())
        scale = 2.0 / wj.sum()
        k = keep[t]
        out["Cu"][t], out["Du"][t] = np.where(k, Cu, 0.0), np.where(k, Du, 0.0)
        out["C"][t] = np.where(k, scale * Cu, 0.0)
        out["bound_Cu"][t], out["bound_Du"][t], out["bound_C"][t] = np.where(k, bCu, 0.0), np.where(k, bDu, 0.0), np.where(k, scale * bCu, 0.0)
        if t in inter:
            mean = (w[:, None] * fup[n]).sum(axis=0) / w.sum()
            aC, aD = np.abs(Cu), np.abs(Du)
            num, den = (Du * np.conj(Cu)).imag, aC ** 2
            with np.errstate(invalid="ignore", divide="ignore"):
                q = num / den
                value = mean - sr / (2 * np.pi) * q
                ok = k & (den != 0) & np.isfinite(value)
                dnum = aD * bCu + aC * bDu + bCu * bDu + 3 * EPS * aD * aC
                dden = 2 * aC * bCu + bCu ** 2 + 3 * EPS * den
                df = sr / (2 * np.pi) * (dnum + np.abs(q) * dden) / (den - dden) + 2.0 ** -23 * np.abs(fv[t])
            f_re[t] = np.where(ok, value, fv[t])
            measured[t] = ok
            bound_f[t] = np.where(ok & (den > 2 * dden), df, np.inf)
            vacuous[t] = ok & ~(den > 2 * dden)
    amp = np.abs(out["C"])
    a = amp.sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(a[:, None] == 0, 1.0 / K, amp / a[:, None])
        bound_a = out["bound_C"].sum(axis=-1)
        bound_c = np.where((a > 100 * bound_a)[:, None], (out["bound_C"] + c * bound_a[:, None]) / (a - bound_a)[:, None], np.inf)
        largest = np.nanmax(np.where(np.isfinite(amp), amp, 0.0)) if amp.size else 0.0
        bound_f = np.where(amp >= 1e-3 * largest, bound_f, np.inf)
        vacuous = vacuous & (amp >= 1e-3 * largest)
    out.update(vacuous=int(vacuous.sum()), a=a, c=c, f_re=f_re, measured=measured, bound_a=bound_a, bound_c=bound_c, bound_f=bound_f, keep=keep)
    return out


def resynth(C, f, hop, sr, cast=True):
    """One row: C [T, K] along f [T, K] -> (harm [T hop], its device bound [T hop])."""
    C = np.asarray(C, dtype=np.complex128)
    T, K = C.shape
    P = phases(f, hop, sr, cast)
    cu = ref.up(C.real, hop) + 1j * ref.up(C.imag, hop)
    harm = (cu * np.exp(2j * np.pi * (P - np.floor(P)))).real.sum(axis=-1)
    mag = np.abs(cu)
    return harm, (mag * sine_allowance(P, T)).sum(axis=-1) + (K + 8) * EPS * mag.sum(axis=-1)


def stretched(K, B_coef, base=None):
    r = np.arange(1, K + 1, dtype=np.float64) if base is None else np.asarray(base, np.float64)
    return r * np.sqrt(1.0 + B_coef * r * r)


def cents(f, g):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / np.asarray(g, np.float64))


def string_tone(f0, B_coef, K, T, hop, sr, a=0.5, weights=None):
    """A steady stiff string through the bank's own forward (fp64): f0 Hz, partials f0 rho_k(B), weights ~ 1 / k, loudness a.
    -> (audio [T hop], f [T, K] fp64, the amplitudes a wn [K])"""
    f = np.tile(f0 * stretched(K, B_coef), (T, 1))
    wgt = 1.0 / np.arange(1, K + 1) if weights is None else np.asarray(weights, np.float64)
    y = sref.forward(f[None], np.tile(wgt, (1, T, 1)), np.full((1, T, 1), a), hop, sr, cast=False)["y"][0]
    return y, f, a * wgt / wgt.sum()


def residual_share(audio, resid, T, hop, W):
    """rms of the residual over rms of the audio, on the samples that interpolate interior frames only."""
    _, samples = ref.interior(T, hop, W)
    return float(np.sqrt(np.mean(np.asarray(resid, np.float64)[samples] ** 2) / np.mean(np.asarray(audio, np.float64)[samples] ** 2)))


def string_rows(B, T, hop, W, K, sr, seed=0):
    """The device tests' rows: (audio [B, T hop] fp32 with peak 1, f [B, T, K] fp32, voiced [B, T]).  A stiff string (B k^2 up to
    4 %) plus noise on an f0 that glides across sr / (2 K) -- so the top partials are masked in some frames and live in others --
    with one detuned pair 3 Hz apart; from four frames on the tracks hold a zero, a negative, a NaN and an above-Nyquist entry;
    voiced is false on the frame before the last, where there are three frames."""
    rng = np.random.default_rng(2000 + seed)
    audio = np.empty((B, T * hop), dtype=np.float32)
    f = np.empty((B, T, K), dtype=np.float32)
    voiced = np.ones((B, T), dtype=bool)
    edge = (sr // 2) / K
    rho = stretched(K, 0.04 / K ** 2)
    for b in range(B):
        lo, hi = (0.7, 1.4) if b % 2 == 0 else (1.3, 0.8)
        f0 = edge * lo * (hi / lo) ** ((np.arange(T) + rng.uniform(0, 1)) / max(T, 2))
        track = f0[:, None] * rho[None, :]
        if K >= 3:
            track[:, 2] = track[:, 1] + 3.0
        track = track.astype(np.float32)
        a = rng.uniform(0.3, 1.0, (1, T, 1))
        c = rng.uniform(0.1, 1.0, (1, T, K)) / np.arange(1, K + 1)[None, None, :] ** 0.5
        y = sref.forward(track[None], c, a, hop, sr)["y"][0] + 0.05 * rng.standard_normal(T * hop)
        audio[b] = (y / np.abs(y).max()).astype(np.float32)
        audio[b] /= np.abs(audio[b]).max()
        f[b] = track
        if T >= 4:
            at = rng.choice(T, 4, replace=False)
            ks = rng.choice(K, 4, replace=K < 4)
            f[b, at, ks] = (0.0, -track[at[1], ks[1]], np.nan, float(sr))
        if T >= 3:
            voiced[b, T - 2] = False
    return audio, f, voiced
