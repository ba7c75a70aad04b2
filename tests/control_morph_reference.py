"""The definition of the control morph in numpy fp64, one row at a time, the same definition in the
kernel's own arithmetic (fp32 combinations, u in fp64, the kernel's summation order), and the inputs of the tests.  What the morph
shares with the transformation (section 14b: the played amplitudes, the envelope, the sums) is taken from
control_transform_reference.

One row: per sound X in {a, b} a dict with f0 [T_X], a [T_X], c [T_X, H_X] (fp32 values), optionally noise bands N [T_X, F], and
pos [T'], the source position of every output frame in X's frames; the weights w_f, w_h, w_n [T'] of sound B (fp32 arrays, as the
package hands them to the kernel).

  A_X[i, k], E_X,i(u), i0, i1, lam_X   section 14b, rules 1 to 3
  f_X        fl32((1 - lam_X) f0[i0] + lam_X f0[i1]) where both are voiced, the voiced one's f0 where one is
  present_X  one of the two is voiced
  frame t'   a weight that is not finite: silent -- f0' = 0, A' = 0, a' = 0, c' = 1 / H', N' = 0; else each is clamped to [0, 1]
             f0' = f_a at w_f = 0, f_b at w_f = 1, else fl32(exp2((1 - w_f) log2 f_a + w_f log2 f_b)) in fp64, kept within
                   [min(f_a, f_b), max(f_a, f_b)];  one sound present: its f_X;  none: 0
             u_X = k' ('harmonic') or (double)k' ((double)f0' / (double)f_X) ('hz'), k' = 1 .. H'
             e_X[k'] = (1 - lam_X) E_X,i0(u_X) + lam_X E_X,i1(u_X), 0 where X is not present
             A'[k'] = (1 - w_h) e_a + w_h e_b; 0 where fl32(k' f0') > sample_rate // 2
             a' = sum A', c' = A' / a', and 1 / H' where a' = 0
             N'[j] = (1 - w_n) X_a[j] + w_n X_b[j], X_X[j] = (1 - lam_X) N_X[i0, j] + lam_X N_X[i1, j] (voicing plays no part)

TOL_M bounds |A'_device - A'_fp64| relative to the largest A of the frame's four source rows (and the same for N' relative to the
largest band of the four).  tests/test_control_morph_host.py derives it: `morph_fp32` below is the kernel's arithmetic operation by
operation, its difference from fp64 on the device tests' own inputs is measured there, and TOL_M is twice that, rounded up.
f0' through exp2 / log2 may differ by one fp32 ulp between two double-precision libraries, so `morph` takes the f0' to evaluate
the amplitudes at (teacher forcing), and that f0' is held to the one-ulp bound on its own.
"""
import numpy as np

import control_transform_reference as tref
from control_transform_reference import convex32, wave_sum32  # noqa: F401

SAMPLE_RATE = tref.SAMPLE_RATE
TOL_M = 3e-7
COORDINATES = ("hz", "harmonic")
GPU_SHAPES = [(1, 1, 1, 1, 1, 1, 1, 2), (3, 7, 9, 5, 5, 3, 5, 2), (2, 9, 12, 23, 100, 80, 100, 65), (2, 16, 11, 16, 180, 180, 180, 195),
              (2, 12, 8, 12, 64, 65, 64, 65), (1, 8, 10, 8, 65, 64, 130, 65), (2, 10, 7, 9, 100, 120, 37, 33),
              (1, 4, 3, 9, 256, 200, 256, 257)]                  # (B, T_a, T_b, T', H_a, H_b, H', F)
GRID_SHAPE = (1, 3, 2, 8192 * 4 + 5, 2, 3, 4, 2)                # five frames more than the kernel's largest grid holds at once


def source_map(f0, pos):
    """One sound's frame pairs: i0, i1, lam (fp64; an fp32 value), f (fp32; 1 where the sound is absent) and present."""
    f = np.asarray(f0, dtype=np.float32)
    T = len(f)
    p = np.asarray(pos, np.float32).astype(np.float64)
    p = np.clip(np.where(np.isnan(p), 0.0, p), 0.0, float(T - 1))
    i0 = np.floor(p).astype(np.int64)
    i1 = np.minimum(i0 + 1, T - 1)
    lam = p - i0
    voiced = tref.voiced_of(f)
    v0, v1 = voiced[i0], voiced[i1]
    with np.errstate(invalid="ignore", over="ignore"):
        glide = ((1.0 - lam) * f[i0].astype(np.float64) + lam * f[i1].astype(np.float64)).astype(np.float32)
    present = v0 | v1
    fx = np.where(v0 & v1, glide, np.where(v0, f[i0], f[i1]))
    return dict(i0=i0, i1=i1, lam=lam, v0=v0, v1=v1, present=present, f=np.where(present, fx, np.float32(1)).astype(np.float32))


def weights(wf, wh, wn):
    """-> sane [T'] and the three weights clamped to [0, 1] (fp32; 0 on the frames that are not sane)."""
    w = [np.asarray(v, np.float32) for v in (wf, wh, wn)]
    sane = np.isfinite(w[0]) & np.isfinite(w[1]) & np.isfinite(w[2])
    return sane, [np.clip(np.where(sane, v, np.float32(0)), np.float32(0), np.float32(1)).astype(np.float32) for v in w]


def pitch(ma, mb, wf):
    """f0' fp32 [T'] from the two (sane-masked) source maps and the clamped pitch weight."""
    fa, fb = ma["f"], mb["f"]
    w = wf.astype(np.float64)
    mean = np.exp2((1.0 - w) * np.log2(fa.astype(np.float64)) + w * np.log2(fb.astype(np.float64))).astype(np.float32)
    mean = np.minimum(np.maximum(mean, np.minimum(fa, fb)), np.maximum(fa, fb))
    both = np.where(wf == 0, fa, np.where(wf == 1, fb, mean))
    return np.where(ma["present"] & mb["present"], both, np.where(ma["present"], fa, np.where(mb["present"], fb, np.float32(0)))).astype(np.float32)


def frame_map(xa, xb, wf, wh, wn, coordinates, f0=None):
    """What both evaluations share, all exact or fp64: the weights, the source maps (present only on sane frames), f0' (fp32; the
    argument `f0` replaces the definition's own: teacher forcing) and u_a, u_b [T', H'] are formed from it by the caller."""
    assert coordinates in COORDINATES
    sane, (wf, wh, wn) = weights(wf, wh, wn)
    ma, mb = source_map(xa["f0"], xa["pos"]), source_map(xb["f0"], xb["pos"])
    for m in (ma, mb):
        m["present"] = m["present"] & sane
        m["f"] = np.where(m["present"], m["f"], np.float32(1)).astype(np.float32)
    own = pitch(ma, mb, wf)
    both = ma["present"] & mb["present"]
    f0o = own if f0 is None else np.asarray(f0, np.float32)
    for m in (ma, mb):
        m["scale"] = np.where(m["present"], f0o.astype(np.float64) / m["f"].astype(np.float64), 1.0) if coordinates == "hz" else np.ones(len(f0o))
    return dict(sane=sane, wf=wf, wh=wh, wn=wn, ma=ma, mb=mb, f0=f0o, f0_definition=own, pa=ma["present"], pb=mb["present"],
                live=ma["present"] | mb["present"], selected=~both | (wf == 0) | (wf == 1))


def morph(xa, xb, wf, wh, wn, sr, H_out, coordinates, f0=None):
    """The definition in fp64 -> dict(f0 fp32 [T'], a [T'], c [T', H'], A [T', H'], N [T', F] or None, scale, nscale, the frame map and
    ua, ub, masked); scale [T'] the largest A of the four source rows, nscale the largest band."""
    m = frame_map(xa, xb, wf, wh, wn, coordinates, f0)
    k = np.arange(1, H_out + 1, dtype=np.float64)[None, :]
    e, scale, u = [], 0.0, []
    for x, s in ((xa, m["ma"]), (xb, m["mb"])):
        A = tref.source_amplitudes(x["f0"], x["a"], x["c"], sr)
        lam = s["lam"][:, None]
        ux = k * s["scale"][:, None]
        ex = (1.0 - lam) * tref.envelope(A[s["i0"]], ux) + lam * tref.envelope(A[s["i1"]], ux)
        e.append(np.where(s["present"][:, None], ex, 0.0))
        u.append(ux)
        scale = np.maximum(scale, np.maximum(A[s["i0"]].max(-1), A[s["i1"]].max(-1)))
    wh64 = m["wh"].astype(np.float64)[:, None]
    out = (1.0 - wh64) * e[0] + wh64 * e[1]
    masked = tref.out_mask(m["f0"], sr, H_out)
    out = np.where(m["live"][:, None] & ~masked, out, 0.0)
    total = out.sum(-1)
    cn = np.where(total[:, None] == 0, 1.0 / H_out, out / np.where(total == 0, 1.0, total)[:, None])
    res = dict(m, ua=u[0], ub=u[1], masked=masked, a=total, c=cn, A=out, N=None, scale=scale)
    if xa.get("N") is not None:
        X, nscale = [], 0.0
        for x, s in ((xa, m["ma"]), (xb, m["mb"])):
            N = np.asarray(x["N"], np.float64)
            lam = s["lam"][:, None]
            X.append((1.0 - lam) * N[s["i0"]] + lam * N[s["i1"]])
            nscale = np.maximum(nscale, np.maximum(np.abs(N[s["i0"]]).max(-1), np.abs(N[s["i1"]]).max(-1)))
        wn64 = m["wn"].astype(np.float64)[:, None]
        res["N"] = np.where(m["sane"][:, None], (1.0 - wn64) * X[0] + wn64 * X[1], 0.0)
        res["nscale"] = nscale
    return res


def morph_fp32(xa, xb, wf, wh, wn, sr, H_out, coordinates, f0=None):
    """The same in the kernel's arithmetic -> dict(f0, a, c fp32, N fp32 or None)."""
    m = frame_map(xa, xb, wf, wh, wn, coordinates, f0)
    k = np.arange(1, H_out + 1, dtype=np.float64)[None, :]
    e = []
    for x, s in ((xa, m["ma"]), (xb, m["mb"])):
        c32 = np.where(tref.keep_mask(x["f0"], sr, x["c"].shape[-1]), np.asarray(x["c"], np.float32), np.float32(0))
        S = wave_sum32(c32)
        with np.errstate(invalid="ignore", divide="ignore"):
            gain = np.where(S == 0, np.float32(0), np.asarray(x["a"], np.float32) / np.where(S == 0, np.float32(1), S)).astype(np.float32)
        A = c32 * gain[:, None]
        ux = k * s["scale"][:, None]
        ex = convex32(s["lam"].astype(np.float32)[:, None], tref.envelope(A[s["i0"]], ux), tref.envelope(A[s["i1"]], ux))
        e.append(np.where(s["present"][:, None], ex, np.float32(0)).astype(np.float32))
    out = convex32(m["wh"][:, None], e[0], e[1])
    out = np.where(m["live"][:, None] & ~tref.out_mask(m["f0"], sr, H_out), out, np.float32(0)).astype(np.float32)
    total = wave_sum32(out)
    with np.errstate(invalid="ignore", divide="ignore"):
        cn = np.where(total[:, None] == 0, np.float32(1) / np.float32(H_out), out / np.where(total == 0, np.float32(1), total)[:, None])
    res = dict(f0=m["f0"], a=total, c=cn.astype(np.float32), N=None)
    if xa.get("N") is not None:
        X = [convex32(s["lam"].astype(np.float32)[:, None], np.asarray(x["N"], np.float32)[s["i0"]], np.asarray(x["N"], np.float32)[s["i1"]])
             for x, s in ((xa, m["ma"]), (xb, m["mb"]))]
        res["N"] = np.where(m["sane"][:, None], convex32(m["wn"][:, None], X[0], X[1]), np.float32(0)).astype(np.float32)
    return res


def linear_positions(T, T_out):
    """pos fp32 [T'] of the linear map of T frames onto T': (t' + 1/2) T / T' - 1/2 clamped to [0, T - 1]."""
    return np.clip((np.arange(T_out, dtype=np.float64) + 0.5) * T / T_out - 0.5, 0.0, float(T - 1)).astype(np.float32)


def nyquist_margin(f0o, sr, H_out):
    """The smallest distance of fl32(k' f) from sr // 2, in fp32 ulps of sr // 2, over k' = 1 .. H', the frames with f0' > 0 and f
    = f0' and its two fp32 neighbours: at 4 or more a one-ulp difference in f0' cannot flip the output's Nyquist mask."""
    f = np.asarray(f0o, np.float32)
    f = f[f > 0]
    if not len(f):
        return np.inf
    k = np.arange(1, H_out + 1, dtype=np.float32)[None, :]
    worst = np.inf
    with np.errstate(over="ignore"):
        for g in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))):
            prod = (k * g[:, None]).astype(np.float32)
            worst = min(worst, float(np.abs(prod.astype(np.float64) - (sr // 2)).min() / np.spacing(np.float32(sr // 2))))
    return worst


def row_of(x, b):
    """Row b of a batch made by `rows` -> (sound A, sound B, w_f, w_h, w_n) as `morph` takes them."""
    return ({k: v[b] for k, v in x["a"].items()}, {k: v[b] for k, v in x["b"].items()}, x["wf"][b], x["wh"][b], x["wn"][b])


def _rows(shape, seed):
    B, T_a, T_b, T_out, H_a, H_b, H_out, F = shape
    rng = np.random.default_rng(1000 * seed + 7 * T_a + 11 * T_b + 13 * T_out + H_a + 3 * H_b + F)
    sounds = []
    for T, H, quiet in ((T_a, H_a, ((4, 2, 0.0), (7, 4, 0.0), (7, 5, np.nan), (9, 7, -1.0))),
                        (T_b, H_b, ((7, 1, 0.0), (7, 2, np.nan), (8, 5, -1.0)))):
        t = np.arange(T)[None, :] / max(1, T - 1)
        f0 = ((SAMPLE_RATE / 2 / H) * (0.7 + 0.7 * np.abs(np.sin(np.pi * (t * rng.uniform(0.5, 1.5, (B, 1)) + rng.uniform(0, 1, (B, 1))))))).astype(np.float32)
        for least, frame, value in quiet:                       # unvoiced frames (0, NaN, negative), alone and in runs
            if T >= least:
                f0[:, frame] = value if value != -1.0 else -f0[:, frame]
        sounds.append(dict(f0=f0, a=rng.uniform(0.1, 1.0, (B, T)).astype(np.float32),
                           c=(rng.uniform(0.05, 1.0, (B, T, H)) / np.sqrt(np.arange(1, H + 1))).astype(np.float32),
                           N=rng.uniform(0.0, 1.0, (B, T, F)).astype(np.float32)))
    # positions: integers, T - 1, outside the range both ways, inside a run of unvoiced frames (no sound present, then one), and
    # halfway between a voiced and an unvoiced frame (the fade)
    fixed = [[1.0 if T_a > 1 else 0.0, T_a - 1.0, -0.75, T_a + 2.5, 4.5 if T_a >= 7 else 0.0, 4.5 if T_a >= 7 else 0.0, 1.5 if T_a >= 4 else 0.0],
             [T_b - 1.0, 1.0 if T_b > 1 else 0.0, T_b + 2.5, -3.0, 1.5 if T_b >= 7 else 0.0, None, 0.5 if T_b >= 7 else 0.0]]
    for sound, T, values in zip(sounds, (T_a, T_b), fixed):
        pos = rng.uniform(0.0, T - 1.0, (B, T_out))
        pos[:, ::3] = np.round(pos[:, ::3])
        for i, value in enumerate(values[:T_out]):
            if value is not None:
                pos[:, i] = value
        sound["pos"] = pos.astype(np.float32)
    # weights: below 0 and above 1, exactly 0 and 1, and not finite
    w = rng.uniform(-0.3, 1.3, (3, B, T_out)).astype(np.float32)
    w[:, :, 3::4], w[:, :, 5::8] = 0.0, 1.0
    if T_out >= 8:
        w[1, :, 7] = np.nan
    if T_out >= 9:
        w[0, :, 8] = np.inf
    return dict(a=sounds[0], b=sounds[1], wf=w[0], wh=w[1], wn=w[2])


def rows(shape, seed=0):
    """The inputs of one shape (B, T_a, T_b, T', H_a, H_b, H', F) at 16 kHz: per sound f0 [B, T_X] gliding around the pitch whose top
    harmonic crosses Nyquist, with unvoiced frames; a, c > 0, N >= 0; pos [B, T']; the three weights [B, T'] in [-0.3, 1.3] with exact
    0 and 1 and values that are not finite.  Drawn again (another seed) until every fl32(k' f0') is 4 ulps or more from Nyquist
    for f0' and its two neighbours, so that one ulp in f0' cannot flip the output mask."""
    B, H_out = shape[0], shape[6]
    for attempt in range(16):
        x = _rows(shape, seed + 100 * attempt)
        f0o = np.concatenate([frame_map(*row_of(x, b), "hz")["f0"] for b in range(B)])
        if nyquist_margin(f0o, SAMPLE_RATE, H_out) >= 4:
            return x
    raise AssertionError(f"no inputs clear of Nyquist for {shape}")


def branches(want, x):
    """How often the frames of `want` (morph's answer of one row made from the inputs x of `row_of`) take each branch."""
    xa, xb = x[0], x[1]
    H_a, H_b = xa["c"].shape[-1], xb["c"].shape[-1]
    ua, ub = want["ua"][want["pa"]], want["ub"][want["pb"]]
    raw = [np.asarray(v, np.float32) for v in x[2:5]]
    count = lambda *masks: int(sum(np.sum(v) for v in masks))                                       # noqa: E731
    edge = lambda p, T: count(p == T - 1)                                                           # noqa: E731
    T_a, T_b = len(xa["f0"]), len(xb["f0"])
    return dict(both=count(want["pa"] & want["pb"]), one=count(want["pa"] != want["pb"]), none=count(want["sane"] & ~want["live"]),
                glide=count(want["pa"] & want["pb"] & ~want["selected"]),
                below=count(ua < 1, ub < 1), above=count(ua > H_a, ub > H_b), top=count(ua == H_a, ub == H_b),
                between=count((ua >= 1) & (ua < H_a), (ub >= 1) & (ub < H_b)),
                masked=count(want["masked"][want["live"]]), audible=count(~want["masked"][want["live"]]),
                weight_low=count(*(v < 0 for v in raw)), weight_high=count(*(v > 1 for v in raw)),
                weight_nan=count(*(~np.isfinite(v) for v in raw)),
                pos_integer=count(xa["pos"] == np.round(xa["pos"]), xb["pos"] == np.round(xb["pos"])),
                pos_last=edge(xa["pos"], T_a) + edge(xb["pos"], T_b),
                pos_outside=count(xa["pos"] < 0, xa["pos"] > T_a - 1, xb["pos"] < 0, xb["pos"] > T_b - 1))


def formant_tone(T, H, f0, formants):
    """A steady tone under formants ((centre Hz, width Hz, gain), ...) at 16 kHz: controls f0 [T], a [T], c [T, H] fp32."""
    f = f0 * np.arange(1, H + 1)
    env = sum(g * np.exp(-0.5 * ((f - fc) / bw) ** 2) for fc, bw, g in formants) + 1e-3
    c = np.tile((env / env.sum()).astype(np.float32), (T, 1))
    return np.full(T, f0, dtype=np.float32), np.full(T, 0.5, dtype=np.float32), c
