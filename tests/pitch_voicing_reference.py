"""The definition of `pitch_voicing` (include/ddsp_hip.h: ddsp_pitch_voicing) as plain loops over one
row, independent of the package, and the seeded inputs its tests share.

"Lower median" of (value, frame) pairs: sort ascending by value, then by frame; take element (count - 1) div 2."""
import bisect

import numpy as np

CENTS_OF_BIN_0 = 1997.3794084376191
FILLS = ("none", "hold", "interpolate")
UPPER, LOWER = np.float32(0.31), np.float32(0.19)
SILENCE = np.float32(0.4)


def lower_median(pairs):
    pairs = sorted(pairs)                       # tuples compare by value first (-0.0 == 0.0), then by frame
    return pairs[(len(pairs) - 1) // 2]


def freq_of(n_out):
    """fl32(10 * 2^((7180 n + 1997.3794084376191) / 1200)), evaluated in fp64 and rounded once"""
    cents = 7180.0 * float(n_out) + CENTS_OF_BIN_0
    return np.float32(10.0 * 2.0 ** (cents / 1200.0))


def voicing_row(f0, n, p, loud=None, state=None, period_window=3, pitch_window=3, upper=0.31, lower=0.19, silence=None,
                fill="hold"):
    """One row, fp32 arrays [T] -> dict(f0, normalized, voiced, periodicity, state [3], interpolated [T] bool)."""
    assert fill in FILLS and period_window in (1, 3, 5, 7, 9) and pitch_window in (1, 3, 5, 7, 9)
    T = len(p)
    upper, lower = np.float32(upper), np.float32(lower)
    hp, hf = (period_window - 1) // 2, (pitch_window - 1) // 2
    # 1. periodicity
    q = [0.0 if np.isnan(x) else float(x) for x in p]
    ps = np.empty(T, dtype=np.float32)
    for t in range(T):
        ps[t] = lower_median([(q[u], u) for u in range(max(0, t - hp), min(T, t + hp + 1))])[0]
    # 2. hysteresis, 3. gate
    v = bool(state is not None and state[0] != 0)
    m = np.zeros(T, dtype=bool)
    for t in range(T):
        if ps[t] >= upper:
            v = True
        elif ps[t] < lower:
            v = False
        loud_ok = True
        if loud is not None and silence is not None:
            loud_ok = bool(loud[t] >= np.float32(silence))
        m[t] = v and bool(np.isfinite(n[t])) and loud_ok
    # 4. voiced pitch
    sn = np.array(n, dtype=np.float32)
    sf = np.array(f0, dtype=np.float32)
    for t in range(T):
        if m[t]:
            _, u = lower_median([(float(n[u]), u) for u in range(max(0, t - hf), min(T, t + hf + 1)) if m[u]])
            sn[t], sf[t] = n[u], f0[u]
    # 5. unvoiced frames
    virtual = state is not None and not np.isnan(state[1])
    out_n, out_f = sn.copy(), sf.copy()
    interpolated = np.zeros(T, dtype=bool)
    voiced_frames = [t for t in range(T) if m[t]]
    for t in range(T):
        if m[t] or fill == "none":
            continue
        k = bisect.bisect_left(voiced_frames, t)          # voiced_frames[:k] lie before t, voiced_frames[k:] after it
        a = voiced_frames[k - 1] if k > 0 else (-1 if virtual else None)
        b = voiced_frames[k] if k < len(voiced_frames) else None
        if a is None and b is None:
            continue
        na, fa = (np.float32(state[1]), np.float32(state[2])) if a == -1 else ((sn[a], sf[a]) if a is not None else (None, None))
        if fill == "interpolate" and a is not None and b is not None:
            with np.errstate(all="ignore"):
                w = np.float32(t - a) / np.float32(b - a)
                d = np.float32(sn[b] - na)
                out_n[t] = na + np.float32(d * w)
                out_f[t] = freq_of(out_n[t])
            interpolated[t] = True
        elif a is not None:
            out_n[t], out_f[t] = na, fa
        else:
            out_n[t], out_f[t] = sn[b], sf[b]
    # 6. state
    if voiced_frames:
        last = (sn[voiced_frames[-1]], sf[voiced_frames[-1]])
    elif virtual:
        last = (np.float32(state[1]), np.float32(state[2]))
    else:
        last = (np.float32(np.nan), np.float32(np.nan))
    state_out = np.array([1.0 if v else 0.0, last[0], last[1]], dtype=np.float32)
    return dict(f0=out_f, normalized=out_n, voiced=m, periodicity=ps, state=state_out, interpolated=interpolated)


def voicing(f0, n, p, loud=None, state=None, **kw):
    """Rows [B, T] -> the same dict of [B, T] (state [B, 3])."""
    rows = [voicing_row(f0[r], n[r], p[r], None if loud is None else loud[r], None if state is None else state[r], **kw)
            for r in range(len(p))]
    return {k: np.stack([row[k] for row in rows]) for k in rows[0]}


def make(seed, B, T, nans=False, kind="walk"):
    """Seeded inputs dict(f0, n, p, loud) of fp32 [B, T].
      p     a clipped random walk through both thresholds with long stays in the band and long gaps, a tenth of the frames
            exactly UPPER or LOWER ('voiced': 0.9 everywhere, 'unvoiced': 0.05 everywhere)
      n     a walk quantised to steps of 0.05, so that windows hold repeated values and the frame tie-break decides
      f0    distinct in every frame, so that the frame a median chose can be read off the output
      loud  a walk around SILENCE
    nans: one NaN in each input of each row (T >= 4)."""
    rng = np.random.default_rng(seed)
    p = np.clip(0.25 + np.cumsum(rng.normal(0, 0.07, (B, T)), axis=1), 0, 1).astype(np.float32)
    exact = rng.random((B, T))
    p[exact < 0.05] = UPPER
    p[exact > 0.95] = LOWER
    if kind == "voiced":
        p[:] = 0.9
    elif kind == "unvoiced":
        p[:] = 0.05
    n = np.clip(0.5 + np.cumsum(rng.normal(0, 0.03, (B, T)), axis=1), 0, 1)
    n = (np.round(n * 20) / 20).astype(np.float32)
    f0 = (100.0 + 0.25 * np.arange(T)[None, :] + 1000.0 * np.arange(B)[:, None] + 0.125 * rng.random((B, T))).astype(np.float32)
    loud = (SILENCE + np.cumsum(rng.normal(0, 0.05, (B, T)), axis=1)).astype(np.float32)
    if nans and T >= 4:
        for r in range(B):
            for x in (f0, n, p, loud):
                x[r, rng.integers(0, T)] = np.nan
    return dict(f0=f0, n=n, p=p, loud=loud)


def make_state(seed, B):
    """[B, 3]: flags of both kinds, and a NaN last_n (no virtual frame) in every third row"""
    rng = np.random.default_rng(seed)
    state = np.stack([rng.integers(0, 2, B).astype(np.float32), (np.round(rng.random(B) * 20) / 20).astype(np.float32),
                      (50.0 + rng.random(B)).astype(np.float32)], axis=1)
    state[2::3, 1] = np.nan
    return state
