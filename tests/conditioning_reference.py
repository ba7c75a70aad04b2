"""The definitions of `conditioning_statistics` and `fit_conditioning` (include/ddsp_hip.h:
ddsp_condition_*) as plain loops, independent of the package, and the seeded inputs their tests share.

Everything a statistic accumulates is an integer (cell counts, and fixed-point sums of llrintf(value * 2^24)), so a result
does not depend on the order its frames were visited in; a table entry is one fp64 expression of exact integers rounded to
fp32 once; the map is fp32 arithmetic with every rounding written out (no fused multiply-add, a correctly rounded
division)."""
import bisect

import numpy as np

F32 = np.float32
FIXED = 1 << 24                     # the fixed-point scale of the two sums
VALUE_LIMIT = F32(1 << 15)          # a frame at or beyond this magnitude is not counted: |value| 2^24 frames stays below 2^63
MAX_GROUP_FRAMES = 1 << 24          # with at most this many frames in one statistic
CENTS_SPAN = 7180.0                 # normalized_cents = (cents - cents of bin 0) / 7180
OCTAVE = 1200.0


def is_on(l, n, h, v, silence, confidence):
    """A note-on frame.  l, n, h: np.float32; v: bool or None"""
    if not (np.isfinite(l) and np.isfinite(n)) or abs(l) >= VALUE_LIMIT or abs(n) >= VALUE_LIMIT:
        return False
    if silence is not None and not l > F32(silence):
        return False
    if not h >= F32(confidence):                    # a NaN harmonicity compares false
        return False
    return v is None or bool(v)


def cell_of(l, lo, hi, bins):
    """floorf((l - lo) * scale) clamped to [0, bins - 1], scale = fl32(bins) / (fl32(hi) - fl32(lo)), every step fp32"""
    lo, hi = F32(lo), F32(hi)
    with np.errstate(all="ignore"):
        scale = F32(bins) / F32(hi - lo)
        u = F32(F32(l - lo) * scale)
    if u < 0:
        return 0
    if u >= bins:
        return bins - 1
    return int(np.floor(u))


def histogram(loud, cents, harm, voiced=None, silence=None, confidence=0.0, lo=-4.0, hi=2.0, bins=4096):
    """One group: the frames of fp32 arrays of any (equal) shape -> (counts [bins] python ints, sum_cents, sum_loudness)."""
    counts, sum_n, sum_l = [0] * bins, 0, 0
    L, N, H = (np.asarray(x, dtype=F32).reshape(-1) for x in (loud, cents, harm))
    V = None if voiced is None else np.asarray(voiced).reshape(-1)
    for i in range(len(L)):
        if not is_on(L[i], N[i], H[i], None if V is None else V[i], silence, confidence):
            continue
        counts[cell_of(L[i], lo, hi, bins)] += 1
        sum_n += int(np.rint(F32(N[i] * F32(FIXED))))           # the product is exact: a power of two
        sum_l += int(np.rint(F32(L[i] * F32(FIXED))))
    return counts, sum_n, sum_l


def quantile_table(counts, Q, lo=-4.0, hi=2.0):
    """S[0 .. Q] fp32 from one group's counts (python ints)."""
    bins = len(counts)
    lo, hi = float(F32(lo)), float(F32(hi))
    width = (hi - lo) / bins
    cum, total = [], 0
    for c in counts:
        total += c
        cum.append(total)
    N = total
    S = np.full(Q + 1, np.nan, dtype=F32)
    if N == 0:
        return S
    b = 0
    for k in range(Q + 1):
        while not (counts[b] > 0 and Q * cum[b] >= k * N):      # the smallest such cell; it does not fall as k grows
            b += 1
        f =float(k * N - Q * (cum[b] - counts[b])) / float(Q * counts[b])
        f = min(max(f, 0.0), 1.0)
        S[k] = F32(lo + (b + f) * width)
    return S


def mean_of(total, N):
    return float(total) / (float(N) * float(FIXED)) if N else float("nan")


def statistics(loud, cents, harm, voiced=None, per_row=False, Q=64, **kw):
    """[R, T] arrays -> dict(counts [G, bins] uint32, sums [G, 2] int64 = (cents, loudness), tables [G, Q + 1] fp32,
    mean_pitch, mean_loudness [G] fp64, frames [G] int64); G = R per row, else 1."""
    loud = np.asarray(loud, dtype=F32)
    R = loud.shape[0]
    groups = [slice(r, r + 1) for r in range(R)] if per_row else [slice(0, R)]
    out = dict(counts=[], sums=[], tables=[], mean_pitch=[], mean_loudness=[], frames=[])
    for g in groups:
        counts, sn, sl = histogram(loud[g], np.asarray(cents)[g], np.asarray(harm)[g],
                                   None if voiced is None else np.asarray(voiced)[g], **kw)
        N = sum(counts)
        out["counts"].append(np.array(counts, dtype=np.uint32))
        out["sums"].append(np.array([sn, sl], dtype=np.int64))
        out["tables"].append(quantile_table(counts, Q, kw.get("lo", -4.0), kw.get("hi", 2.0)))
        out["mean_pitch"].append(mean_of(sn, N))
        out["mean_loudness"].append(mean_of(sl, N))
        out["frames"].append(N)
    return dict(counts=np.stack(out["counts"]), sums=np.stack(out["sums"]), tables=np.stack(out["tables"]),
                mean_pitch=np.array(out["mean_pitch"], dtype=np.float64),
                mean_loudness=np.array(out["mean_loudness"], dtype=np.float64), frames=np.array(out["frames"], dtype=np.int64))


def map_loudness(l, S, T, strength=1.0):
    """One frame through the source table S and the target table T (fp32 arrays [Q + 1], non-decreasing, no NaN)."""
    l, Q, strength = F32(l), len(S) - 1, F32(strength)
    if not np.isfinite(l):
        return l
    with np.errstate(all="ignore"):
        if l < S[0]:
            mapped = F32(l + F32(T[0] - S[0]))
        elif l >= S[Q]:
            mapped = F32(l + F32(T[Q] - S[Q]))
        else:
            k = min(bisect.bisect_right([float(s) for s in S], float(l)) - 1, Q - 1)     # the largest k with S[k] <= l
            d = F32(S[k + 1] - S[k])
            w = F32(F32(l - S[k]) / d) if d > 0 else F32(0.5)
            mapped = F32(T[k] + F32(w * F32(T[k + 1] - T[k])))
        return F32(l + F32(strength * F32(mapped - l)))


def octave_shift(target_mean, source_mean, octaves=True, max_octaves=2):
    """k of one row: octaves False -> 0, an int -> itself, True -> the rounded distance of the means, clamped"""
    if octaves is False:
        return 0
    if octaves is not True:
        return int(octaves)
    with np.errstate(all="ignore"):
        x = np.rint((np.float64(target_mean) - np.float64(source_mean)) * CENTS_SPAN / OCTAVE)   # ties to even
    if not np.isfinite(x):
        return 0
    return int(min(max(x, -max_octaves), max_octaves))


def fit(f0, cents, loud, source, target, octaves=True, max_octaves=2, strength=1.0, min_frames=8):
    """[B, T] fp32 arrays; source, target: dicts as `statistics` returns (G = 1 or B; only tables, mean_pitch and frames
    are read) -> dict(f0, cents, loud [B, T] fp32, octaves [B] int32, frames [B] int64)."""
    f0, cents, loud = (np.asarray(x, dtype=F32) for x in (f0, cents, loud))
    B, T = loud.shape
    out = dict(f0=f0.copy(), cents=cents.copy(), loud=loud.copy(), octaves=np.zeros(B, dtype=np.int32),
               frames=np.zeros(B, dtype=np.int64))
    strength = np.broadcast_to(np.asarray(strength, dtype=F32), (B,))
    for r in range(B):
        gs, gt = (r if len(source["tables"]) > 1 else 0), (r if len(target["tables"]) > 1 else 0)
        S, Tt = source["tables"][gs], target["tables"][gt]
        out["frames"][r] = source["frames"][gs]
        if source["frames"][gs] < min_frames or np.isnan(S).any() or np.isnan(Tt).any():
            continue                                            # too little to go on: the row as it came
        k = octave_shift(target["mean_pitch"][gt], source["mean_pitch"][gs], octaves, max_octaves)
        out["octaves"][r] = k
        step = F32(k * OCTAVE / CENTS_SPAN)
        for t in range(T):
            with np.errstate(all="ignore"):
                out["f0"][r, t] = np.ldexp(f0[r, t], k)
                out["cents"][r, t] = F32(cents[r, t] + step)
            out["loud"][r, t] = map_loudness(loud[r, t], S, Tt, strength[r])
    return out


def make(seed, R, T, special=False, voiced=False):
    """Seeded inputs dict(f0, cents, loud, harm[, voiced]) of fp32 [R, T].
      loud   a walk inside [-4, 2) quantised to steps of 1/64, so that cells repeat and cell edges are hit exactly
      cents  a walk in [0, 1];  harm in [0, 1];  f0 distinct in every frame
    special: row 0 (with R >= 2: otherwise nothing) has no on frame; values below lo, exactly hi, above hi, huge, NaN and
    +-inf are planted in every input (T >= 5)."""
    rng = np.random.default_rng(seed)
    loud = np.clip(-1.5 + np.cumsum(rng.normal(0, 0.2, (R, T)), axis=1), -3.9, 1.9)
    loud = (np.round(loud * 64) / 64).astype(F32)
    cents = np.clip(0.5 + np.cumsum(rng.normal(0, 0.02, (R, T)), axis=1), 0, 1).astype(F32)
    harm = rng.random((R, T)).astype(F32)
    f0 = (100.0 + 0.25 * np.arange(T)[None, :] + 1000.0 * np.arange(R)[:, None] + 0.125 * rng.random((R, T))).astype(F32)
    x = dict(f0=f0, cents=cents, loud=loud, harm=harm)
    if voiced:
        x["voiced"] = rng.random((R, T)) < 0.7
    if special:
        if T >= 5:
            for r in range(R):
                at = rng.permutation(T)
                loud[r, at[0]], loud[r, at[1]], loud[r, at[2]] = -4.5, 2.0, 7.25
                loud[r, at[3]] = (np.nan, np.inf, -np.inf, 1e30)[r % 4]
                cents[r, at[4]] = (np.inf, np.nan, 1e30, -np.inf)[r % 4]
                harm[r, at[(5 + r) % T]] = (np.nan, np.inf, -np.inf)[r % 3]
                f0[r, at[(6 + r) % T]] = (np.nan, np.inf)[r % 2]
        if R >= 2:
            harm[0] = -1.0                                      # below any confidence >= 0: no on frame in row 0
    return x
