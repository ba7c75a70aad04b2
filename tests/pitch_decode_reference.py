"""fp64 numpy oracle of the pitch decoders, written as plain loops and independent of the package:
`centered` (the nine-bin weighted average, every probability with its own bin's cents), a Viterbi dynamic programme under
the triangular +-11-bin transition, `path_score`, a brute-force enumeration of every banded path for T <= 3, and the
seeded input makers the decoder tests share."""
import numpy as np

BINS = 360
BAND = 11
HALF = 4
CENTS_0 = 1997.3794084376191
FLOOR = float(np.float32(1e-30))


def cents_map(b):
    return 20.0 * np.asarray(b, dtype=np.float64) + CENTS_0


def log_transition():
    """[360, 23] by target bin j and k - j + 11: log(max(12 - |k - j|, 0) / S_k), fp64, rounded once to fp32 (the table the
    kernel is given), returned as float64; -inf where k is outside 0 .. 359."""
    table = np.full((BINS, 2 * BAND + 1), -np.inf)
    for k in range(BINS):
        row = [max(BAND + 1 - abs(k - j), 0) for j in range(BINS)]
        total = float(sum(row))
        for j in range(max(0, k - BAND), min(BINS, k + BAND + 1)):
            table[j, k - j + BAND] = np.log(row[j] / total)
    return table.astype(np.float32).astype(np.float64)


def centered(center, p):
    """center [...] integer bins, p [..., 360] -> dict of cents, f0, harmonicity, normalized_cents ([...], fp64)."""
    p = np.asarray(p, dtype=np.float64)
    center = np.asarray(center, dtype=np.int64)
    num = np.zeros(center.shape)
    den = np.zeros(center.shape)
    for i in range(-HALF, HALF + 1):
        k = center + i
        ok = (k >= 0) & (k < BINS)
        w = np.where(ok, np.take_along_axis(p, np.clip(k, 0, BINS - 1)[..., None], axis=-1)[..., 0], 0.0)
        num = num + i * w
        den = den + w
    with np.errstate(invalid="ignore", divide="ignore"):
        cents = cents_map(center) + 20.0 * num / den
    return dict(cents=cents, f0=10.0 * 2.0 ** (cents / 1200.0),
                harmonicity=np.take_along_axis(p, center[..., None], axis=-1)[..., 0],
                normalized_cents=(cents - cents_map(0)) / (cents_map(BINS - 1) - cents_map(0)))


def emissions(p):
    return np.log(np.fmax(np.asarray(p, dtype=np.float64), FLOOR))          # fmax drops a NaN


def _advance(v, log_a):
    """scores [360] of one frame -> (best predecessor score, best predecessor) per target bin; ties to the lower predecessor"""
    padded = np.full(BINS + 2 * BAND, -np.inf)
    padded[BAND:BAND + BINS] = v
    best = padded[0:BINS] + log_a[:, 0]
    arg = np.zeros(BINS, dtype=np.int64)
    for d in range(1, 2 * BAND + 1):
        cand = padded[d:d + BINS] + log_a[:, d]
        take = cand > best
        best = np.where(take, cand, best)
        arg = np.where(take, d, arg)
    return best, arg - BAND + np.arange(BINS)


def viterbi(p, state=None, log_a=None):
    """p [T, 360] -> (path int64 [T], last frame's scores [360]); ties to the lower predecessor and the lower final state."""
    log_a = log_transition() if log_a is None else log_a
    e = emissions(p)
    T = e.shape[0]
    back = np.zeros((T, BINS), dtype=np.int64)
    v = e[0] if state is None else _advance(np.asarray(state, dtype=np.float64), log_a)[0] + e[0]
    for t in range(1, T):
        best, back[t] = _advance(v, log_a)
        v = best + e[t]
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = int(np.argmax(v))
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path, v


def path_score(path, p, log_a=None):
    """sum_t e_t[s_t] + sum_{t >= 1} log A[s_{t-1}][s_t] in fp64, summed in frame order; -inf for a step beyond the band."""
    log_a = log_transition() if log_a is None else log_a
    e = emissions(p)
    score = e[0, path[0]]
    for t in range(1, len(path)):
        d = int(path[t - 1]) - int(path[t]) + BAND
        if d < 0 or d > 2 * BAND:
            return -np.inf
        score = (score + log_a[path[t], d]) + e[t, path[t]]
    return score


def brute_force(p, log_a=None):
    """Every banded path of T <= 3 frames (360 * 23 * 23 at T = 3) -> (best path, its score).  The flattened order is (final
    state, its predecessor's offset, that one's predecessor's offset), so the first maximum obeys the tie rule."""
    log_a = log_transition() if log_a is None else log_a
    e = emissions(p)
    T = e.shape[0]
    assert 1 <= T <= 3
    best_score, best_path = -np.inf, None
    offsets = range(2 * BAND + 1)
    for s_last in range(BINS):
        if T == 1:
            cands = [((s_last,), e[0, s_last])]
        else:
            cands = []
            for d1 in offsets:
                k1 = s_last + d1 - BAND
                if k1 < 0 or k1 >= BINS:
                    continue
                if T == 2:
                    cands.append(((k1, s_last), (e[0, k1] + log_a[s_last, d1]) + e[1, s_last]))
                    continue
                d0 = np.arange(2 * BAND + 1)
                k0 = k1 + d0 - BAND
                ok = (k0 >= 0) & (k0 < BINS)
                first = np.where(ok, e[0, np.clip(k0, 0, BINS - 1)] + log_a[k1, d0], -np.inf)
                total = ((first + e[1, k1]) + log_a[s_last, d1]) + e[2, s_last]
                i = int(np.argmax(total))
                cands.append(((int(k0[i]), k1, s_last), total[i]))
        for path, score in cands:
            if score > best_score:
                best_score, best_path = score, path
    return np.array(best_path, dtype=np.int64), best_score


# ------------------------------------------------------------------------------------------------------------------ inputs

def rand(seed, T):
    """uniform probabilities [T, 360] fp32"""
    return np.random.default_rng(seed).random((T, BINS), dtype=np.float32)


def track(seed, T):
    """A wandering peak: width 1.5 bins at 180 + 60 sin(t / 9) plus unit jitter, over a uniform floor below 0.02; 10 % of the
    frames have the peak displaced by +120 bins (kept inside the range).  -> (p [T, 360] fp32, centre [T], displaced [T] bool)"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    centre = 180.0 + 60.0 * np.sin(t / 9.0) + rng.standard_normal(T)
    displaced = rng.random(T) < 0.10
    peak = np.where(displaced, np.minimum(centre + 120.0, BINS - 3.0), centre)
    b = np.arange(BINS)[None, :]
    p = 0.9 * np.exp(-0.5 * ((b - peak[:, None]) / 1.5) ** 2) + 0.02 * rng.random((T, BINS))
    return p.astype(np.float32), centre, displaced


def make(kind, seed, T):
    return rand(seed, T) if kind == "rand" else track(seed, T)[0]
