"""The definition of the time alignment in numpy, one row at a time: the features of a control dict, the
dynamic time warping of two feature sequences and the resampling of its path onto an output timeline in fp64, the same warping
in the kernel's own arithmetic (`dtw_fp32`: numpy float32, every operation rounded on its own, the kernel's summation order), and
the inputs of the tests.

  d(i, j)   sum_k (x_a[i, k] - x_b[j, k])^2, ascending k, one accumulator from 0; a value that is not < +inf (NaN) counts as +inf
  band      p = T_a - 1, q = T_b - 1: d(i, j) = +inf where |i q - j p| > radius max(p, q) (integers); radius None: no band
  D(0, 0)   d(0, 0);  D(i, j) = d(i, j) + best, best the first of D(i - 1, j - 1), D(i - 1, j) + penalty, D(i, j - 1) + penalty
            (those that exist, in this order) that no later one is strictly below: the cell's back-pointer
  path      the back-pointers from (T_a - 1, T_b - 1) to (0, 0), in forward order; cost = D(T_a - 1, T_b - 1)
  timeline  tau clamped to [0, 1], s_k = (1 - tau) i_k + tau j_k, S = s of the end cell; output frame t' of T' targets
            s = min(t' S / (T' - 1), S) (0 for T' = 1); k the largest index with s_k <= s; the end cell where k is the last point,
            else (i_k, j_k) + lam (i_k+1 - i_k, j_k+1 - j_k), lam = (s - s_k) / (s_k+1 - s_k); rounded once to fp32
  features  l(x) = (log2(max(x, 2^-L)) + L) / L.  With Delta = (sr // 2) / n_bands: the played amplitudes sampled at m Delta Hz,
            m = 1 .. n_bands, which is control_transform_reference.transform at pos = t, r = fl32(Delta / f0), q = 1, H' = n_bands
            (A'); l(A' / max over the row of A') / sqrt(n_bands); the noise bands pooled by mean over [(g F) // G, ((g + 1) F) // G)
            (an empty group is 0), l(pooled / max over the row) / sqrt(G); l(a / max over the voiced frames of a) on voiced
            frames, 0 elsewhere; 1 on voiced frames, 0 elsewhere.  A maximum of 0 divides by 1.

TOL_P bounds how much the fp32 path, scored in fp64, may cost more than the fp64 optimum, relative to that optimum + 1; TOL_F
bounds |features - fp64 features|.  tests/test_control_align_host.py derives both: the emulation's figure on the tests' own
inputs, doubled and rounded up, and fails if the figure outgrows the bound or the bound 1.5 times the doubled figure."""

import numpy as np

import control_transform_reference as tref

SAMPLE_RATE = tref.SAMPLE_RATE
TOL_P = 1e-12
TOL_F = 1.5e-7
KERNEL_MAX_FRAMES, KERNEL_MAX_FEATURES = 2048, 64
BAND_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 40), (40, 5), (64, 65), (7, 7)]
WARP_SHAPES = [(1, 1), (5, 3), (65, 64), (130, 7)]             # (T_a, D)
# (B, T_a, T_b, D, radius, penalty)
GPU_CASES = [(1, 1, 1, 1, None, 0.0), (2, 1, 9, 3, None, 0.0), (2, 9, 1, 3, None, 0.01), (3, 5, 40, 2, 1, 0.0), (2, 64, 65, 64, None, 0.0),
             (2, 65, 64, 1, None, 0.01), (2, 130, 3, 7, None, 0.0)] + \
            [(1, 129, 200, 42, radius, penalty) for radius in (None, 1, 8) for penalty in (0.0, 0.01)]
TIMINGS = (0.0, 0.5, 1.0)


def local_costs(xa, xb, dtype=np.float64):
    """d [T_a, T_b] in `dtype`."""
    xa, xb = np.asarray(xa, dtype), np.asarray(xb, dtype)
    acc = np.zeros((xa.shape[0], xb.shape[0]), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(xa.shape[1]):
            t = xa[:, None, k] - xb[None, :, k]
            acc = acc + t * t
        return np.where(acc < np.inf, acc, dtype(np.inf))


def allowed(T_a, T_b, radius):
    """[T_a, T_b]: the cells inside the band (integer arithmetic)."""
    if radius is None:
        return np.ones((T_a, T_b), bool)
    p, q = T_a - 1, T_b - 1
    i, j = np.arange(T_a, dtype=np.int64)[:, None], np.arange(T_b, dtype=np.int64)[None, :]
    return np.abs(i * q - j * p) <= int(radius) * max(p, q)


def dtw(xa, xb, radius=None, penalty=0.0, dtype=np.float64):
    """The recurrence and the walk back in `dtype` -> path int [L, 2], cost (a Python float holding a `dtype` value)."""
    T_a, T_b = len(xa), len(xb)
    d = np.where(allowed(T_a, T_b, radius), local_costs(xa, xb, dtype), dtype(np.inf)).astype(np.float64).tolist()
    if dtype is np.float64:
        rnd = float
    else:
        def rnd(v):                                             # a sum of two fp32 values formed in fp64 rounds as the fp32 sum does
            with np.errstate(over="ignore"):
                return float(np.float32(v))
    pen = float(dtype(penalty))
    D = [[0.0] * T_b for _ in range(T_a)]
    back = [[0] * T_b for _ in range(T_a)]
    for i in range(T_a):
        for j in range(T_b):
            if i == 0 and j == 0:
                D[0][0] = d[0][0]
                continue
            if i == 0:
                best, code = rnd(D[0][j - 1] + pen), 2
            elif j == 0:
                best, code = rnd(D[i - 1][0] + pen), 1
            else:
                best, code = D[i - 1][j - 1], 0
                up, left = rnd(D[i - 1][j] + pen), rnd(D[i][j - 1] + pen)
                if up < best:
                    best, code = up, 1
                if left < best:
                    best, code = left, 2
            D[i][j] = rnd(d[i][j] + best)
            back[i][j] = code
    i, j = T_a - 1, T_b - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        code = back[i][j]
        i, j = i - (code != 2), j - (code != 1)
        path.append((i, j))
    return np.array(path[::-1], dtype=np.int64), D[T_a - 1][T_b - 1]


def dtw_fp32(xa, xb, radius=None, penalty=0.0):
    """The kernel's arithmetic, operation by operation."""
    return dtw(xa, xb, radius, penalty, np.float32)


def path_cost(path, xa, xb, radius=None, penalty=0.0):
    """Any monotone path scored in fp64 by the definition: its local costs plus the penalty of every step that is not diagonal."""
    d = np.where(allowed(len(xa), len(xb), radius), local_costs(xa, xb), np.inf)
    steps = np.diff(path, axis=0)
    assert (path[0] == 0).all() and (path[-1] == (len(xa) - 1, len(xb) - 1)).all()
    assert ((steps >= 0) & (steps <= 1)).all() and (steps.sum(1) >= 1).all()
    return float(d[path[:, 0], path[:, 1]].sum() + float(penalty) * (steps.sum(1) == 1).sum())


def brute_force(xa, xb, radius=None, penalty=0.0):
    """The smallest path_cost over every monotone path (tiny shapes)."""
    T_a, T_b = len(xa), len(xb)
    best = np.inf

    def extend(path):
        nonlocal best
        i, j = path[-1]
        if (i, j) == (T_a - 1, T_b - 1):
            best = min(best, path_cost(np.array(path), xa, xb, radius, penalty))
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < T_a and j + dj < T_b:
                extend(path + [(i + di, j + dj)])
    extend([(0, 0)])
    return best


def default_frames(T_a, T_b, timing):
    tau = min(1.0, max(0.0, float(timing)))
    return max(1, int(np.floor((1.0 - tau) * T_a + tau * T_b + 0.5)))


def timeline(path, T_a, T_b, timing, frames=None):
    """-> positions_a, positions_b fp64 [T'] (the definition before its one rounding to fp32)."""
    tau = min(1.0, max(0.0, float(timing)))
    T_out = default_frames(T_a, T_b, tau) if frames is None else frames
    wa, wb = 1.0 - tau, tau
    pi, pj = path[:, 0].astype(np.float64), path[:, 1].astype(np.float64)
    s_k = wa * pi + wb * pj
    S = wa * float(T_a - 1) + wb * float(T_b - 1)
    out = np.zeros((2, T_out))
    for t in range(T_out):
        s = min(t * S / float(T_out - 1), S) if T_out > 1 else 0.0
        k = int(np.searchsorted(s_k, s, side="right")) - 1
        if k == len(path) - 1:
            out[:, t] = pi[k], pj[k]
        else:
            lam = (s - s_k[k]) / (s_k[k + 1] - s_k[k])
            out[:, t] = pi[k] + lam * (pi[k + 1] - pi[k]), pj[k] + lam * (pj[k + 1] - pj[k])
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------------------------ features

def level(x, L, dtype):
    with np.errstate(invalid="ignore"):
        return ((np.log2(np.maximum(x, dtype(2.0 ** -L))) + dtype(L)) / dtype(L)).astype(dtype)


def over_max(x):
    top = x.max()
    return x / (top if top > 0 else x.dtype.type(1))


def features(f0, a, c, N, sr, n_bands=32, noise_groups=8, range_log2=10.0, dtype=np.float64):
    """One row's features [T, D] in `dtype`: np.float64 is the definition, np.float32 the package's arithmetic with the transformation
    kernel's own (control_transform_reference.transform_fp32)."""
    f0 = np.asarray(f0, np.float32)
    T = len(f0)
    voiced = tref.voiced_of(f0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = tref.ratio_of(12.0 * np.log2(((sr // 2) / n_bands) / f0.astype(np.float64)))
    pos, q = np.arange(T, dtype=np.float32), np.ones(T, np.float32)
    if dtype is np.float64:
        A = tref.transform(f0, a, c, None, pos, r, q, sr, n_bands)["A"]
    else:
        res = tref.transform_fp32(f0, a, c, None, pos, r, q, sr, n_bands)
        A = res["a"][:, None] * res["c"]
    parts = [level(over_max(A), range_log2, dtype) / dtype(np.sqrt(n_bands))]
    if N is not None:
        N = np.asarray(N, dtype)
        F = N.shape[-1]
        edges = [(g * F) // noise_groups for g in range(noise_groups + 1)]
        pooled = np.stack([N[:, lo:hi].mean(-1) if hi > lo else np.zeros(T, dtype) for lo, hi in zip(edges, edges[1:])], -1).astype(dtype)
        parts.append(level(over_max(pooled), range_log2, dtype) / dtype(np.sqrt(noise_groups)))
    av = np.where(voiced, np.asarray(a, dtype), dtype(0))
    parts.append(np.where(voiced, level(over_max(av), range_log2, dtype), dtype(0))[:, None])
    parts.append(voiced.astype(dtype)[:, None])
    return np.concatenate(parts, -1).astype(dtype)


# ------------------------------------------------------------------------------------------------------------------ inputs

def random_warp(T_a, T_b, rng, among=None):
    """w [T_b]: non-decreasing from 0 to T_a - 1 and onto (T_b >= T_a); the frames that repeat are drawn from the first `among`."""
    assert T_b >= T_a
    w = np.sort(np.concatenate([np.arange(T_a), rng.integers(0, among or T_a, T_b - T_a)]))
    return w.astype(np.int64)


def sequences(B, T_a, T_b, D, seed=0):
    """x_a [B, T_a, D], x_b [B, T_b, D] fp32: smooth random curves; x_b follows x_a along a bent time axis, with noise, so that the
    best path is neither the diagonal nor trivial; every sixth frame of x_a and every fourth of x_b repeats the frame before it."""
    rng = np.random.default_rng(100 * seed + 7 * T_a + 11 * T_b + 13 * D + B)
    xa = np.cumsum(rng.normal(0.0, 0.3, (B, T_a, D)), 1)
    t = np.linspace(0.0, 1.0, T_b) ** rng.uniform(0.6, 1.6)
    at = np.clip(np.round(t * (T_a - 1)).astype(np.int64), 0, T_a - 1)
    xb = xa[:, at] + rng.normal(0.0, 0.05, (B, T_b, D))
    xa, xb = xa.astype(np.float32), xb.astype(np.float32)
    for x, every in ((xa, 6), (xb, 4)):                         # repeated frames: equal costs, which only the rounding tells apart
        for t in range(every - 1, x.shape[1], every):
            x[:, t] = x[:, t - 1]
    return xa, xb


def warped_copy(T_a, D, seed=0):
    """x_a [T_a, D] with distinct rows, x_b[j] = x_a[w(j)] -> (x_a, x_b, w): the cells (w(j), j) cost 0 and no other cell does."""
    rng = np.random.default_rng(1000 + 31 * T_a + D + seed)
    xa = rng.permutation(4 * T_a)[:T_a, None] + rng.uniform(0.0, 0.5, (T_a, D))       # the first feature alone tells the rows apart
    w = random_warp(T_a, T_a + (T_a + 1) // 2, rng)
    xa = xa.astype(np.float32)
    return xa, xa[w].copy(), w


def hostile(B, T_a, T_b, D, seed=0):
    """`sequences` with NaN, +-inf and 3e38 scattered in both inputs of every row but the first, and a last row of x_a that is all
    NaN."""
    rng = np.random.default_rng(77 + seed)
    xa, xb = sequences(B, T_a, T_b, D, seed)
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    for x in (xa, xb):                                          # (one such value makes its frame cost +inf against every frame)
        part = x[1:].reshape(-1)
        at = rng.integers(0, part.size, max(4, part.size // 40))
        part[at] = bad[rng.integers(0, len(bad), len(at))]
    xa[-1] = np.nan
    return xa, xb


SEGMENTS, SEGMENT_FRAMES, PHRASE_H, PHRASE_F, PHRASE_F0 = 6, 8, 40, 65, 200.0
PHRASE_CENTRES = (500.0, 1500.0, 900.0, None, 2500.0, 700.0)  # Hz at the segment's first frame; None: unvoiced


def phrase_formant(t):
    """The centre (Hz) of frame t's formant, None on the unvoiced segment."""
    centre = PHRASE_CENTRES[t // SEGMENT_FRAMES]
    return None if centre is None else centre + 60.0 * (t % SEGMENT_FRAMES)


def phrase(seed=0):
    """Six segments of eight frames at 16 kHz, 40 harmonics at 200 Hz: one Gaussian formant per segment that glides 60 Hz a frame,
    the fourth segment unvoiced under a noise band that moves -> (the controls f0 [T], a [T], c [T, H], N [T, F] fp32, and w [71], the
    frames of the phrase that a second, slower take of 71 frames plays)."""
    T = SEGMENTS * SEGMENT_FRAMES
    hz = PHRASE_F0 * np.arange(1, PHRASE_H + 1)
    f0, a = np.full(T, PHRASE_F0, np.float32), np.full(T, 0.5, np.float32)
    c, N = np.zeros((T, PHRASE_H)), np.full((T, PHRASE_F), 0.01)
    for t in range(T):
        centre = phrase_formant(t)
        if centre is None:
            f0[t], a[t] = 0.0, 0.0
            c[t] = 1.0 / PHRASE_H
            N[t] = 0.01 + np.exp(-0.5 * ((np.arange(PHRASE_F) - (12.0 + 5.0 * (t % SEGMENT_FRAMES))) / 4.0) ** 2)
        else:
            env = np.exp(-0.5 * ((hz - centre) / 200.0) ** 2) + 1e-3
            c[t] = env / env.sum()
    w = random_warp(T, 71, np.random.default_rng(5 + seed), among=2 * SEGMENT_FRAMES)       # it lingers on the first two segments
    return dict(f0=f0, a=a, c=c.astype(np.float32), N=N.astype(np.float32)), w


def phrase_deviation(path, w):
    """-> (path points whose i and w(j) lie in different segments, the largest |i - w(j)|)."""
    i, wj = path[:, 0], w[path[:, 1]]
    return int((i // SEGMENT_FRAMES != wj // SEGMENT_FRAMES).sum()), int(np.abs(i - wj).max())
