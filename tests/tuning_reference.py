"""The definitions of `tuning_statistics` and `tune_pitch` (include/ddsp_hip.h: ddsp_tuning_*) as
plain loops over Python ints and floats, independent of the package, and the seeded inputs their tests share.

Every position is a Python int counting 2^-16 cent on the MIDI scale (note m at m S, S = 100 * 65536; A4 = 69).  A frame's
position carries one fp64 rounding; everything after it -- cells, costs, notes, sums, means, the glide -- is integer
arithmetic, so no result depends on the order its frames were visited in."""
import math

import numpy as np

F32 = np.float32
S = 100 * 65536                             # one semitone
OCTAVE = 12 * S
K = 2346.0614660728625                      # 1997.3794084376191 - 1200 log2(44) + 6900: cents of normalized_cents = 0 above MIDI note 0
CENTS_SPAN = 7180.0
LIMIT = 4.0                                 # |normalized_cents| beyond it is not on: |position| stays below 2^31
OFF = -(1 << 31)                            # notes_out of an off frame
SCALES = dict(chromatic=0xFFF, major=0xAB5, minor=0x5AD, pentatonic=0x295)


def position(n):
    """n: an fp32 value -> int.  The product is exact in fp64 (13 bits times 24), the sum rounds once, the scale is exact."""
    return round((CENTS_SPAN * float(n) + K) * 65536.0)           # round(): ties to even, as llrint


def is_on(n, h=None, l=None, v=None, silence=None, confidence=0.0):
    if not abs(float(n)) <= LIMIT:                                # a NaN compares false
        return False
    if v is not None and not bool(v):
        return False
    if h is not None and not F32(h) >= F32(confidence):
        return False
    if l is not None and silence is not None and not F32(l) > F32(silence):
        return False
    return True


def on_mask(cents, harm=None, loud=None, voiced=None, silence=None, confidence=0.0):
    """[R, T] arrays -> list of lists of bool"""
    R, T = cents.shape
    return [[is_on(cents[r, t], None if harm is None else harm[r, t], None if loud is None else loud[r, t],
                   None if voiced is None else voiced[r, t], silence, confidence) for t in range(T)] for r in range(R)]


def histogram(cents, on):
    """one group: a flat list of fp32 values and of bools -> H[1200]"""
    H = [0] * 1200
    for n, o in zip(cents, on):
        if o:
            H[((position(n) + 32768) % OCTAVE) // 65536] += 1
    return H


def rdiv(a, b):
    return (2 * a + b) // (2 * b)


def estimate(H, mask, root=None):
    """H[1200] -> dict(offset, root, profile [12], frames)"""
    N = sum(H)
    if N == 0:
        return dict(offset=0, root=0 if root is None else root, profile=[0] * 12, frames=0)
    D = [sum(H[100 * p + d] for p in range(12)) for d in range(100)]
    best = None
    for o in range(-50, 50):
        cost = sum(D[d] * min((d - o) % 100, (o - d) % 100) for d in range(100))
        key = (cost, abs(o), 0 if o >= 0 else 1)
        if best is None or key < best[0]:
            best = (key, o)
    o = best[1]
    P = [sum(H[(100 * p + o + j) % 1200] for j in range(-50, 50)) for p in range(12)]
    if root is None:
        scores = [sum(P[p] * ((mask >> ((p - r) % 12)) & 1) for p in range(12)) for r in range(12)]
        root = max(range(12), key=lambda r: (scores[r], -r))
    return dict(offset=o, root=root, profile=P, frames=N)


def statistics(cents, on, per_row=False, mask=SCALES["major"], root=None):
    """cents [R, T] fp32, on: on_mask(...) -> dict of numpy arrays: histogram [G, 1200], offset, root [G], profile [G, 12], frames"""
    R, T = cents.shape
    groups = [[r] for r in range(R)] if per_row else [list(range(R))]
    hs, es = [], []
    for g in groups:
        hs.append(histogram([cents[r, t] for r in g for t in range(T)], [on[r][t] for r in g for t in range(T)]))
        es.append(estimate(hs[-1], mask, root))
    return dict(histogram=np.array(hs, dtype=np.int64), offset=np.array([e["offset"] for e in es], dtype=np.int32),
                root=np.array([e["root"] for e in es], dtype=np.int32), profile=np.array([e["profile"] for e in es], dtype=np.int64),
                frames=np.array([e["frames"] for e in es], dtype=np.int64))


def allowed(m, root, mask):
    return (mask >> ((m - root) % 12)) & 1


def nearest(v, root, mask):
    """the allowed note nearest to v, ties to the lower one"""
    lo = v // S
    while not allowed(lo, root, mask):
        lo -= 1
    hi = v // S + 1
    while not allowed(hi, root, mask):
        hi += 1
    return lo if v - lo * S <= hi * S - v else hi


def snap_row(n, f0, on, o, root, mask, h=0, min_note_frames=0, glide=0, vibrato=True, concert=False, amount=1.0):
    """One row.  n, f0: fp32 arrays [T]; on: bools; h: hysteresis in units; amount: an fp32 value.
    -> dict(notes [T] int32, correction [T] int32, cents [T] fp32, f0 [T] fp32, v: the positions (None where off))"""
    T = len(n)
    v = [position(n[t]) - 65536 * o if on[t] else None for t in range(T)]
    note = [None] * T
    for t in range(T):
        if not on[t]:
            continue
        q = nearest(v[t], root, mask)
        if t > 0 and on[t - 1] and abs(v[t] - note[t - 1] * S) <= abs(v[t] - q * S) + h:
            note[t] = note[t - 1]
        else:
            note[t] = q
    corr = [0] * T
    t = 0
    while t < T:
        if not on[t]:
            t += 1
            continue
        e = t
        while e + 1 < T and on[e + 1] and note[e + 1] == note[t]:
            e += 1
        L = e - t + 1
        if L >= min_note_frames:
            shift = 65536 * o if concert else 0
            if vibrato:
                c = rdiv(note[t] * S * L - sum(v[t:e + 1]), L) - shift
                for u in range(t, e + 1):
                    corr[u] = c
            else:
                for u in range(t, e + 1):
                    corr[u] = note[t] * S - v[u] - shift
        t = e + 1
    a = min(max(float(F32(amount)), 0.0), 1.0) if amount == amount else 0.0     # (a per-row amount is clamped; a NaN is 0)
    d = [0] * T
    for t in range(T):
        if not on[t]:
            continue
        first, last = t, t
        while first > 0 and on[first - 1]:
            first -= 1
        while last + 1 < T and on[last + 1]:
            last += 1
        lo, hi = max(t - glide, first), min(t + glide, last)
        smoothed = rdiv(sum(corr[lo:hi + 1]), hi - lo + 1)
        d[t] = round(a * float(smoothed))
    cents, f0_out = np.array(n, dtype=F32), np.array(f0, dtype=F32)
    for t in range(T):
        if d[t]:
            cents[t] = F32(n[t]) + F32(d[t] / (65536.0 * CENTS_SPAN))
            f0_out[t] = F32(float(f0[t]) * 2.0 ** (d[t] / (65536.0 * 1200.0)))
    notes = np.array([OFF if x is None else x for x in note], dtype=np.int64).astype(np.int32)
    return dict(notes=notes, correction=np.array(d, dtype=np.int64).astype(np.int32), cents=cents, f0=f0_out, v=v)


def tune(cents, f0, on, offset, root, mask, amount=1.0, **options):
    """[B, T] -> dict of [B, T] arrays; offset, root: one value or one per row; amount likewise"""
    B = cents.shape[0]
    per = lambda x, b: x[b if len(x) > 1 else 0] if hasattr(x, "__len__") else x        # noqa: E731
    rows = [snap_row(cents[b], f0[b], on[b], int(per(offset, b)), int(per(root, b)), mask, amount=per(amount, b), **options)
            for b in range(B)]
    return {k: np.stack([r[k] for r in rows]) for k in ("notes", "correction", "cents", "f0")}


def cents_of_f0(f0):
    """normalized_cents of a frequency in Hz, formed in fp64 and rounded once"""
    return F32((1200.0 * math.log2(float(f0) / 10.0) - 1997.3794084376191) / CENTS_SPAN)


def f0_of_cents(n):
    return (10.0 * np.exp2((CENTS_SPAN * np.asarray(n, dtype=np.float64) + 1997.3794084376191) / 1200.0)).astype(F32)


def make(seed, R, T, special=False, low=False):
    """Seeded inputs [R, T]: cents (a random walk over notes with vibrato), f0 to match, harm, loud fp32 and voiced bool.
    special: NaN, +-inf, values beyond the limit and at it in every input, a row without an on frame (when R > 1),
    a row that alternates on and off (R > 2).  low: positions below MIDI note 0 (a negative position: the floor-mod)."""
    rng = np.random.default_rng(seed)
    midi = 57.0 + np.cumsum((rng.random((R, T)) < 0.12) * rng.integers(-4, 5, (R, T)), axis=1)
    midi = midi + 0.3 * np.sin(0.9 * np.arange(T))[None] * rng.random((R, 1)) + 0.45 * (rng.random((R, 1)) - 0.5) \
        + 0.08 * rng.standard_normal((R, T))
    if low:
        midi = midi - 60.0
    cents = ((midi * 100.0 - K) / CENTS_SPAN).astype(F32)
    harm = rng.random((R, T)).astype(F32)
    loud = (rng.random((R, T)) * 5.0 - 4.0).astype(F32)
    voiced = rng.random((R, T)) < 0.85
    f0 = f0_of_cents(cents)
    if special:
        bad = [np.nan, np.inf, -np.inf, 4.5, -1e30, 4.0, -4.0, 4.0000005]
        for x in (cents, harm, loud, f0):
            for k, value in enumerate(bad):
                at = rng.integers(0, R * T)
                x.reshape(-1)[at] = value
        if R > 1:
            voiced[1] = False
        if R > 2:
            voiced[2] = np.arange(T) % 2 == 0
            harm[2], loud[2] = 0.9, 0.0
    return dict(cents=cents, f0=f0, harm=harm, loud=loud, voiced=voiced)


def melody(seed=5, frames=860, detune=37.0, key=2, vibrato=20.0, noise=5.0):
    """A D-major melody: notes 8..40 frames long, `detune` cents sharp, with +-`vibrato` cents of vibrato and `noise` cents
    (standard deviation) of jitter -> (cents [1, frames] fp32, the notes played [frames])."""
    rng = np.random.default_rng(seed)
    degrees = [0, 2, 4, 5, 7, 9, 11]
    played, at = [], 3
    while len(played) < frames:
        at = int(np.clip(at + rng.integers(-2, 3), 0, 13))
        note = 60 + key + 12 * (at // 7) + degrees[at % 7]
        played += [note] * int(rng.integers(8, 41))
    played = np.array(played[:frames])
    t = np.arange(frames)
    c = played * 100.0 + detune + vibrato * np.sin(2 * np.pi * t / 9.0) + noise * rng.standard_normal(frames)
    return ((c - K) / CENTS_SPAN).astype(F32)[None], played
