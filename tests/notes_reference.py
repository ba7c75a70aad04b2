"""The definitions of `extract_notes` and `render_notes` (include/ddsp_hip.h: ddsp_notes_*) as plain
loops over Python ints and floats, independent of the package.  Positions, the on test, the nearest allowed note and rdiv are
those of tests/tuning_reference.py: a position is a Python int counting 2^-16 cent on the MIDI scale."""
import math

import numpy as np

from tuning_reference import F32, K, OFF, S, is_on, nearest, position, rdiv  # noqa: F401

NO_PITCH = -(1 << 31)                       # the pitch of an unused slot
NAN = F32(np.nan)
HOLD = 6900 * 65536                         # the position held where no note gives one
MAX_DETUNE = 1 << 30


def level_max(a, b):
    """the larger of two fp32 levels: a NaN never wins, +0 beats -0"""
    if b != b:
        return a
    if a != a:
        return b
    if b > a or (b == a and np.signbit(a) and not np.signbit(b)):
        return b
    return a


def row_notes(n, on, o, root, mask, h):
    """§10e steps 1, 2 and 5 for one row -> (v, note): lists with None where off"""
    T = len(n)
    o = min(max(int(o), -50), 50)
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
    return v, note


def extract_row(n, on, o, root, mask, h=0, min_note_frames=0, loud=None):
    """One row -> the kept notes as a list of (onset, frames, pitch, detune, level), in order of onset."""
    T = len(n)
    v, note = row_notes(n, on, o, root % 12, mask, h)
    out, t = [], 0
    while t < T:
        if not on[t]:
            t += 1
            continue
        e = t
        while e + 1 < T and on[e + 1] and note[e + 1] == note[t]:
            e += 1
        L = e - t + 1
        if L >= min_note_frames:
            level = NAN
            if loud is not None:
                for u in range(t, e + 1):
                    level = level_max(level, F32(loud[u]))
            out.append((t, L, note[t], -rdiv(note[t] * S * L - sum(v[t:e + 1]), L), F32(level)))
        t = e + 1
    return out


def extract(cents, on, offset, root, mask, max_notes, h=0, min_note_frames=0, loud=None):
    """[B, T] -> dict of [B, N] arrays (onset, frames, pitch, detune int32; level fp32) and count [B] int32"""
    B, N = cents.shape[0], max_notes
    per = lambda x, b: int(x[b if len(x) > 1 else 0]) if hasattr(x, "__len__") else int(x)      # noqa: E731
    out = dict(onset=np.full((B, N), -1, np.int32), frames=np.zeros((B, N), np.int32), pitch=np.full((B, N), NO_PITCH, np.int32),
               detune=np.zeros((B, N), np.int32), level=np.full((B, N), NAN, np.float32), count=np.zeros(B, np.int32))
    for b in range(B):
        notes = extract_row(cents[b], on[b], per(offset, b), per(root, b), mask, h, min_note_frames, None if loud is None else loud[b])
        out["count"][b] = len(notes)
        for i, (s, L, p, d, lv) in enumerate(notes[:N]):
            out["onset"][b, i], out["frames"][b, i], out["pitch"][b, i], out["detune"][b, i], out["level"][b, i] = s, L, p, d, lv
    return out


def expand(rec, T):
    """records -> the per-frame note array [B, T] (OFF where no kept note), and the per-frame detune"""
    B = rec["onset"].shape[0]
    notes, detune = np.full((B, T), OFF, np.int64), np.zeros((B, T), np.int64)
    for b in range(B):
        for i in range(min(int(rec["count"][b]), rec["onset"].shape[1])):
            s, L = int(rec["onset"][b, i]), int(rec["frames"][b, i])
            notes[b, s:s + L], detune[b, s:s + L] = rec["pitch"][b, i], rec["detune"][b, i]
    return notes.astype(np.int32), detune


def render_row(onset, frames, pitch, detune, level, count, o, T, keep_detune=True, concert=False, transpose_units=0, glide=0,
               attack=0, release=0, floor=0.0, default_level=1.0, depth_units=0.0, omega=0.0, delay=0, ramp=1):
    """One row.  The records are sequences of N values; omega = 2 pi cycles_per_frame.
    -> dict(position, owner: lists of int; loudness: list of float (fp64, before the rounding to fp32))"""
    N = len(onset)
    n = min(max(int(count), 0), N)
    o = min(max(int(o), -50), 50)
    floor, default_level = float(F32(floor)), float(F32(default_level))
    onset, frames, pitch, detune = ([int(x) for x in a] for a in (onset, frames, pitch, detune))
    valid = lambda i: frames[i] >= 1 and 0 <= pitch[i] <= 127 and abs(detune[i]) <= MAX_DETUNE       # noqa: E731
    centre = lambda i: pitch[i] * S + (detune[i] if keep_detune else 0) + (0 if concert else 65536 * o) + transpose_units  # noqa: E731
    pos, owner, loud = [], [], []
    for t in range(T):
        i = -1
        for j in range(n):
            if onset[j] <= t:
                i = j
        p, own, lo = HOLD, -1, floor
        if i < 0:
            if n > 0 and valid(0):
                p = centre(0)
        elif valid(i):
            p = b = centre(i)
            k = t - onset[i]
            if k < frames[i]:
                own = i
                if glide > 0 and k < glide and i > 0 and valid(i - 1) and onset[i] <= onset[i - 1] + frames[i - 1]:
                    p += rdiv((centre(i - 1) - b) * (glide - k), glide + 1)
                if depth_units > 0 and k >= delay:
                    p += round(depth_units * min(1.0, (k - delay + 1) / ramp) * math.sin(omega * (k - delay)))
                length = frames[i] if i + 1 >= n else min(frames[i], onset[i + 1] - onset[i])
                lv = float(level[i]) if level[i] == level[i] else default_level
                ga = min(1.0, (k + 1) / attack) if attack > 0 else 1.0
                gr = min(1.0, (length - k) / release) if release > 0 else 1.0
                lo = floor + (lv - floor) * ga * gr
        pos.append(p)
        owner.append(own)
        loud.append(lo)
    return dict(position=pos, owner=owner, loudness=loud)


def controls_of(position):
    """positions (ints) -> (normalized_cents, f0) fp32 arrays, formed in fp64"""
    c = np.array([p / 65536.0 for p in np.asarray(position).reshape(-1)], dtype=np.float64).reshape(np.shape(position))
    return ((c - K) / 7180.0).astype(F32), (440.0 * np.exp2((c - 6900.0) / 1200.0)).astype(F32)


def render(rec, offset, T, **options):
    """dict of [B, N] record arrays and count [B] -> dict of [B, T] arrays"""
    B = rec["onset"].shape[0]
    per = lambda x, b: int(x[b if len(x) > 1 else 0]) if hasattr(x, "__len__") else int(x)      # noqa: E731
    rows = [render_row(rec["onset"][b], rec["frames"][b], rec["pitch"][b], rec["detune"][b], rec["level"][b], rec["count"][b],
                       per(offset, b), T, **options) for b in range(B)]
    position = np.array([r["position"] for r in rows], dtype=np.int64).reshape(B, T)
    owner = np.array([r["owner"] for r in rows], dtype=np.int32).reshape(B, T)
    cents, f0 = controls_of(position)
    return dict(position=position, owner=owner, cents=cents, f0=f0, loudness=np.array([r["loudness"] for r in rows]).astype(F32).reshape(B, T),
                harmonicity=(owner >= 0).astype(F32), voiced=owner >= 0)
