"""The definitions of `note_expression` and of `render_notes(..., expression=...)` (include/ddsp_hip.h:
ddsp_notes_expression, ddsp_notes_render_expr) as plain loops over Python ints and floats, independent of the package.  The
plain render underneath is tests/notes_reference.py's, term for term; positions, `rdiv` and the conventions are
tests/tuning_reference.py's: a position is a Python int counting 2^-16 cent on the MIDI scale."""
import numpy as np

import notes_reference as nref
from tuning_reference import F32, LIMIT, S, position

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def valid(frames, pitch, detune):
    return frames >= 1 and 0 <= pitch <= 127 and abs(detune) <= nref.MAX_DETUNE


def expression_row(cents, onset, frames, pitch, detune, count, o):
    """One row: cents fp32 [T], the records sequences of N values -> (bend, owner): lists of T ints"""
    N = len(onset)
    n = min(max(int(count), 0), N)
    o = min(max(int(o), -50), 50)
    onset, frames, pitch, detune = ([int(x) for x in a] for a in (onset, frames, pitch, detune))
    bend, owner = [], []
    for t in range(len(cents)):
        i = -1
        for j in range(n):
            if onset[j] <= t:
                i = j
        b, own = 0, -1
        if i >= 0 and valid(frames[i], pitch[i], detune[i]) and t < onset[i] + frames[i] and abs(float(cents[t])) <= LIMIT:
            own = i
            b = position(cents[t]) - 65536 * o - pitch[i] * S - detune[i]
            b = min(max(b, INT32_MIN), INT32_MAX)               # records that do not match the track: saturated
        bend.append(b)
        owner.append(own)
    return bend, owner


def expression(cents, rec, offset):
    """cents [B, T], dict of [B, N] record arrays and count [B] -> dict(bend, owner: int32 [B, T])"""
    B = cents.shape[0]
    per = lambda x, b: int(x[b if len(x) > 1 else 0]) if hasattr(x, "__len__") else int(x)      # noqa: E731
    rows = [expression_row(cents[b], rec["onset"][b], rec["frames"][b], rec["pitch"][b], rec["detune"][b], rec["count"][b], per(offset, b))
            for b in range(B)]
    return dict(bend=np.array([r[0] for r in rows], dtype=np.int64).astype(np.int32).reshape(cents.shape),
                owner=np.array([r[1] for r in rows], dtype=np.int32).reshape(cents.shape))


def time_map(Ls, Lp, keep_attack, keep_release, k):
    """Destination frame k (0 <= k < Lp) of a note that sounds Lp frames -> (q, f): frame q of its source note of Ls frames and
    a fraction f in 2^-16 frame.  Python ints throughout."""
    a = min(keep_attack, Ls, Lp)
    r = min(keep_release, Ls - a, Lp - a)
    if k < a:
        q, f = k, 0
    elif k >= Lp - r:
        q, f = Ls - (Lp - k), 0
    else:
        m, Ns, D = k - a + 1, Ls - a - r + 1, Lp - a - r + 1
        q, f = a - 1 + (m * Ns) // D, (((m * Ns) % D) * 65536) // D
    if q < 0:
        return 0, 0
    if q >= Ls - 1:
        return Ls - 1, 0
    return q, f


def render_expr_row(onset, frames, pitch, detune, level, count, o, T, source, src_onset, src_frames, src_level, src_count, bend, src_loudness,
                    bend_amount=1.0, dyn_amount=1.0, keep_attack=0, keep_release=0, **options):
    """One row.  The plain render (notes_reference.render_row and its options), then on every on frame the source's curves.
    source: a sequence of N ints or None; the source records: sequences of Nsrc values; bend: Tsrc ints; src_loudness: Tsrc fp32
    values or None.  -> dict(position, owner: lists of int; loudness: list of float, before the rounding to fp32)"""
    out = nref.render_row(onset, frames, pitch, detune, level, count, o, T, **options)
    n = min(max(int(count), 0), len(onset))
    n_src = min(max(int(src_count), 0), len(src_onset))
    Tsrc = len(bend)
    for t in range(T):
        i = out["owner"][t]
        if i < 0:
            continue
        k = t - int(onset[i])
        Lp = int(frames[i]) if i + 1 >= n else min(int(frames[i]), int(onset[i + 1]) - int(onset[i]))
        j = i if source is None else int(source[i])
        if not (k < Lp and 0 <= j < n_src):
            continue
        Ls, so = int(src_frames[j]), int(src_onset[j])
        if not (Ls >= 1 and so >= 0 and so + Ls <= Tsrc):
            continue
        q, f = time_map(Ls, Lp, keep_attack, keep_release, k)
        b = int(bend[so + q])
        if f:
            b += ((int(bend[so + q + 1]) - b) * f + 32768) // 65536
        out["position"][t] += round(float(bend_amount) * float(b))               # round(): ties to even, as llrint
        sl = float(src_level[j])
        if src_loudness is not None and sl == sl and dyn_amount != 0.0:
            with np.errstate(all="ignore"):
                l = np.float64(src_loudness[so + q])
                if f:
                    l = l + (np.float64(src_loudness[so + q + 1]) - l) * np.float64(f / 65536.0)
                out["loudness"][t] = float(np.float64(out["loudness"][t]) + np.float64(dyn_amount) * (l - np.float64(sl)))
    return out


def render_expr(rec, offset, T, src, source=None, **options):
    """rec: dict of [B, N] record arrays and count [B]; src: dict(onset, frames, level [B, Nsrc], count [B], bend int32 [B, Tsrc],
    loudness fp32 [B, Tsrc] or None); source: int [B, N] or None -> dict of [B, T] arrays, as notes_reference.render"""
    B = rec["onset"].shape[0]
    per = lambda x, b: int(x[b if len(x) > 1 else 0]) if hasattr(x, "__len__") else int(x)      # noqa: E731
    rows = [render_expr_row(rec["onset"][b], rec["frames"][b], rec["pitch"][b], rec["detune"][b], rec["level"][b], rec["count"][b],
                            per(offset, b), T, None if source is None else source[b], src["onset"][b], src["frames"][b], src["level"][b],
                            src["count"][b], src["bend"][b], None if src.get("loudness") is None else src["loudness"][b], **options)
            for b in range(B)]
    position = np.array([r["position"] for r in rows], dtype=np.int64).reshape(B, T)
    owner = np.array([r["owner"] for r in rows], dtype=np.int32).reshape(B, T)
    cents, f0 = nref.controls_of(position)
    with np.errstate(all="ignore"):
        loudness = np.array([r["loudness"] for r in rows]).astype(F32).reshape(B, T)
    return dict(position=position, owner=owner, cents=cents, f0=f0, loudness=loudness, harmonicity=(owner >= 0).astype(F32), voiced=owner >= 0)
