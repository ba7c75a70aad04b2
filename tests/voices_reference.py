"""The two definitions of polyphony (include/ddsp_hip.h: ddsp_voices_allocate, ddsp_voices_mix) as plain
Python loops: the allocation on Python ints, the mix in fp64.  The tests compare the package's CPU path and the kernels with them."""
import math
import struct

NO_PITCH = -(1 << 31)
MAX_DETUNE = 1 << 30
ASSIGN = {"lowest": 0, "oldest": 1, "nearest": 2}
STEAL = {"oldest": 0, "quietest": 1, "drop": 2}
NAN = float("nan")


def level_order(x):
    """the uint32 that orders fp32 values; a NaN is the largest"""
    if x != x:
        return 0xFFFFFFFF
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def allocate_row(onset, frames, pitch, detune, level, count, V, Nv, assign, steal, gap):
    """One score row (sequences of N values, `count` its notes) -> dict: per voice the records `onset`, `frames`, `pitch`, `detune`,
    `level` and `index` (lists of Nv values), `count` [V]; per source note `voice` and `slot` [N]; `stolen`, `dropped`."""
    N = len(onset)
    n = min(max(int(count), 0), N)
    fill = dict(onset=-1, frames=0, pitch=NO_PITCH, detune=0, level=NAN, index=-1)
    out = {k: [[v] * Nv for _ in range(V)] for k, v in fill.items()}
    until, last_onset, last_pitch = [-(1 << 31)] * V, [0] * V, [None] * V
    last_level, cnt = [NAN] * V, [0] * V
    voice, slot, stolen, dropped = [-1] * N, [-1] * N, 0, 0
    for i in range(n):
        o, f, p, d = int(onset[i]), int(frames[i]), int(pitch[i]), int(detune[i])
        if f < 1 or o < 0 or not 0 <= p <= 127 or abs(d) > MAX_DETUNE:
            continue                                                            # sounds nowhere
        best = None
        for v in range(V):
            if until[v] + gap <= o:                                             # free
                if assign == 0:
                    k = 0
                elif assign == 1:
                    k = until[v] + (1 << 31)
                else:
                    k = 128 if last_pitch[v] is None else abs(p - last_pitch[v])
                key = k * 64 + v
                best = key if best is None or key < best else best
        if best is None:
            if steal == 2:
                dropped += 1
                continue
            for v in range(V):
                key = (last_onset[v] if steal == 0 else level_order(last_level[v])) * 64 + v
                best = key if best is None or key < best else best
            w = best % 64
            stolen += 1
            if 1 <= cnt[w] <= Nv:                                               # the stolen note ends where this one begins
                out["frames"][w][cnt[w] - 1] = max(0, min(until[w] - last_onset[w], o - last_onset[w]))
        else:
            w = best % 64
        if cnt[w] < Nv:
            s = cnt[w]
            out["onset"][w][s], out["frames"][w][s], out["pitch"][w][s], out["detune"][w][s] = o, f, p, d
            out["level"][w][s], out["index"][w][s] = level[i], i
            slot[i] = s
        voice[i] = w
        cnt[w] += 1
        until[w], last_onset[w], last_pitch[w], last_level[w] = o + f, o, p, level[i]
    return dict(out, count=cnt, voice=voice, slot=slot, stolen=stolen, dropped=dropped)


def envelope(active, hold, fade):
    """active: T truth values -> e[t] as Python floats"""
    e, last = [], None
    for t, on in enumerate(active):
        if on:
            last = t
        if last is None:
            e.append(0.0)
            continue
        d = t - last
        e.append(1.0 if d <= hold else max(0.0, (fade - (d - hold)) / fade) if fade > 0 else 0.0)
    return e


# The bound on |fp32 result - fp64 definition| for one output sample is ROUNDINGS(V) 2^-24 times the sum of the terms' magnitudes.
# One term gains g audio, as the kernel and the CPU path form it (no fused multiply-add), carries at most six roundings:
#   g = fl(a (hop - r) + a' r) * fl(1 / fl(F hop))      the numerator is an exact integer below 2^31: its conversion      1
#                                                       the denominator's conversion                                      1
#                                                       the reciprocal                                                    1
#                                                       the product                                                       1
#   (gains * g) * audio                                 two products                                                      2
# (without a gate only one product), and the sum over V voices in ascending order adds V - 1 more, each relative to a partial sum
# that the magnitudes bound.  That is V + 5; the issue's V + 6 leaves one unit for the second-order terms.
def roundings(V):
    return V + 6


def mix(audio, gains, active, V, hop, hold, fade):
    """audio: B V rows of L floats; gains [B][V][C]; active: B V rows of T truth values, or None.
    -> (want, magnitude), each [B][C][L] of Python floats: the definition in fp64 and the sum of its terms' magnitudes"""
    B, C, L = len(audio) // V, len(gains[0][0]), len(audio[0])
    want = [[[0.0] * L for _ in range(C)] for _ in range(B)]
    mag = [[[0.0] * L for _ in range(C)] for _ in range(B)]
    for b in range(B):
        for v in range(V):
            row = audio[b * V + v]
            e = None if active is None else envelope(active[b * V + v], hold, fade)
            T = 0 if e is None else len(e)
            for n in range(L):
                g = 1.0
                if e is not None:
                    t = min(n // hop, T - 1)
                    g = e[t] + (e[min(t + 1, T - 1)] - e[t]) * (n % hop) / hop
                x = g * float(row[n])
                for c in range(C):
                    term = float(gains[b][v][c]) * x
                    want[b][c][n] += term
                    mag[b][c][n] += math.fabs(term)
    return want, mag
