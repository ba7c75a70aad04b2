"""Polyphony: voice allocation and mixdown (csrc/ddsp_voices.hip).

The oscillator bank has one f0 per row, and the note layer of notes.py is monophonic: a later note cuts an earlier one off.  A
score whose notes overlap is therefore played by V monophonic voices, each a row of the batch the decoder already handles:

  allocate_voices       Notes of B rows -> Notes of B V rows (row b V + v is voice v of score b): which voice plays which note,
                        decided note by note in slot order -- a free voice by 'lowest', 'oldest' or 'nearest', else a stolen one
                        ('oldest', 'quietest') or the note dropped ('drop')
  mix_voices            audio [B V, L] -> [B, L], or [B, 2, L] with `pan`: the voices summed in ascending order in fp32, each under
                        its gain and, with `active`, under a gate that follows the voice's on frames (hold, then a linear fade)

`AutoEncoder.play(notes, voices=V)` chains them around render_notes and the decoder.  Allocation is integer arithmetic: CUDA
tensors run the kernel, CPU tensors the same definition as numpy operations, to the same bits; the mix agrees with its fp64
definition within (V + 6) 2^-24 of the sum of the terms' magnitudes (tests/voices_reference.py has both as plain loops and the
count of the roundings).  Neither call synchronises with the host or allocates after its outputs."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .encoder import _refuse_grad
from .notes import MAX_DETUNE, NO_PITCH, Notes, _count

ASSIGN = {"lowest": 0, "oldest": 1, "nearest": 2}               # DDSP_VOICES_*
STEAL = {"oldest": 0, "quietest": 1, "drop": 2}
MAX_VOICES = 64
MAX_GAP = 1 << 24
MAX_LOOK_BACK = 1 << 16                                         # hold + fade stays below it
MAX_HOP = 1 << 15
_NAN = np.float32(np.nan)
_RECORDS = ("onset", "frames", "pitch", "detune", "level")


# ------------------------------------------------------------------------------------------------------------------ the CPU path
def _level_order_host(level):
    """fp32 array -> int64 array of the uint32 keys that order the values; a NaN is the largest"""
    u = np.ascontiguousarray(level, dtype=np.float32).view(np.uint32).astype(np.int64)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(level), 0xFFFFFFFF, k)


def _allocate_host(onset, frames, pitch, detune, level, count, V, Nv, assign, steal, gap):
    """The definition of ddsp_voices_allocate (include/ddsp_hip.h), every row at once, note by note.
    -> (the voices' onset, frames, pitch, detune, level [B V, Nv], count [B V], index [B V, Nv], voice, slot [B, N], stats [B, 2])"""
    B, N = onset.shape
    n = np.clip(count.astype(np.int64), 0, N)
    lanes, rows, big = np.arange(V, dtype=np.int64), np.arange(B), np.iinfo(np.int64).max
    until = np.full((B, V), -(1 << 31), dtype=np.int64)
    last_onset, last_pitch = np.zeros((B, V), dtype=np.int64), np.full((B, V), -1, dtype=np.int64)
    last_level, cnt = np.full((B, V), _NAN, dtype=np.float32), np.zeros((B, V), dtype=np.int64)
    out = dict(onset=np.full((B, V, Nv), -1, dtype=np.int32), frames=np.zeros((B, V, Nv), dtype=np.int32),
               pitch=np.full((B, V, Nv), NO_PITCH, dtype=np.int32), detune=np.zeros((B, V, Nv), dtype=np.int32),
               level=np.full((B, V, Nv), _NAN, dtype=np.float32), index=np.full((B, V, Nv), -1, dtype=np.int32))
    voice, slot = np.full((B, N), -1, dtype=np.int32), np.full((B, N), -1, dtype=np.int32)
    stats = np.zeros((B, 2), dtype=np.int32)
    for i in range(N):
        o, f, p, d = (x[:, i].astype(np.int64) for x in (onset, frames, pitch, detune))
        live = (i < n) & (f >= 1) & (o >= 0) & (p >= 0) & (p <= 127) & (np.abs(d) <= MAX_DETUNE)
        if not live.any():
            continue
        free = until + gap <= o[:, None]
        if assign == 0:
            k = np.zeros((B, V), dtype=np.int64)
        elif assign == 1:
            k = until + (1 << 31)
        else:
            k = np.where(last_pitch < 0, 128, np.abs(p[:, None] - last_pitch))
        key = np.where(free, (k << 6) | lanes, big).min(axis=1)
        has = key != big
        none = live & ~has                                                      # no voice is free
        if steal == 2:
            stats[:, 1] += none
            takes, steals = live & has, np.zeros(B, dtype=bool)
        else:
            sk = last_onset if steal == 0 else _level_order_host(last_level)
            key = np.where(has, key, ((sk << 6) | lanes).min(axis=1))
            stats[:, 0] += none
            takes, steals = live, none
        r = rows[takes]
        w = key[takes] & 63
        rs, ws = r[steals[takes]], w[steals[takes]]                             # the stolen notes end where the new ones begin
        c = cnt[rs, ws]
        ok = (c >= 1) & (c - 1 < Nv)
        cut = np.maximum(0, np.minimum(o[rs] - last_onset[rs, ws], until[rs, ws] - last_onset[rs, ws]))
        out["frames"][rs[ok], ws[ok], c[ok] - 1] = cut[ok]
        c = cnt[r, w]
        ok = c < Nv
        for name, x in zip(_RECORDS, (onset, frames, pitch, detune, level)):
            out[name][r[ok], w[ok], c[ok]] = x[r[ok], i]
        out["index"][r[ok], w[ok], c[ok]] = i
        voice[r, i] = w
        slot[r, i] = np.where(ok, c, -1)
        cnt[r, w] += 1
        until[r, w] = o[r] + f[r]
        last_onset[r, w], last_pitch[r, w], last_level[r, w] = o[r], p[r], level[r, i]
    flat = {k: v.reshape(B * V, Nv) for k, v in out.items()}
    return (*(flat[k] for k in _RECORDS), cnt.reshape(B * V).astype(np.int32), flat["index"], voice, slot, stats)


def _envelope_host(active, hold, fade):
    """active bool [T] -> int64 [T]: max(fade, 1) e[t], an integer"""
    T = active.shape[0]
    t = np.arange(T, dtype=np.int64)
    last = np.maximum.accumulate(np.where(active, t, -1))
    d = t - last
    num = np.where(d <= hold, max(fade, 1), np.clip(fade - (d - hold), 0, None))
    return np.where(last < 0, 0, num).astype(np.int64)


def _mix_host(audio, gains, active, hop, hold, fade):
    """The definition of ddsp_voices_mix with the kernel's roundings: audio fp32 [B, V, L], gains fp32 [B, V, C], active bool
    [B, V, T] or None -> fp32 [B, C, L]"""
    B, V, L = audio.shape
    C = gains.shape[2]
    out = np.empty((B, C, L), dtype=np.float32)
    if active is not None:
        T = active.shape[2]
        n = np.arange(L, dtype=np.int64)
        q = n // hop
        r = n - q * hop
        t = np.minimum(q, T - 1)
        t1 = np.minimum(t + 1, T - 1)
        whole = max(fade, 1) * hop
        inv = np.float32(1.0) / np.float32(whole)
    for b in range(B):
        acc = [None] * C
        for v in range(V):
            a = audio[b, v]
            if active is not None:
                e = _envelope_host(active[b, v], hold, fade)
                num = e[t] * (hop - r) + e[t1] * r
                g = np.where(num == whole, np.float32(1.0), num.astype(np.float32) * inv)
            for c in range(C):
                term = (gains[b, v, c] * g) * a if active is not None else gains[b, v, c] * a
                acc[c] = term if v == 0 else acc[c] + term
        for c in range(C):
            out[b, c] = acc[c]
    return out


# ------------------------------------------------------------------------------------------------------------------ the calls
def _voices(voices, what):
    return _count(voices, "voices", what, 1, MAX_VOICES + 1)


def allocate_voices(notes: Notes, voices: int, assign: str = "nearest", steal: str = "oldest", gap: int = 0, max_notes=None,
                    return_info: bool = False):
    """Notes of B rows, whose notes may overlap -> Notes of B `voices` rows in which none does: row b V + v holds the notes voice
    v of score b plays, in order, `max_notes` slots each (None: as many as the score has).  `render_notes` and the decoder take the
    result as any other batch; `mix_voices` sums the rows back.

    The notes are placed one by one in slot order (onsets in order: Notes.sorted()); a note render_notes would sound nowhere is
    skipped.  A voice is free once its last note has ended `gap` frames ago.  Among the free voices `assign` chooses: 'lowest'
    the lowest voice, 'oldest' the one whose last note ended first (round robin), 'nearest' the one whose last pitch is nearest
    the note's (a line stays in its voice and a re-struck pitch returns to it; a voice that never played counts as 128 semitones
    away); ties go to the lowest voice.  With no voice free `steal` decides: 'oldest' takes the voice whose note began first,
    'quietest' the one whose note has the smallest level (a note without a level is never chosen), and the stolen note is cut
    off at the new note's onset; 'drop' leaves the new note out.  A voice that gets more notes than it has slots counts them
    and writes nothing past the last slot (Notes.validate() tells).

    offset and root are repeated per voice where the score has one per row; the scale and the options are carried over.
    return_info=True -> (notes, info): `voice` and `slot` int32 [B, N] (where each note went; -1: nowhere), `index` int32
    [B V, Nv] (the source slot of each voice note, -1 in unused slots: what `render_notes(..., source=)` takes, so that an
    Expression repeated V times row-wise still finds every note's curve), `stolen` and `dropped` int32 [B].  One launch."""
    what = "allocate_voices"
    if not isinstance(notes, Notes):
        raise ValueError(f"{what}: notes must be a Notes, got {type(notes).__name__}")
    V = _voices(voices, what)
    if assign not in ASSIGN or steal not in STEAL:
        raise ValueError(f"{what}: assign must be one of {sorted(ASSIGN)} and steal one of {sorted(STEAL)}, got {assign!r} and {steal!r}")
    gap = _count(gap, "gap", what, 0, MAX_GAP)
    B, N = notes.rows, notes.max_notes
    Nv = N if max_notes is None else _count(max_notes, "max_notes", what)
    if B * N >= 1 << 31 or B * V * Nv >= 1 << 31:
        raise ValueError(f"{what}: {B} rows of {N} slots into {V} voices of {Nv} slots: a call takes fewer than 2^31 slots")
    _refuse_grad(notes.level, what)
    a, s = ASSIGN[assign], STEAL[steal]
    if notes.onset.is_cuda:
        dev = notes.device
        rec = torch.empty((5, B * V, Nv), device=dev, dtype=torch.int32)         # onset, frames, pitch, detune, index
        level = torch.empty((B * V, Nv), device=dev, dtype=torch.float32)
        count = torch.empty(B * V, device=dev, dtype=torch.int32)
        where = torch.empty((2, B, N), device=dev, dtype=torch.int32)
        stats = torch.empty((B, 2), device=dev, dtype=torch.int32)
        ptr = lambda x: x.data_ptr() if x.numel() else None                   # noqa: E731
        with torch.cuda.device(dev):
            rc = _lib.lib().ddsp_voices_allocate(ptr(notes.onset), ptr(notes.frames), ptr(notes.pitch), ptr(notes.detune), ptr(notes.level),
                                                 notes.count.data_ptr(), ptr(rec[0]), ptr(rec[1]), ptr(rec[2]), ptr(rec[3]), ptr(level),
                                                 ptr(count), ptr(rec[4]), ptr(where[0]), ptr(where[1]), ptr(stats), B, N, V, Nv, a, s, gap,
                                                 torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_voices_allocate")
        fields = (rec[0], rec[1], rec[2], rec[3], level, count)
        index, voice, slot = rec[4], where[0], where[1]
    else:
        got = _allocate_host(*(getattr(notes, k).numpy() for k in _RECORDS), notes.count.numpy(), V, Nv, a, s, gap)
        fields = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in got[:6])
        index, voice, slot, stats = (torch.from_numpy(np.ascontiguousarray(x)) for x in got[6:])
    per_voice = lambda x: x.repeat_interleave(V) if notes.groups > 1 else x    # noqa: E731
    found = Notes(*fields, offset=per_voice(notes.offset), root=per_voice(notes.root), **notes.options())
    if not return_info:
        return found
    return found, dict(voice=voice, slot=slot, index=index, stolen=stats[:, 0], dropped=stats[:, 1])


def _gain_table(gain, pan, B, V, device, what):
    """gain [V] or [B, V] (None: 1) and pan [V] or [B, V] in -1 .. 1 (None: one channel) -> fp32 [B, V, C] on `device`: constant-power
    gains gain cos((pan + 1) pi / 4) and gain sin((pan + 1) pi / 4), formed in fp64.  Values that live on the host are checked;
    a pan already on the device is clamped instead, which needs no read-back."""
    def table(x, name):
        on_host = not (isinstance(x, torch.Tensor) and x.is_cuda)
        x = torch.as_tensor(x, dtype=torch.float64) if on_host else x.detach().to(torch.float64)
        if x.dim() == 1:
            x = x[None].expand(B, -1)
        if x.shape != (B, V):
            raise ValueError(f"{what}: {name} must be [{V}] or [{B}, {V}], got {tuple(x.shape)}")
        if on_host and not bool(torch.isfinite(x).all()):
            raise ValueError(f"{what}: {name} must be finite")
        return x, on_host

    if gain is None and pan is None:
        return torch.ones((B, V, 1), device=device, dtype=torch.float32)
    g = 1.0 if gain is None else table(gain, "gain")[0]
    if pan is None:
        return g.to(device=device, dtype=torch.float32).reshape(B, V, 1).contiguous()
    p, on_host = table(pan, "pan")
    if on_host and not bool((p.abs() <= 1.0).all()):
        raise ValueError(f"{what}: pan must lie in -1 .. 1")
    theta = (p.clamp(-1.0, 1.0) + 1.0) * (math.pi / 4.0)
    if gain is not None:                                                        # (one of the two on the device: the other follows it there)
        both = g.device if g.is_cuda else theta.device
        g, theta = g.to(both), theta.to(both)
    return torch.stack((g * torch.cos(theta), g * torch.sin(theta)), dim=2).to(device=device, dtype=torch.float32).contiguous()


def mix_voices(audio: torch.Tensor, voices: int, gain=None, pan=None, active=None, hop_length=None, hold: int = 0, fade: int = 0,
               out=None) -> torch.Tensor:
    """audio fp32 [B V, L] (row b V + v is voice v of score b, as allocate_voices orders them) -> [B, L]: the voices summed in
    ascending order in fp32.  `gain` ([V] or [B, V]) weighs them; `pan` ([V] or [B, V], -1 left .. 1 right) gives [B, 2, L] with
    constant-power gains, formed in fp64 before the call.

    `active` (render_notes' `voiced` of the B V rows, [B V, T, 1] or [B V, T], with `hop_length`) gates each voice: an idle
    voice's decoder still emits its noise floor, and V of them add up.  The gate is 1 up to `hold` frames after the voice's last
    active frame, falls linearly to 0 over the next `fade` frames (fade=0: at once), is 0 where the voice has not played yet,
    and is interpolated linearly between frames; hold + fade stays below 2^16.  `out` takes the result.  One launch."""
    what = "mix_voices"
    V = _voices(voices, what)
    if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or audio.shape[0] % V or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"{what}: audio must be [B * {V}, L] with B, L >= 1, got "
                         f"{tuple(audio.shape) if isinstance(audio, torch.Tensor) else type(audio).__name__}")
    _refuse_grad(audio, what)
    dev = audio.device
    B, L = audio.shape[0] // V, audio.shape[1]
    hold, fade = _count(hold, "hold", what), _count(fade, "fade", what)
    if hold + fade >= MAX_LOOK_BACK:
        raise ValueError(f"{what}: hold + fade must stay below {MAX_LOOK_BACK} frames, got {hold} + {fade}")
    if L >= 1 << 31 or B * V * L >= 1 << 47:
        raise ValueError(f"{what}: {B * V} rows of {L} samples: a row takes fewer than 2^31 samples, a call fewer than 2^47")
    T, hop = 0, 0
    if active is not None:
        if hop_length is None:
            raise ValueError(f"{what}: active counts frames; hop_length says how long one is")
        hop = _count(hop_length, "hop_length", what, 1, MAX_HOP + 1)
        if not isinstance(active, torch.Tensor) or active.dtype not in (torch.bool, torch.uint8) or active.device != dev:
            raise ValueError(f"{what}: active must be a bool or uint8 tensor on {dev}")
        if active.dim() == 3 and active.shape[2] == 1:
            active = active[..., 0]
        if active.dim() != 2 or active.shape[0] != B * V or active.shape[1] < 1:
            raise ValueError(f"{what}: active must be [{B * V}, T] or [{B * V}, T, 1] with T >= 1, got {tuple(active.shape)}")
        T = active.shape[1]
        active = active.contiguous()
        active = active.view(torch.uint8) if active.dtype == torch.bool else active
    gains = _gain_table(gain, pan, B, V, dev, what)
    C = gains.shape[2]
    shape = (B, L) if pan is None else (B, 2, L)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    elif not isinstance(out, torch.Tensor) or out.shape != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous fp32 {shape} tensor on {dev}")
    x = audio.detach().float().contiguous()
    if x.is_cuda:
        with torch.cuda.device(dev):
            rc = _lib.lib().ddsp_voices_mix(x.data_ptr(), gains.data_ptr(), None if active is None else active.data_ptr(), out.data_ptr(),
                                            B, V, C, L, T, hop, hold, fade, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_voices_mix")
        return out
    act = None if active is None else active.numpy().reshape(B, V, T) != 0
    out.copy_(torch.from_numpy(_mix_host(x.numpy().reshape(B, V, L), gains.numpy(), act, hop, hold, fade)).reshape(shape))
    return out
