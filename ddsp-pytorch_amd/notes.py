"""Notes: the note events of a pitch track, and note events rendered back to controls (DESIGN.md section 10f;
csrc/ddsp_notes.hip).

The unit a musician edits is the note.  `tune_pitch` already finds notes -- runs of on frames with one note_t -- and stops at a
per-frame array; this module turns the runs into a list of events and goes the other way, both on the device:

  Notes                 onset, frames, pitch, detune [B, N] int32, level [B, N] fp32, count [B] int32, offset and root [G] int32,
                        the scale, the source's frame count and the note-on options; to_dict() / from_dict(), .to(device);
                        constructible by hand from Python lists (a score); transpose, transpose_degrees, quantize, sorted,
                        validate; write_midi / read_midi
  extract_notes         a control dict -> Notes (the notes `tune_pitch` would move, as records)
  render_notes          Notes -> a control dict with f0, normalized_cents, loudness, harmonicity and voiced: what the Controller and
                        the oscillator bank read, so a trained decoder can be played from a score
  Expression            what a record does not hold (section 10g): bend [B, T] int32 (each frame's distance from its note's centre),
                        loudness [B, T] fp32 or None, and the source notes' onset, frames, level and count
  note_expression       a control dict and the Notes found on it -> Expression; render_notes(..., expression=e) gives the curves
                        back to the notes after an edit, stretched to each note's new length

Everything is integer arithmetic on positions of 2^-16 cent (include/ddsp_hip.h has the text): CUDA tensors run the kernels
of csrc/ddsp_notes.hip, CPU tensors the same definition as numpy operations, to the same bits in every integer output and in
normalized_cents (tests/notes_reference.py and tests/notes_expression_reference.py have it as plain loops).  No call synchronises
with the host or allocates after its outputs, so all can be captured in a graph."""
from __future__ import annotations

import math
import struct
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .encoder import _refuse_grad
from .tuning import (LIMIT, MAX_HYSTERESIS, ORIGIN, SCALES, SEMITONE, TuningStatistics, _gates, _inputs, _on_host, _positions_host, _root,
                     _row_notes_host, scale_mask, tuning_statistics)

NO_PITCH = -(1 << 31)                                           # the pitch of an unused slot
HOLD = 6900 * 65536                                             # the position held where no note gives one (A4)
MAX_DETUNE = 1 << 30
MAX_STEPS = 1 << 24                                             # glide, attack, release, delay and ramp stay below it
MAX_TRANSPOSE = 128.0                                           # semitones
MAX_AMOUNT = 16.0                                               # |bend_amount| and |dynamics_amount| up to it
_KEEP_DETUNE, _CONCERT = 1, 2                                   # DDSP_NOTES_*
_NAN = np.float32(np.nan)
TICKS_PER_QUARTER, TEMPO = 480, 500000                          # write_midi: 120 quarter notes a minute, 960 ticks a second


class Notes:
    """Note events, row by row: `onset` (first frame), `frames` (length), `pitch` (MIDI note), `detune` (units of 2^-16 cent
    above the pitch, on the performance's own grid) as [B, N] int32, `level` [B, N] fp32 (the note's largest loudness; NaN:
    none), `count` [B] int32 (the notes of the row; more than N after an overflow).  Slots from min(count, N) on hold onset -1,
    frames 0, pitch INT32_MIN, detune 0, level NaN.  `offset` and `root` [G] int32 (G = 1 or B) and `scale` are the tuning the
    notes were found with, `source_frames` the length of the track they came from (None for a score), `silence` and
    `confidence` the note-on options.

    By hand: Notes(onset=[0, 10], frames=[10, 8], pitch=[60, 62]) is one row; nested lists give several rows of equal length
    (pad with count).  detune defaults to 0, level to NaN (render_notes' default_level), count to N, offset and root to 0."""

    def __init__(self, onset, frames, pitch, detune=None, level=None, count=None, offset=0, root=0, scale="major", source_frames=None,
                 silence=None, confidence: float = 0.0):
        dev = onset.device if isinstance(onset, torch.Tensor) else None

        def records(x, dtype, name):
            x = torch.as_tensor(x, dtype=dtype, device=dev)
            x = x.reshape(1, -1) if x.dim() < 2 else x
            if x.dim() != 2:
                raise ValueError(f"Notes: {name} must be [B, N] (or one row [N]), got {tuple(x.shape)}")
            return x.contiguous()

        self.onset = records(onset, torch.int32, "onset")
        dev = self.onset.device
        B, N = self.onset.shape
        self.frames = records(frames, torch.int32, "frames")
        self.pitch = records(pitch, torch.int32, "pitch")
        self.detune = records(detune, torch.int32, "detune") if detune is not None else torch.zeros((B, N), dtype=torch.int32, device=dev)
        self.level = records(level, torch.float32, "level") if level is not None else \
            torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
        for name in ("frames", "pitch", "detune", "level"):
            if getattr(self, name).shape != (B, N):
                raise ValueError(f"Notes: {name} is {tuple(getattr(self, name).shape)}, onset {(B, N)}")
        if count is None:
            count = torch.full((B,), N, dtype=torch.int32, device=dev)
        self.count = torch.as_tensor(count, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        if self.count.shape[0] != B:
            raise ValueError(f"Notes: count must hold one value per row ({B}), got {self.count.shape[0]}")
        by_hand = not isinstance(offset, torch.Tensor)
        self.offset = torch.as_tensor(offset, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        self.root = torch.as_tensor(root, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        G = self.offset.shape[0]
        if G not in (1, B) or self.root.shape[0] != G:
            raise ValueError(f"Notes: offset and root must hold 1 or {B} values each, got {G} and {self.root.shape[0]}")
        if by_hand and not (bool((self.offset.abs() <= 50).all()) and bool(((self.root >= 0) & (self.root <= 11)).all())):
            raise ValueError("Notes: an offset lies within +-50 cents, a root in 0 .. 11")
        self.mask = scale_mask(scale, "Notes")
        self.scale = scale if isinstance(scale, str) else int(scale)
        if source_frames is not None and (isinstance(source_frames, bool) or not isinstance(source_frames, (int, np.integer)) or source_frames < 0):
            raise ValueError(f"Notes: source_frames must be None or a non-negative int, got {source_frames!r}")
        self.source_frames = None if source_frames is None else int(source_frames)
        self.silence = None if silence is None else float(silence)
        self.confidence = float(confidence)

    # ------------------------------------------------------------------------------------------------------------ the object
    @property
    def rows(self) -> int:
        return self.onset.shape[0]

    @property
    def max_notes(self) -> int:
        return self.onset.shape[1]

    @property
    def groups(self) -> int:
        return self.offset.shape[0]

    @property
    def device(self):
        return self.onset.device

    def options(self) -> dict:
        return dict(scale=self.scale, source_frames=self.source_frames, silence=self.silence, confidence=self.confidence)

    def _tensors(self) -> dict:
        return dict(onset=self.onset, frames=self.frames, pitch=self.pitch, detune=self.detune, level=self.level, count=self.count,
                    offset=self.offset, root=self.root)

    def _with(self, **changed) -> "Notes":
        return Notes(**dict(self._tensors(), **changed), **self.options())

    def to(self, device) -> "Notes":
        return Notes(**{k: v.to(device) for k, v in self._tensors().items()}, **self.options())

    def to_dict(self) -> dict:
        """Plain tensors (on the CPU), the scale, ints and floats."""
        return dict({k: v.cpu() for k, v in self._tensors().items()}, **self.options())

    @classmethod
    def from_dict(cls, d: dict) -> "Notes":
        return cls(**{k: d[k] for k in ("onset", "frames", "pitch", "detune", "level", "count", "offset", "root", "scale", "source_frames",
                                        "silence", "confidence")})

    def tuning(self) -> TuningStatistics:
        """the tuning the notes were found with, for tune_pitch or extract_notes"""
        return TuningStatistics(self.offset, self.root, scale=self.scale, silence=self.silence, confidence=self.confidence)

    def _used(self) -> torch.Tensor:
        """[B, N] bool: the slots below min(count, N)"""
        return torch.arange(self.max_notes, device=self.device)[None] < self.count[:, None]

    # -------------------------------------------------------------------------------------------------------------- the edits
    def transpose(self, semitones) -> "Notes":
        """Every note `semitones` higher: whole semitones move the pitch, a fraction goes into detune.  -> a new Notes."""
        whole = int(round(float(semitones)))
        rest = int(round((float(semitones) - whole) * SEMITONE))
        live = self.pitch != NO_PITCH
        return self._with(pitch=torch.where(live, self.pitch + whole, self.pitch),
                          detune=torch.where(live, self.detune + rest, self.detune))

    def transpose_degrees(self, k: int) -> "Notes":
        """Every pitch moves `k` allowed notes of its own scale and root: the k-th allowed note above it (below, for k < 0).
        Integer tensor operations on the notes' own device; -> a new Notes."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"transpose_degrees: k must be an int, got {k!r}")
        if k == 0:
            return self._with()
        dev = self.device
        classes = [c for c in range(12) if (self.mask >> c) & 1]
        D = len(classes)
        allowed = torch.tensor([(self.mask >> c) & 1 for c in range(12)], dtype=torch.int64, device=dev)
        below = torch.tensor([sum((self.mask >> c) & 1 for c in range(rel)) for rel in range(12)], dtype=torch.int64, device=dev)
        table = torch.tensor(classes, dtype=torch.int64, device=dev)
        live = self.pitch != NO_PITCH
        p = torch.where(live, self.pitch, torch.zeros_like(self.pitch)).to(torch.int64)
        r = torch.remainder(self.root.to(torch.int64), 12)[:, None]            # [G, 1] broadcasts over the rows
        rel = torch.remainder(p - r, 12)
        octave = torch.div(p - r - rel, 12, rounding_mode="floor")
        index = octave * D + below[rel]                                         # of the pitch itself, or of the allowed note above it
        if k > 0:
            index = index - (1 - allowed[rel])                                  # off the scale: count from the allowed note below
        index = index + int(k)
        up = torch.div(index, D, rounding_mode="floor")
        moved = r + 12 * up + table[index - up * D]
        return self._with(pitch=torch.where(live, moved.to(torch.int32), self.pitch))

    def quantize(self, grid_frames: int) -> "Notes":
        """Onsets go to the nearest multiple of `grid_frames`, ties down; lengths are kept, the order is preserved."""
        g = grid_frames
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or g < 1:
            raise ValueError(f"quantize: grid_frames must be a positive int, got {g!r}")
        o = self.onset.to(torch.int64)
        snapped = torch.div(2 * o + (int(g) - 1), 2 * int(g), rounding_mode="floor") * int(g)
        return self._with(onset=torch.where(self._used(), snapped.to(torch.int32), self.onset))

    def sorted(self, return_order: bool = False):
        """The used slots in order of onset (a stable sort), the unused ones behind them.  return_order=True -> (notes, order):
        `order` int32 [B, N], the slot each note came from -- what `render_notes(..., source=order)` needs to find the notes'
        curves in an Expression taken before the sort."""
        key = torch.where(self._used(), self.onset.to(torch.int64), torch.full_like(self.onset, 1 << 31, dtype=torch.int64))
        order = torch.sort(key, dim=1, stable=True).indices
        notes = self._with(**{k: torch.gather(getattr(self, k), 1, order) for k in ("onset", "frames", "pitch", "detune", "level")})
        return (notes, order.to(torch.int32)) if return_order else notes

    def validate(self) -> "Notes":
        """Raises a ValueError on count > N or onsets that are not in order.  Opt-in: it synchronises with the device."""
        if bool((self.count > self.max_notes).any()):
            raise ValueError(f"Notes: a row holds more notes than its {self.max_notes} slots (count up to {int(self.count.max())})")
        if self.max_notes > 1:
            used = self._used()
            if bool(((self.onset[:, 1:] < self.onset[:, :-1]) & used[:, 1:]).any()):
                raise ValueError("Notes: onsets are not in order; .sorted() puts them in order")
        return self

    # ------------------------------------------------------------------------------------------------- standard MIDI files
    def write_midi(self, path, hop_length: int, sample_rate: int, level_range=(0.0, 1.0), row: int = 0, polyphonic: bool = False) -> None:
        """Row `row` as a standard MIDI file, format 0: one track, 480 ticks per quarter at 120 quarters a minute, velocity
        clamp(round(127 (level - lo) / (hi - lo)), 1, 127) (64 for a NaN level).  A later note cuts an earlier one off, as in
        render_notes; polyphonic=True writes every note at its full length instead (a chord stays a chord; DESIGN.md section
        10i).  detune is not written.  Host only."""
        lo, hi = float(level_range[0]), float(level_range[1])
        if not hi > lo:
            raise ValueError(f"write_midi: level_range must be (lo, hi) with hi > lo, got {level_range!r}")
        n = min(max(int(self.count[row]), 0), self.max_notes)
        onset, frames, pitch = (getattr(self, k)[row, :n].cpu().tolist() for k in ("onset", "frames", "pitch"))
        level = self.level[row, :n].cpu().tolist()
        tick = lambda f: int(round(Fraction(f * int(hop_length) * 2 * TICKS_PER_QUARTER, int(sample_rate))))       # noqa: E731
        events = []                                                             # (tick, 0: off / 1: on, note, velocity)
        for i in range(n):
            length = frames[i] if polyphonic or i + 1 >= n else min(frames[i], onset[i + 1] - onset[i])
            if length < 1 or not 0 <= pitch[i] <= 127 or onset[i] < 0:
                continue
            velocity = 64 if level[i] != level[i] else min(max(int(round(127.0 * (level[i] - lo) / (hi - lo))), 1), 127)
            events.append((tick(onset[i]), 1, pitch[i], velocity))
            events.append((tick(onset[i] + length), 0, pitch[i], 0))
        events.sort(key=lambda e: (e[0], e[1]))
        track, at = bytearray(b"\x00\xff\x51\x03" + TEMPO.to_bytes(3, "big")), 0
        for when, on, note, velocity in events:
            track += _vlq(when - at) + bytes([0x90 if on else 0x80, note, velocity])
            at = when
        track += b"\x00\xff\x2f\x00"
        with open(path, "wb") as f:
            f.write(b"MThd" + struct.pack(">IHHH", 6, 0, 1, TICKS_PER_QUARTER) + b"MTrk" + struct.pack(">I", len(track)) + bytes(track))

    @classmethod
    def read_midi(cls, path, hop_length: int, sample_rate: int, level_range=(0.0, 1.0), polyphonic: bool = False) -> "Notes":
        """A standard MIDI file (format 0, or 1 with its tracks merged) -> one row of Notes on the chromatic scale.  Running
        status and every set-tempo event are honoured, a note-on with velocity 0 is a note-off, a new note-on cuts the sounding
        note (the instrument is monophonic), everything else is ignored.  Files with SMPTE time division are refused.
        polyphonic=True keeps chords: a note-on cuts nothing and a note-off closes the oldest open note of
        its own pitch; the notes come out in order of onset, and of pitch within one onset -- what voices.allocate_voices takes."""
        lo, hi = float(level_range[0]), float(level_range[1])
        with open(path, "rb") as f:
            data = f.read()
        division, events = _midi_events(data)
        events.sort(key=lambda e: (e[0], e[1]))                                 # by tick; tempo, then note-offs, then note-ons
        tempo, at_tick, at_us = TEMPO, 0, Fraction(0)
        notes, sounding = [], None                                              # sounding: (onset frame, note, velocity)
        held = {}                                                               # polyphonic: note -> [(onset frame, velocity)], oldest first

        def close(frame):
            if sounding is not None and frame > sounding[0]:
                notes.append((sounding[0], frame - sounding[0], sounding[1], sounding[2]))

        for when, kind, a, b in events:
            at_us += Fraction((when - at_tick) * tempo, division)
            at_tick = when
            if kind == 0:
                tempo = a
                continue
            frame = int(round(at_us * int(sample_rate) / (1000000 * int(hop_length))))
            if polyphonic:
                if kind == 2:
                    held.setdefault(a, []).append((frame, b))
                elif held.get(a):
                    began, velocity = held[a].pop(0)
                    if frame > began:
                        notes.append((began, frame - began, a, velocity))
                continue
            if kind == 2:
                close(frame)
                sounding = (frame, a, b)
            elif sounding is not None and sounding[1] == a:
                close(frame)
                sounding = None
        if polyphonic:
            notes.sort(key=lambda x: (x[0], x[2]))
        return cls(onset=[x[0] for x in notes], frames=[x[1] for x in notes], pitch=[x[2] for x in notes],
                   level=[lo + x[3] * (hi - lo) / 127.0 for x in notes], scale="chromatic")


class Expression:
    """What a performer gave the notes of a performance beyond the five numbers of a record: `bend`
    int32 [B, T], each frame's distance from its note's centre in units of 2^-16 cent (0 on a frame of no note); `loudness`
    fp32 [B, T], a copy of the performance's loudness track, or None; and the records that say where each note's curve lies:
    the source notes' `onset`, `frames` [B, N] int32, `level` [B, N] fp32 and `count` [B] int32.  `owner` int32 [B, T] (the note
    of each frame, -1 for none) is there when note_expression was asked for it.  `render_notes(notes, ..., expression=e)` reads
    it; the notes may have been edited in between."""

    def __init__(self, bend, loudness, onset, frames, level, count, owner=None):
        self.bend = torch.as_tensor(bend, dtype=torch.int32).contiguous()
        dev = self.bend.device
        if self.bend.dim() != 2 or self.bend.shape[0] < 1 or self.bend.shape[1] < 1:
            raise ValueError(f"Expression: bend must be [B, T] with B, T >= 1, got {tuple(self.bend.shape)}")
        B = self.bend.shape[0]
        self.loudness = None if loudness is None else torch.as_tensor(loudness, dtype=torch.float32, device=dev).contiguous()
        self.owner = None if owner is None else torch.as_tensor(owner, dtype=torch.int32, device=dev).contiguous()
        for name in ("loudness", "owner"):
            x = getattr(self, name)
            if x is not None and x.shape != self.bend.shape:
                raise ValueError(f"Expression: {name} is {tuple(x.shape)}, bend {tuple(self.bend.shape)}")
        self.onset = torch.as_tensor(onset, dtype=torch.int32, device=dev).contiguous()
        self.frames = torch.as_tensor(frames, dtype=torch.int32, device=dev).contiguous()
        self.level = torch.as_tensor(level, dtype=torch.float32, device=dev).contiguous()
        if self.onset.dim() != 2 or self.onset.shape[0] != B or self.frames.shape != self.onset.shape or self.level.shape != self.onset.shape:
            raise ValueError(f"Expression: onset, frames and level must be [{B}, N], got {tuple(self.onset.shape)}, "
                             f"{tuple(self.frames.shape)} and {tuple(self.level.shape)}")
        self.count = torch.as_tensor(count, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        if self.count.shape[0] != B:
            raise ValueError(f"Expression: count must hold one value per row ({B}), got {self.count.shape[0]}")

    @property
    def rows(self) -> int:
        return self.bend.shape[0]

    @property
    def source_frames(self) -> int:
        return self.bend.shape[1]

    @property
    def max_notes(self) -> int:
        return self.onset.shape[1]

    @property
    def device(self):
        return self.bend.device

    def _tensors(self) -> dict:
        return dict(bend=self.bend, loudness=self.loudness, onset=self.onset, frames=self.frames, level=self.level, count=self.count,
                    owner=self.owner)

    def to(self, device) -> "Expression":
        return Expression(**{k: None if v is None else v.to(device) for k, v in self._tensors().items()})

    def to_dict(self) -> dict:
        """Plain tensors (on the CPU); None where there is no loudness or owner."""
        return {k: None if v is None else v.cpu() for k, v in self._tensors().items()}

    @classmethod
    def from_dict(cls, d: dict) -> "Expression":
        return cls(d["bend"], d["loudness"], d["onset"], d["frames"], d["level"], d["count"], d.get("owner"))


def _vlq(value: int) -> bytes:
    out = [value & 0x7F]
    value >>= 7
    while value:
        out.append(0x80 | (value & 0x7F))
        value >>= 7
    return bytes(reversed(out))


def _midi_events(data: bytes):
    """-> (ticks per quarter, [(tick, kind, a, b)]): kind 0 a set-tempo (a: microseconds per quarter), 1 a note-off (a: note),
    2 a note-on (a: note, b: velocity)"""
    if len(data) < 14 or data[:4] != b"MThd":
        raise ValueError("read_midi: not a standard MIDI file")
    length, fmt, tracks, division = struct.unpack(">IHHH", data[4:14])
    if fmt not in (0, 1):
        raise ValueError(f"read_midi: format {fmt} is not supported (0 or 1)")
    if division & 0x8000:
        raise ValueError("read_midi: SMPTE time division is not supported")
    if division == 0:
        raise ValueError("read_midi: a time division of 0 ticks per quarter")
    events, at = [], 8 + length
    for _ in range(tracks):
        if data[at:at + 4] != b"MTrk" or at + 8 > len(data):
            raise ValueError("read_midi: a track chunk is missing")
        end = at + 8 + struct.unpack(">I", data[at + 4:at + 8])[0]
        if end > len(data):
            raise ValueError("read_midi: a track runs past the end of the file")
        i, tick, status = at + 8, 0, 0

        def vlq():
            nonlocal i
            value = 0
            while True:
                if i >= end:
                    raise ValueError("read_midi: a track ends inside an event")
                byte = data[i]
                i += 1
                value = (value << 7) | (byte & 0x7F)
                if not byte & 0x80:
                    return value

        while i < end:
            tick += vlq()
            if i >= end:
                raise ValueError("read_midi: a track ends inside an event")
            if data[i] & 0x80:
                status = data[i]
                i += 1
            elif not 0x80 <= status < 0xF0:
                raise ValueError("read_midi: a data byte without a running status")
            if status == 0xFF:                                                  # meta: type, length, data
                kind = data[i] if i < end else 0
                i += 1
                size = vlq()
                if kind == 0x51 and size == 3 and i + 3 <= end:
                    events.append((tick, 0, int.from_bytes(data[i:i + 3], "big"), 0))
                i += size
                status = 0
            elif status in (0xF0, 0xF7):                                        # system exclusive: length, data
                size = vlq()
                i += size
                status = 0
            elif status >= 0xF0:                                                # system common / real time: not in files; skip their data
                i += {0xF1: 1, 0xF2: 2, 0xF3: 1}.get(status, 0)
                status = 0
            else:
                size = 1 if status & 0xE0 == 0xC0 else 2                        # program change and channel pressure: one data byte
                if i + size > end:
                    raise ValueError("read_midi: a track ends inside an event")
                a, b = data[i], data[i + 1] if size == 2 else 0
                i += size
                if status & 0xF0 == 0x90 and b > 0:
                    events.append((tick, 2, a, b))
                elif status & 0xF0 in (0x80, 0x90):
                    events.append((tick, 1, a, 0))
        at = end
    return division, events


# ------------------------------------------------------------------------------------------------------------------ the CPU path
def _level_host(x):
    """the largest value of an fp32 array that is not a NaN (+0 above -0), the canonical NaN where there is none"""
    x = x[x == x]
    if x.size == 0:
        return _NAN
    m = x.max()
    if m == 0:
        return np.float32(0.0) if (~np.signbit(x[x == 0])).any() else np.float32(-0.0)
    return m


def _extract_row_host(n, on, loud, o, root, mask, h, min_note):
    """-> the kept notes of one row: arrays onset, frames, pitch, detune (int64) and level (fp32)"""
    if not on.any():
        return (np.zeros(0, dtype=np.int64),) * 4 + (np.zeros(0, dtype=np.float32),)
    v, notes, starts, ends = _row_notes_host(n, on, int(min(max(o, -50), 50)), int(root) % 12, mask, h)
    L = ends - starts + 1
    prefix = np.cumsum(v)
    total = prefix[ends] - prefix[starts] + v[starts]
    pitch = notes[starts]
    detune = -((2 * (pitch * SEMITONE * L - total) + L) // (2 * L))        # minus tune_pitch's correction, ties included
    level = np.array([_NAN if loud is None else _level_host(loud[s:e + 1]) for s, e in zip(starts, ends)], dtype=np.float32)
    kept = L >= min_note
    return starts[kept], L[kept], pitch[kept], detune[kept], level[kept]


def _render_row_host(onset, frames, pitch, detune, level, n, o, T, keep, concert, transpose, glide, attack, release, floor, default,
                     depth, omega, delay, ramp):
    """-> position int64 [T], owner int32 [T], loudness fp64 [T]"""
    pos, owner, loud = np.full(T, HOLD, dtype=np.int64), np.full(T, -1, dtype=np.int32), np.full(T, floor, dtype=np.float64)
    if n == 0:
        return pos, owner, loud
    onset, frames, pitch, detune = (x[:n].astype(np.int64) for x in (onset, frames, pitch, detune))
    level = level[:n]
    valid = (frames >= 1) & (pitch >= 0) & (pitch <= 127) & (np.abs(detune) <= MAX_DETUNE)
    centre = pitch * SEMITONE + (detune if keep else 0) + (0 if concert else 65536 * int(min(max(o, -50), 50))) + transpose
    t = np.arange(T, dtype=np.int64)
    star = np.searchsorted(onset, t, side="right") - 1                          # i*, -1 before every onset
    i = np.maximum(star, 0)
    has = (star >= 0) & valid[i]
    pos = np.where(has, centre[i], np.where((star < 0) & valid[0], centre[0], HOLD))
    k = t - onset[i]
    on = has & (k < frames[i])
    owner = np.where(on, star, -1).astype(np.int32)
    if glide > 0:
        prev = np.maximum(i - 1, 0)
        slides = on & (k < glide) & (i > 0) & valid[prev] & (onset[i] <= onset[prev] + frames[prev])
        a = (centre[prev] - centre[i]) * (glide - k)
        pos = pos + np.where(slides, (2 * a + (glide + 1)) // (2 * (glide + 1)), 0)
    if depth > 0.0:
        sways = on & (k >= delay)
        ks = np.where(sways, k - delay, 0).astype(np.float64)
        pos = pos + np.where(sways, np.rint(depth * np.minimum(1.0, (ks + 1.0) / float(ramp)) * np.sin(omega * ks)).astype(np.int64), 0)
    nxt = np.minimum(i + 1, n - 1)
    length = np.where(i + 1 < n, np.minimum(frames[i], onset[nxt] - onset[i]), frames[i])
    lv = np.where(np.isnan(level[i]), np.float64(default), level[i].astype(np.float64))
    ga = np.minimum(1.0, (k + 1).astype(np.float64) / float(attack)) if attack > 0 else 1.0
    gr = np.minimum(1.0, (length - k).astype(np.float64) / float(release)) if release > 0 else 1.0
    loud = np.where(on, floor + (lv - floor) * ga * gr, floor)
    return pos, owner, loud


def _expression_row_host(cents, onset, frames, pitch, detune, n, o):
    """-> bend int32 [T], owner int32 [T] of one row"""
    T = cents.shape[0]
    if n == 0:
        return np.zeros(T, dtype=np.int32), np.full(T, -1, dtype=np.int32)
    onset, frames, pitch, detune = (x[:n].astype(np.int64) for x in (onset, frames, pitch, detune))
    valid = (frames >= 1) & (pitch >= 0) & (pitch <= 127) & (np.abs(detune) <= MAX_DETUNE)
    t = np.arange(T, dtype=np.int64)
    star = np.searchsorted(onset, t, side="right") - 1
    i = np.maximum(star, 0)
    with np.errstate(all="ignore"):
        own = (star >= 0) & valid[i] & (t - onset[i] < frames[i]) & (np.abs(cents) <= LIMIT)
    bend = _positions_host(cents, own) - 65536 * int(min(max(o, -50), 50)) - pitch[i] * SEMITONE - detune[i]
    bend = np.clip(bend, -(1 << 31), (1 << 31) - 1)                        # (records that do not match the track)
    return np.where(own, bend, 0).astype(np.int32), np.where(own, star, -1).astype(np.int32)


def _time_map_host(k, length, Ls, keep_attack, keep_release):
    """Destination frame k of a note that sounds `length` frames -> (q, f), the position in its source note of Ls frames, f in
    2^-16 frame; int64 arrays with 0 <= k < length and Ls >= 1."""
    a = np.minimum(np.minimum(keep_attack, Ls), length)
    r = np.minimum(np.minimum(keep_release, Ls - a), length - a)
    middle = (k >= a) & (k < length - r)
    D = np.where(middle, length - a - r + 1, 1)
    x = np.where(middle, (k - a + 1) * (Ls - a - r + 1), 0)
    q = np.where(k < a, k, np.where(middle, a - 1 + x // D, Ls - (length - k)))
    f = ((x % D) << 16) // D
    ends = (q < 0) | (q >= Ls - 1)
    return np.clip(q, 0, Ls - 1), np.where(ends, 0, f)


def _express_row_host(pos, owner, loud, onset, frames, n, source, src_onset, src_frames, src_level, n_src, bend, src_loud, bend_amount,
                      dyn_amount, keep_attack, keep_release):
    """One row of the plain render (position int64, owner, loudness fp64 [T]) -> position and loudness with the source's curves"""
    on = owner >= 0
    if n == 0 or n_src == 0 or not on.any():
        return pos, loud
    Tsrc = bend.shape[0]
    onset, frames = onset[:n].astype(np.int64), frames[:n].astype(np.int64)
    i = np.maximum(owner, 0).astype(np.int64)
    k = np.arange(pos.shape[0], dtype=np.int64) - onset[i]
    nxt = np.minimum(i + 1, n - 1)
    length = np.where(i + 1 < n, np.minimum(frames[i], onset[nxt] - onset[i]), frames[i])       # L'
    j = i if source is None else source[i].astype(np.int64)
    ok = on & (k < length) & (j >= 0) & (j < n_src)
    j = np.where(ok, j, 0)
    Ls, so = src_frames[j].astype(np.int64), src_onset[j].astype(np.int64)
    ok &= (Ls >= 1) & (so >= 0) & (so + Ls <= Tsrc)
    Ls, so = np.where(ok, Ls, 1), np.where(ok, so, 0)
    q, f = _time_map_host(np.where(ok, k, 0), np.where(ok, length, 1), Ls, keep_attack, keep_release)
    at = so + q
    nxt = np.minimum(at + 1, Tsrc - 1)                                      # (read only where f > 0: inside the source note)
    b = bend[at].astype(np.int64)
    b = b + np.where(f > 0, ((bend[nxt].astype(np.int64) - b) * f + 32768) >> 16, 0)
    pos = pos + np.where(ok, np.rint(bend_amount * b.astype(np.float64)).astype(np.int64), 0)
    if src_loud is not None and dyn_amount != 0.0:
        with np.errstate(all="ignore"):
            sl = src_level[j].astype(np.float64)
            l = src_loud[at].astype(np.float64)
            l = np.where(f > 0, l + (src_loud[nxt].astype(np.float64) - l) * (f.astype(np.float64) / 65536.0), l)
            loud = np.where(ok & ~np.isnan(sl), loud + dyn_amount * (l - sl), loud)
    return pos, loud


# ------------------------------------------------------------------------------------------------------------------ the calls
def _count(x, name, what, least=0, most=None):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < least or (most is not None and x >= most):
        raise ValueError(f"{what}: {name} must be an int of at least {least}" + (f" and below {most}" if most else "") + f", got {x!r}")
    return int(x)


def extract_notes(z: dict, tuning=None, scale=None, root=None, hysteresis: float = 20.0, min_note_frames: int = 0, max_notes=None) -> Notes:
    """The notes of the controls `z` (normalized_cents as [B, T, 1]; a dict with only f0 has its normalized_cents derived in
    fp64 first; harmonicity, loudness and voiced where the dict has them) as records: -> Notes with N = `max_notes` slots per row.

    The notes are `tune_pitch`'s, found the same way: tuning=None measures each row of z itself (with `scale` -- 'major' when
    None -- and `root`); a given `tuning` (G = 1 or B) is used as is, with its note-on options, `scale` and `root` overriding
    its own: one launch.  A note is a maximal run of on frames with one note; notes shorter than `min_note_frames` are dropped.
    `detune` is the note's mean above its pitch on the performance's own grid -- minus the correction `tune_pitch` gives the
    note with vibrato=True --, `level` its largest loudness.  max_notes=None takes T // max(1, min_note_frames), which cannot
    overflow; with a smaller N, `count` still counts every note and nothing is written past N (Notes.validate() tells)."""
    what = "extract_notes"
    if tuning is not None and not isinstance(tuning, TuningStatistics):
        raise ValueError(f"{what}: tuning must be a TuningStatistics or None, got {type(tuning).__name__}")
    forced = _root(root, what)
    mask = scale_mask(scale, what) if scale is not None else (tuning.mask if tuning is not None else SCALES["major"])
    scale_out = scale if scale is not None else (tuning.scale if tuning is not None else "major")
    min_note_frames = _count(min_note_frames, "min_note_frames", what)
    if isinstance(hysteresis, bool) or not isinstance(hysteresis, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(hysteresis) <= MAX_HYSTERESIS:
        raise ValueError(f"{what}: hysteresis must be 0 .. {MAX_HYSTERESIS:g} cents, got {hysteresis!r}")
    h_units = int(round(float(hysteresis) * 65536.0))
    silence, confidence = (tuning.silence, tuning.confidence) if tuning is not None else (None, 0.0)
    silence, confidence = _gates(silence, confidence, what)
    n, _, h, gate, voiced = _inputs(z, what, None, silence, False)
    B, T = n.shape[:2]
    loud = z.get("loudness")
    if loud is not None:
        if loud.shape != n.shape or loud.device != n.device:
            raise ValueError(f"{what}: loudness is {tuple(loud.shape)} on {loud.device}, the pitch {tuple(n.shape)} on {n.device}")
        _refuse_grad(loud, what)
    N = T // max(1, min_note_frames) if max_notes is None else _count(max_notes, "max_notes", what)
    if T >= 1 << 24 or B * T >= 1 << 31 or B * N >= 1 << 31:
        raise ValueError(f"{what}: {B} x {T} frames, {N} slots: a row takes fewer than 2^24 frames, a call fewer than 2^31 frames and slots")
    if tuning is None:
        stats_z = dict(z, normalized_cents=n) if "normalized_cents" not in z else z
        tuning = tuning_statistics(stats_z, per_row=True, scale=mask, root=root)
    if tuning.groups not in (1, B):
        raise ValueError(f"{what}: tuning has {tuning.groups} groups, the batch {B} rows: expected 1 or {B}")
    if tuning.device != n.device:
        raise ValueError(f"{what}: tuning is on {tuning.device}, the controls on {n.device}: move it once with .to()")
    root_info = tuning.root if forced < 0 else torch.full_like(tuning.root, forced)
    opts = dict(offset=tuning.offset, root=root_info, scale=scale_out, source_frames=T, silence=silence, confidence=confidence)
    if n.is_cuda:
        dev = n.device
        L = _lib.lib()
        nc = n.detach().float().contiguous()
        hc = h.detach().float().contiguous() if h is not None else None
        lc = loud.detach().float().contiguous() if loud is not None else None
        vc = voiced.contiguous().view(torch.uint8) if voiced is not None else None
        rec = torch.empty((4, B, N), device=dev, dtype=torch.int32)
        level = torch.empty((B, N), device=dev, dtype=torch.float32)
        count = torch.empty(B, device=dev, dtype=torch.int32)
        ptr = lambda x: x.data_ptr() if x is not None else None            # noqa: E731
        with torch.cuda.device(dev):
            rc = L.ddsp_notes_extract(nc.data_ptr(), ptr(hc), ptr(lc), ptr(vc), tuning.offset.data_ptr(), tuning.root.data_ptr(),
                                      rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), rec[3].data_ptr(), level.data_ptr(),
                                      count.data_ptr(), B, T, N, tuning.groups, mask, forced, h_units, min_note_frames,
                                      1 if gate is not None else 0, 0.0 if silence is None else silence, confidence,
                                      torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_notes_extract")
        return Notes(rec[0], rec[1], rec[2], rec[3], level, count, **opts)
    flat = lambda x: None if x is None else x.detach().float().numpy().reshape(B, T)       # noqa: E731
    nn_, ln = flat(n), flat(loud)
    on = _on_host(nn_, flat(h), flat(gate), None if voiced is None else voiced.numpy().reshape(B, T), silence, confidence)
    offs, roots = tuning.offset.numpy(), root_info.numpy()
    rec = np.zeros((4, B, N), dtype=np.int32)
    rec[0], rec[2] = -1, NO_PITCH
    level, count = np.full((B, N), _NAN, dtype=np.float32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        g = b if tuning.groups > 1 else 0
        s, L_, p, d, lv = _extract_row_host(nn_[b], on[b], None if ln is None else ln[b], offs[g], roots[g], mask, h_units, min_note_frames)
        count[b] = len(s)
        m = min(len(s), N)
        rec[0, b, :m], rec[1, b, :m], rec[2, b, :m], rec[3, b, :m], level[b, :m] = s[:m], L_[:m], p[:m], d[:m], lv[:m]
    return Notes(*(torch.from_numpy(rec[i]) for i in range(4)), torch.from_numpy(level), torch.from_numpy(count), **opts)


def note_expression(z: dict, notes: Notes, return_owner: bool = False) -> Expression:
    """The expression of the performance `z` (the controls `extract_notes` reads) under the notes found on it: -> Expression.
    A frame belongs to the note that owns it in `render_notes`' sense (the last note that began at or before it, valid, not yet
    over) where its normalized_cents lies within +-4; its `bend` is its position minus the note's centre on the performance's own
    grid, pitch S + detune + 65536 offset, so that rendering the unedited notes with the expression returns every position to
    the bit.  The loudness track, where z has one, is copied.  Records that do not match z give defined values.  One launch."""
    what = "note_expression"
    if not isinstance(notes, Notes):
        raise ValueError(f"{what}: notes must be a Notes, got {type(notes).__name__}")
    n, _, _, _, _ = _inputs(z, what, None, None, False)
    B, T = n.shape[:2]
    N = notes.max_notes
    if notes.rows != B:
        raise ValueError(f"{what}: the notes have {notes.rows} rows, the controls {B}")
    if notes.device != n.device:
        raise ValueError(f"{what}: the notes are on {notes.device}, the controls on {n.device}: move them once with .to()")
    loud = z.get("loudness")
    if loud is not None:
        if loud.shape != n.shape or loud.device != n.device:
            raise ValueError(f"{what}: loudness is {tuple(loud.shape)} on {loud.device}, the pitch {tuple(n.shape)} on {n.device}")
        _refuse_grad(loud, what)
        loud = loud.detach().float().reshape(B, T).clone()
    if T >= 1 << 24 or B * T >= 1 << 31 or B * N >= 1 << 31:
        raise ValueError(f"{what}: {B} x {T} frames, {N} slots: a row takes fewer than 2^24 frames, a call fewer than 2^31 frames and slots")
    if n.is_cuda:
        dev = n.device
        L = _lib.lib()
        nc = n.detach().float().contiguous()
        bend = torch.empty((B, T), device=dev, dtype=torch.int32)
        owner = torch.empty((B, T), device=dev, dtype=torch.int32) if return_owner else None
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        with torch.cuda.device(dev):
            rc = L.ddsp_notes_expression(nc.data_ptr(), ptr(notes.onset), ptr(notes.frames), ptr(notes.pitch), ptr(notes.detune),
                                         notes.count.data_ptr(), notes.offset.data_ptr(), bend.data_ptr(), ptr(owner), B, T, N, notes.groups,
                                         torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_notes_expression")
        return Expression(bend, loud, notes.onset.clone(), notes.frames.clone(), notes.level.clone(), notes.count.clone(), owner)
    rec = [getattr(notes, k).numpy() for k in ("onset", "frames", "pitch", "detune")]
    counts, offs = notes.count.numpy(), notes.offset.numpy()
    cents = n.detach().float().numpy().reshape(B, T)
    rows = [_expression_row_host(cents[b], *(x[b] for x in rec), min(max(int(counts[b]), 0), N), offs[b if notes.groups > 1 else 0])
            for b in range(B)]
    return Expression(torch.from_numpy(np.stack([r[0] for r in rows])), loud, notes.onset.clone(), notes.frames.clone(), notes.level.clone(),
                      notes.count.clone(), torch.from_numpy(np.stack([r[1] for r in rows])) if return_owner else None)


def render_notes(notes: Notes, frames: int, sample_rate: int, hop_length: int, detune: bool = True, concert: bool = False,
                 transpose: float = 0.0, glide: int = 0, attack: int = 0, release: int = 0, floor: float = 0.0, default_level: float = 1.0,
                 vibrato_cents: float = 0.0, vibrato_hz: float = 5.5, vibrato_delay: int = 0, vibrato_ramp: int = 1,
                 return_info: bool = False, expression=None, source=None, bend_amount: float = 1.0, dynamics_amount: float = 1.0,
                 keep_attack: int = 0, keep_release: int = 0) -> dict:
    """Note events -> `frames` frames of controls: a dict with f0, normalized_cents, loudness, harmonicity (fp32 [B, T, 1]) and
    voiced (bool [B, T, 1]); return_info=True adds position (int64 [B, T], units of 2^-16 cent on the MIDI scale) and owner
    (int32 [B, T]: the note a frame belongs to, -1 for none).

    The instrument is monophonic: a frame belongs to the last note that began at or before it, so a later note cuts an earlier
    one off; onsets are expected in order (Notes.sorted()).  A note with frames < 1, a pitch outside 0 .. 127 or |detune| beyond
    2^30 units sounds nowhere.  A note sounds at its pitch on the performance's own grid (A440 plus the notes' offset;
    concert=True: A440's grid), plus its `detune` unless detune=False, plus `transpose` semitones.  `glide` frames of
    portamento lead from the previous note where the two touch; vibrato of `vibrato_cents` at `vibrato_hz` starts
    `vibrato_delay` frames into a note and swells over `vibrato_ramp` frames.  Off frames hold the pitch of the note before
    them.  Loudness is the note's level (`default_level` where that is NaN) over `floor`, with `attack` and `release` frames of
    linear ramp at the note's ends; off frames are at `floor`.  harmonicity is 1 on and 0 off.  One launch.

    `expression` (an Expression from `note_expression`, on the notes' device and with as many rows) gives the notes their
    performer's curves back: note i reads the curve of the expression's note `source[i]` (`source` int32
    [B, N]; None: note i itself -- right after any edit that keeps the slots, such as transpose, quantize or moved onsets; after
    `sorted(return_order=True)` pass the order), stretched linearly to the note's sounding length with the first `keep_attack`
    and the last `keep_release` frames kept one to one.  The pitch gains `bend_amount` times the curve's bend, the loudness
    `dynamics_amount` times the curve's loudness above the source note's level, on top of everything above.  A note without a
    valid source is rendered as without an expression; expression=None is the call as it always was."""
    what = "render_notes"
    if not isinstance(notes, Notes):
        raise ValueError(f"{what}: notes must be a Notes, got {type(notes).__name__}")
    _refuse_grad(notes.level, what)
    T = _count(frames, "frames", what, 1)
    sample_rate, hop_length = _count(sample_rate, "sample_rate", what, 1), _count(hop_length, "hop_length", what, 1)
    glide, attack, release = (_count(x, k, what, 0, MAX_STEPS) for k, x in (("glide", glide), ("attack", attack), ("release", release)))
    delay, ramp = _count(vibrato_delay, "vibrato_delay", what, 0, MAX_STEPS), _count(vibrato_ramp, "vibrato_ramp", what, 1, MAX_STEPS)
    if not abs(float(transpose)) <= MAX_TRANSPOSE:
        raise ValueError(f"{what}: transpose must lie within +-{MAX_TRANSPOSE:g} semitones, got {transpose!r}")
    if not 0.0 <= float(vibrato_cents) <= 100.0 * MAX_TRANSPOSE or not 0.0 <= float(vibrato_hz) <= float(sample_rate):
        raise ValueError(f"{what}: vibrato_cents must be 0 .. {100 * MAX_TRANSPOSE:g} and vibrato_hz 0 .. the sample rate")
    floor, default_level = float(np.float32(floor)), float(np.float32(default_level))
    if not (math.isfinite(floor) and math.isfinite(default_level)):
        raise ValueError(f"{what}: floor and default_level must be finite")
    B, N = notes.rows, notes.max_notes
    if T >= 1 << 24 or B * T >= 1 << 31 or B * N >= 1 << 31:
        raise ValueError(f"{what}: {B} x {T} frames, {N} slots: a row takes fewer than 2^24 frames, a call fewer than 2^31 frames and slots")
    units = int(round(float(transpose) * SEMITONE))
    depth = float(vibrato_cents) * 65536.0
    omega = 2.0 * math.pi * (float(vibrato_hz) * hop_length / sample_rate)
    flags = (_KEEP_DETUNE if detune else 0) | (_CONCERT if concert else 0)
    e = expression
    if e is None:
        if source is not None:
            raise ValueError(f"{what}: source names the notes of an expression; none is given")
    else:
        if not isinstance(e, Expression):
            raise ValueError(f"{what}: expression must be an Expression or None, got {type(e).__name__}")
        if e.rows != B:
            raise ValueError(f"{what}: the expression has {e.rows} rows, the notes {B}")
        if e.device != notes.device:
            raise ValueError(f"{what}: the expression is on {e.device}, the notes on {notes.device}: move it once with .to()")
        if source is not None:
            source = torch.as_tensor(source, dtype=torch.int32, device=notes.device).contiguous()
            if source.shape != (B, N):
                raise ValueError(f"{what}: source must be [{B}, {N}] (one source note per note), got {tuple(source.shape)}")
        keep_attack, keep_release = (_count(x, k, what, 0, MAX_STEPS) for k, x in (("keep_attack", keep_attack), ("keep_release", keep_release)))
        bend_amount, dynamics_amount = float(bend_amount), float(dynamics_amount)
        if not (abs(bend_amount) <= MAX_AMOUNT and abs(dynamics_amount) <= MAX_AMOUNT):
            raise ValueError(f"{what}: bend_amount and dynamics_amount must be finite and within +-{MAX_AMOUNT:g}")
        Ts, Ns = e.source_frames, e.max_notes
        if Ts >= 1 << 24 or B * Ts >= 1 << 31 or B * Ns >= 1 << 31:
            raise ValueError(f"{what}: an expression of {B} x {Ts} frames, {Ns} slots: a row takes fewer than 2^24 frames, a call fewer "
                             "than 2^31 frames and slots")
    if notes.onset.is_cuda:
        dev = notes.device
        L = _lib.lib()
        out = torch.empty((4, B, T, 1), device=dev, dtype=torch.float32)
        voiced = torch.empty((B, T, 1), device=dev, dtype=torch.bool)
        position = torch.empty((B, T), device=dev, dtype=torch.int64) if return_info else None
        owner = torch.empty((B, T), device=dev, dtype=torch.int32) if return_info else None
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        args = (ptr(notes.onset), ptr(notes.frames), ptr(notes.pitch), ptr(notes.detune), ptr(notes.level), notes.count.data_ptr(),
                notes.offset.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), voiced.data_ptr(),
                ptr(position), ptr(owner), B, T, N, notes.groups, flags, units, glide, attack, release, delay, ramp, depth, omega, floor,
                default_level)
        with torch.cuda.device(dev):
            if e is None:
                rc = L.ddsp_notes_render(*args, torch.cuda.current_stream().cuda_stream)
            else:
                rc = L.ddsp_notes_render_expr(*args, ptr(source), ptr(e.onset), ptr(e.frames), ptr(e.level), e.count.data_ptr(),
                                              e.bend.data_ptr(), ptr(e.loudness), Ts, Ns, bend_amount, dynamics_amount, keep_attack,
                                              keep_release, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_notes_render" if e is None else "ddsp_notes_render_expr")
        z = dict(f0=out[0], normalized_cents=out[1], loudness=out[2], harmonicity=out[3], voiced=voiced)
        return dict(z, position=position, owner=owner) if return_info else z
    rec = [getattr(notes, k).numpy() for k in ("onset", "frames", "pitch", "detune", "level")]
    counts, offs = notes.count.numpy(), notes.offset.numpy()
    rows = [_render_row_host(*(x[b] for x in rec), min(max(int(counts[b]), 0), N), offs[b if notes.groups > 1 else 0], T, bool(detune),
                             bool(concert), units, glide, attack, release, floor, default_level, depth, omega, delay, ramp) for b in range(B)]
    if e is not None:
        src = None if source is None else source.numpy()
        so, sf, sl, sc, bend = (x.numpy() for x in (e.onset, e.frames, e.level, e.count, e.bend))
        sloud = None if e.loudness is None else e.loudness.numpy()
        for b in range(B):
            pos, loud = _express_row_host(rows[b][0], rows[b][1], rows[b][2], rec[0][b], rec[1][b], min(max(int(counts[b]), 0), N),
                                          None if src is None else src[b], so[b], sf[b], sl[b], min(max(int(sc[b]), 0), Ns), bend[b],
                                          None if sloud is None else sloud[b], bend_amount, dynamics_amount, keep_attack, keep_release)
            rows[b] = (pos, rows[b][1], loud)
    position = np.stack([r[0] for r in rows])
    owner = np.stack([r[1] for r in rows])
    c = position.astype(np.float64) / 65536.0
    on = owner >= 0
    with np.errstate(all="ignore"):
        z = dict(f0=(440.0 * np.exp2((c - 6900.0) / 1200.0)).astype(np.float32), normalized_cents=((c - ORIGIN) / 7180.0).astype(np.float32),
                 loudness=np.stack([r[2] for r in rows]).astype(np.float32), harmonicity=on.astype(np.float32), voiced=on)
    z = {k: torch.from_numpy(np.ascontiguousarray(v)).reshape(B, T, 1) for k, v in z.items()}
    return dict(z, position=torch.from_numpy(position), owner=torch.from_numpy(owner)) if return_info else z
