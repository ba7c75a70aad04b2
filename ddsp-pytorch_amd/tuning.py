"""Auto-tune: tuning statistics and scale-aware pitch snapping (csrc/ddsp_tuning.hip).

The last step of the timbre-transfer chain (octave shift -> loudness match -> auto-tune): `tuning_statistics` measures how a
performance is tuned -- its offset from A440 equal temperament in whole cents, and its key --, and `tune_pitch` moves its notes
onto a scale while keeping what makes it a performance: every frame of a note gets the same correction, so the note's centre
lands on the pitch and its vibrato and inflection stay.

  TuningStatistics      offset [G] int32 cents, root [G] int32, profile [G, 12] int64, frames [G] int64, the scale and the
                        note-on options; to_dict() / from_dict(), .to(device); constructible by hand
  tuning_statistics     a dict with normalized_cents [R, T, 1] (and harmonicity, loudness, voiced) -> TuningStatistics
  tune_pitch            a control dict -> the dict with f0 and normalized_cents moved onto the scale

Everything is defined in integer arithmetic on positions of 2^-16 cent (include/ddsp_hip.h has the text): CUDA tensors run
the three kernels of csrc/ddsp_tuning.hip, CPU tensors the same definition as numpy operations, to the same bits
(tests/tuning_reference.py has it as plain loops)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .encoder import _refuse_grad

CELLS = 1200                                                    # DDSP_TUNING_CELLS
LDS_FRAMES = 1536                                               # DDSP_TUNING_LDS_FRAMES
SEMITONE = 100 * 65536
OCTAVE = 12 * SEMITONE
ORIGIN = 2346.0614660728625                                     # 1997.3794084376191 - 1200 log2(44) + 6900
LIMIT = np.float32(4.0)                                         # |normalized_cents| beyond it is not on
MAX_GROUP_FRAMES = 1 << 24
MAX_HYSTERESIS = 1200.0                                         # cents
OFF = -(1 << 31)                                                # `notes` of an off frame
SCALES = dict(chromatic=0xFFF, major=0xAB5, minor=0x5AD, pentatonic=0x295)
_VIBRATO, _CONCERT = 1, 2


def scale_mask(scale, what="scale_mask") -> int:
    """A scale's name, or 12 bits (bit i: the degree i semitones above the root is allowed) -> the bits."""
    if isinstance(scale, str):
        if scale not in SCALES:
            raise ValueError(f"{what}: unknown scale {scale!r}; one of {sorted(SCALES)} or a 12-bit mask")
        return SCALES[scale]
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= int(scale) <= 0xFFF:
        raise ValueError(f"{what}: a scale is a name or a mask in 1 .. 0xFFF, got {scale!r}")
    return int(scale)


def _root(root, what):
    if root is None:
        return -1
    if isinstance(root, bool) or not isinstance(root, (int, np.integer)) or not 0 <= int(root) <= 11:
        raise ValueError(f"{what}: root must be None or a pitch class 0 .. 11, got {root!r}")
    return int(root)


class TuningStatistics:
    """What `tuning_statistics` measured, or values set by hand: `offset` [G] int32 (whole cents the performance lies above
    A440 equal temperament, -50 .. 49), `root` [G] int32 (pitch class 0 .. 11, C = 0), `profile` [G, 12] int64 (on frames per
    pitch class, around the offset grid), `frames` [G] int64, `scale` (a name or a 12-bit mask) and the note-on options
    `silence` and `confidence`.  G = 1 for pooled statistics, else one group per row."""

    def __init__(self, offset, root, profile=None, frames=None, scale="major", silence=None, confidence: float = 0.0):
        by_hand = not isinstance(offset, torch.Tensor)
        self.offset = torch.as_tensor(offset, dtype=torch.int32).reshape(-1).contiguous()
        dev, G = self.offset.device, self.offset.shape[0]
        self.root = torch.as_tensor(root, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        if G < 1 or self.root.shape[0] != G:
            raise ValueError(f"TuningStatistics: offset and root must hold the same number (>= 1) of values, got {G} and {self.root.shape[0]}")
        if by_hand and not (bool((self.offset.abs() <= 50).all()) and bool(((self.root >= 0) & (self.root <= 11)).all())):
            raise ValueError("TuningStatistics: an offset lies within +-50 cents, a root in 0 .. 11")
        if profile is None:
            profile = torch.zeros((G, 12), dtype=torch.int64, device=dev)
        self.profile = torch.as_tensor(profile, dtype=torch.int64, device=dev).reshape(-1, 12).contiguous()
        if frames is None:
            frames = torch.zeros(G, dtype=torch.int64, device=dev)
        self.frames = torch.as_tensor(frames, dtype=torch.int64, device=dev).reshape(-1).contiguous()
        if self.profile.shape[0] != G or self.frames.shape[0] != G:
            raise ValueError(f"TuningStatistics: profile must be [{G}, 12] and frames [{G}]")
        self.mask = scale_mask(scale, "TuningStatistics")
        self.scale = scale if isinstance(scale, str) else int(scale)
        self.silence = None if silence is None else float(silence)
        self.confidence = float(confidence)

    @property
    def groups(self) -> int:
        return self.offset.shape[0]

    @property
    def device(self):
        return self.offset.device

    def options(self) -> dict:
        return dict(scale=self.scale, silence=self.silence, confidence=self.confidence)

    def to(self, device) -> "TuningStatistics":
        return TuningStatistics(self.offset.to(device), self.root.to(device), self.profile.to(device), self.frames.to(device),
                                **self.options())

    def to_dict(self) -> dict:
        """Plain tensors (on the CPU), the scale and floats."""
        return dict(offset=self.offset.cpu(), root=self.root.cpu(), profile=self.profile.cpu(), frames=self.frames.cpu(), **self.options())

    @classmethod
    def from_dict(cls, d: dict) -> "TuningStatistics":
        return cls(d["offset"], d["root"], d["profile"], d["frames"], scale=d["scale"], silence=d["silence"], confidence=d["confidence"])


def _cents_of_f0(f0: torch.Tensor) -> torch.Tensor:
    """normalized_cents of a frequency track, formed in fp64 and rounded once (a dict that has only f0)"""
    return ((1200.0 * torch.log2(f0.detach().double() / 10.0) - 1997.3794084376191) / 7180.0).float()


def _inputs(z, what, voiced, silence, need_f0):
    """the [R, T, 1] inputs of z: (cents, f0 or None, harmonicity or None, loudness or None, voiced or None)"""
    if "normalized_cents" in z:
        n = z["normalized_cents"]
    elif "f0" in z:
        n = None
    else:
        raise ValueError(f"{what}: the dict has neither 'normalized_cents' nor 'f0'")
    first = n if n is not None else z["f0"]
    if first.dim() != 3 or first.shape[-1] != 1 or first.shape[0] < 1 or first.shape[1] < 1:
        raise ValueError(f"{what}: the pitch must be [R, T, 1] with R, T >= 1, got {tuple(first.shape)}")

    def same(x, name):
        if x.shape != first.shape or x.device != first.device:
            raise ValueError(f"{what}: {name} is {tuple(x.shape)} on {x.device}, the pitch {tuple(first.shape)} on {first.device}")
        _refuse_grad(x, what)
        return x

    same(first, "the pitch")
    f0 = None
    if need_f0 or n is None:
        if "f0" not in z:
            raise ValueError(f"{what}: the dict has no 'f0'")
        f0 = same(z["f0"], "f0")
    if n is None:
        n = _cents_of_f0(f0)
    h = same(z["harmonicity"], "harmonicity") if "harmonicity" in z else None
    l = same(z["loudness"], "loudness") if silence is not None and "loudness" in z else None
    if voiced is None:
        voiced = z.get("voiced")
    if voiced is not None and (voiced.shape != first.shape or voiced.device != first.device or voiced.dtype != torch.bool):
        raise ValueError(f"{what}: voiced must be a bool tensor {tuple(first.shape)} on {first.device}")
    return n, f0, h, l, voiced


def _gates(silence, confidence, what):
    if silence is not None and np.isnan(np.float32(silence)) or np.isnan(np.float32(confidence)):
        raise ValueError(f"{what}: silence and confidence must not be NaN")
    return (None if silence is None else float(np.float32(silence))), float(np.float32(confidence))


# ------------------------------------------------------------------------------------------------------------------ the CPU path
def _on_host(n, h, l, v, silence, confidence):
    with np.errstate(all="ignore"):
        on = np.abs(n) <= LIMIT
        if h is not None:
            on &= h >= np.float32(confidence)
        if l is not None and silence is not None:
            on &= l > np.float32(silence)
        if v is not None:
            on &= v
    return on


def _positions_host(n, on):
    """int64 positions (0 where off): the product exact in fp64, one rounding in the sum, llrint"""
    x = np.where(on, n, np.float32(0)).astype(np.float64)
    return np.where(on, np.rint((7180.0 * x + ORIGIN) * 65536.0).astype(np.int64), 0)


_OFFSETS = np.array(sorted(range(-50, 50), key=lambda o: (abs(o), o < 0)), dtype=np.int64)      # the tie order
_DEVIATION = np.minimum((np.arange(100)[None] - _OFFSETS[:, None]) % 100, (_OFFSETS[:, None] - np.arange(100)[None]) % 100)


def _estimate_host(H, mask, forced_root):
    """H [G, 1200] int64 -> offset, root int32 [G], profile int64 [G, 12], frames int64 [G]"""
    G = H.shape[0]
    D = H.reshape(G, 12, 100).sum(axis=1)
    cost = D @ _DEVIATION.T                                                 # [G, 100] int64, exact
    offset = _OFFSETS[np.argmin(cost, axis=1)]                              # (the first minimum in the tie order)
    cells = (100 * np.arange(12)[None, :, None] + offset[:, None, None] + np.arange(-50, 50)[None, None, :]) % CELLS
    profile = np.take_along_axis(H, cells.reshape(G, -1), axis=1).reshape(G, 12, 100).sum(axis=2)
    if forced_root >= 0:
        root = np.full(G, forced_root, dtype=np.int64)
    else:
        allowed = (mask >> ((np.arange(12)[None] - np.arange(12)[:, None]) % 12)) & 1        # [r, p]
        root = np.argmax(profile @ allowed.T, axis=1)                       # (the first maximum: the smallest r)
    return offset.astype(np.int32), root.astype(np.int32), profile.astype(np.int64), H.sum(axis=1).astype(np.int64)


def _row_notes_host(n, on, o, root, mask, h):
    """One row with an on frame -> (v, notes, starts, ends): the positions relative to the row's own grid (0 where off), note_t
    (OFF where off), and the first and last frame of every note (notes.py reads the same four)"""
    T = n.shape[0]
    notes = np.full(T, OFF, dtype=np.int64)
    v = np.where(on, _positions_host(n, on) - 65536 * o, 0)
    c = v // SEMITONE
    rel = (c - root) % 12
    down = np.array([next(k for k in range(12) if (mask >> ((r - k) % 12)) & 1) for r in range(12)], dtype=np.int64)
    up = np.array([next(k for k in range(12) if (mask >> ((r + 1 + k) % 12)) & 1) for r in range(12)], dtype=np.int64)
    lo, hi = c - down[rel], c + 1 + up[rel]
    q = np.where(v - lo * SEMITONE <= hi * SEMITONE - v, lo, hi)
    before = np.concatenate([[False], on[:-1]])
    fresh = on & ~before
    reach = np.abs(v - q * SEMITONE) + h
    at, cur = 0, 0
    while at < T:                                                       # one turn per note change, as the kernel's ballot
        leaves = on[at:] & (fresh[at:] | (np.abs(v[at:] - cur * SEMITONE) > reach[at:]))
        if not leaves.any():
            notes[at:][on[at:]] = cur
            break
        first = at + int(np.argmax(leaves))
        notes[at:first][on[at:first]] = cur
        cur = int(q[first])
        notes[first] = cur
        at = first + 1
    starts = np.flatnonzero(on & (np.concatenate([[OFF], notes[:-1]]) != notes))
    ends = np.flatnonzero(on & (np.concatenate([notes[1:], [OFF]]) != notes))
    return v, notes, starts, ends


def _snap_row_host(n, f0, on, o, root, mask, h, min_note, glide, vibrato, concert, amount):
    T = n.shape[0]
    o = int(min(max(o, -50), 50))
    root = int(root) % 12
    shift = 65536 * o
    conc = shift if concert else 0
    notes, d = np.full(T, OFF, dtype=np.int64), np.zeros(T, dtype=np.int64)
    out_n, out_f = n.copy(), f0.copy()
    if on.any():
        v, notes, starts, ends = _row_notes_host(n, on, o, root, mask, h)
        before = np.concatenate([[False], on[:-1]])
        after = np.concatenate([on[1:], [False]])
        fresh = on & ~before
        L = ends - starts + 1
        prefix = np.cumsum(v)
        total = prefix[ends] - prefix[starts] + v[starts]
        kept = L >= min_note
        corr = np.zeros(T, dtype=np.int64)
        if vibrato:
            mean = (2 * (notes[starts] * SEMITONE * L - total) + L) // (2 * L) - conc
            corr[on] = np.repeat(np.where(kept, mean, 0), L)
        else:
            corr[on] = np.where(np.repeat(kept, L), notes[on] * SEMITONE - v[on] - conc, 0)
        run_first, run_last = np.flatnonzero(fresh), np.flatnonzero(on & ~after)
        lengths = run_last - run_first + 1
        t = np.flatnonzero(on)
        a = np.maximum(t - glide, np.repeat(run_first, lengths))
        b = np.minimum(t + glide, np.repeat(run_last, lengths))
        prefix = np.cumsum(corr)
        total, count = prefix[b] - prefix[a] + corr[a], b - a + 1
        smoothed = (2 * total + count) // (2 * count)
        mix = float(min(max(np.float32(amount), np.float32(0)), np.float32(1))) if amount == amount else 0.0
        d[t] = np.rint(mix * smoothed.astype(np.float64)).astype(np.int64)
        moved = d != 0
        with np.errstate(all="ignore"):
            out_n[moved] = n[moved] + (d[moved] / (65536.0 * 7180.0)).astype(np.float32)
            out_f[moved] = (f0[moved].astype(np.float64) * np.exp2(d[moved] / (65536.0 * 1200.0))).astype(np.float32)
    return notes.astype(np.int32), d.astype(np.int32), out_n, out_f


# ------------------------------------------------------------------------------------------------------------------ the calls
def tuning_statistics(z: dict, per_row: bool = False, scale="major", root=None, silence=None, confidence: float = 0.0, voiced=None,
                      return_histogram: bool = False):
    """How the on frames of `z` are tuned: any dict with `normalized_cents` [R, T, 1] (an Encoder's output, an analysis
    result; a dict with only `f0` has its normalized_cents derived in fp64 first).  Pooled (per_row=False) all rows make one
    statistic (G = 1); per_row=True gives one per row.

    A frame is on when |normalized_cents| <= 4, `voiced` (a bool [R, T, 1]; None: z['voiced'] where the dict has one) is
    true, harmonicity >= `confidence` where the dict has a harmonicity, and loudness > `silence` where `silence` is given and
    the dict has a loudness.  The defaults count every frame in range; they are not tuned here.

    The on frames are counted in 1200 one-cent pitch-class cells; `offset` is the circular median of their deviations from
    the semitone grid (whole cents, -50 .. 49), `profile` the frames per pitch class around that grid, `root` the rotation
    of `scale` (a name -- chromatic, major, minor, pentatonic -- or a 12-bit mask) that covers the most frames, or the
    `root` given.  Only integers are accumulated: the same bits for any order of the rows, and from run to run.  One
    statistic takes at most 2^24 frames, a call fewer than 2^32.  A statistic without an on frame has offset 0, root 0.

    -> TuningStatistics; with return_histogram=True, (statistics, counts [G, 1200] int64).
    On the device: one statistics launch (behind one memset when pooled) and one estimate launch, no host synchronisation."""
    what = "tuning_statistics"
    mask, forced = scale_mask(scale, what), _root(root, what)
    silence, confidence = _gates(silence, confidence, what)
    n, _, h, l, voiced = _inputs(z, what, voiced, silence, False)
    R, T = n.shape[:2]
    if R * T >= 1 << 32 or (T if per_row else R * T) > MAX_GROUP_FRAMES:
        raise ValueError(f"{what}: {R} x {T} frames: one statistic takes at most 2^24 frames, a call fewer than 2^32")
    G = R if per_row else 1
    opts = dict(scale=scale, silence=silence, confidence=confidence)
    if n.is_cuda:
        dev = n.device
        L = _lib.lib()
        nc = n.detach().float().contiguous()
        hc = h.detach().float().contiguous() if h is not None else None
        lc = l.detach().float().contiguous() if l is not None else None
        vc = voiced.contiguous().view(torch.uint8) if voiced is not None else None
        accum = torch.empty(L.ddsp_tuning_accum_bytes(G) // 4, device=dev, dtype=torch.int32)
        offset, root_out = torch.empty(G, device=dev, dtype=torch.int32), torch.empty(G, device=dev, dtype=torch.int32)
        profile, frames = torch.empty((G, 12), device=dev, dtype=torch.int64), torch.empty(G, device=dev, dtype=torch.int64)
        ptr = lambda x: x.data_ptr() if x is not None else None            # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            rc = L.ddsp_tuning_stats(nc.data_ptr(), ptr(hc), ptr(lc), ptr(vc), accum.data_ptr(), R, T, 0 if per_row else 1,
                                     0.0 if silence is None else silence, confidence, stream)
            _lib.check(rc, "ddsp_tuning_stats")
            rc = L.ddsp_tuning_estimate(accum.data_ptr(), offset.data_ptr(), root_out.data_ptr(), profile.data_ptr(), frames.data_ptr(),
                                        G, mask, forced, stream)
            _lib.check(rc, "ddsp_tuning_estimate")
        stats = TuningStatistics(offset, root_out, profile, frames, **opts)
        return (stats, accum.view(G, CELLS).to(torch.int64) & 0xFFFFFFFF) if return_histogram else stats
    flat = lambda x: None if x is None else x.detach().float().numpy().reshape(R, T)       # noqa: E731
    nn_ = flat(n)
    on = _on_host(nn_, flat(h), flat(l), None if voiced is None else voiced.numpy().reshape(R, T), silence, confidence)
    cell = ((_positions_host(nn_, on) + 32768) % OCTAVE) // 65536
    groups = [slice(r, r + 1) for r in range(R)] if per_row else [slice(None)]
    H = np.stack([np.bincount(cell[g][on[g]], minlength=CELLS) for g in groups]).astype(np.int64)
    offset, root_out, profile, frames = _estimate_host(H, mask, forced)
    stats = TuningStatistics(torch.from_numpy(offset), torch.from_numpy(root_out), torch.from_numpy(profile), torch.from_numpy(frames),
                             **opts)
    return (stats, torch.from_numpy(H)) if return_histogram else stats


def tune_pitch(z: dict, tuning=None, amount=1.0, scale=None, root=None, hysteresis: float = 20.0, min_note_frames: int = 0,
               glide: int = 0, vibrato: bool = True, concert: bool = False, return_info: bool = False):
    """Move the notes of the controls `z` (f0 and normalized_cents as [B, T, 1]; a dict with only f0 has its normalized_cents
    derived in fp64 first) onto a scale: -> a new dict with `f0` and `normalized_cents` replaced, every other key the same
    object.

    tuning=None measures each row of z itself (`tuning_statistics(z, per_row=True)` with `scale` -- 'major' when None -- and
    `root`): three launches.  A given `tuning` (G = 1 or B) is used as is, with its note-on options; `scale` and `root`
    (None: the tuning's own) override its scale and root: one launch, no host synchronisation, no allocation after the
    outputs, so the call can be captured in a graph.

    With v the frame's position relative to the performance's own grid (A440 plus the offset), every on frame takes the
    nearest allowed note, but stays on the previous frame's note while that is no more than `hysteresis` cents (0 .. 1200)
    farther than the nearest.  A note -- a run of on frames with one note -- of at least `min_note_frames` frames is
    corrected: with vibrato=True every frame by the same amount, which moves the note's mean onto the pitch and keeps its
    vibrato and inflection; with vibrato=False every frame onto the pitch (the hard snap).  concert=True lands on A440's grid
    instead of the performance's own.  The corrections are averaged over `glide` frames either side within a run of on
    frames, and scaled by `amount` (0 .. 1; a float, or a tensor with one value per row).  Frames that are off, or whose
    correction is 0, return f0 and normalized_cents bit for bit.  The defaults -- hysteresis 20 cents, no minimum length, no
    glide -- are not tuned by ear here.

    return_info=True adds a dict of `notes` [B, T] int32 (MIDI notes; INT32_MIN where off), `correction_cents` [B, T] fp64,
    `correction` [B, T] int32 (units of 2^-16 cent), `offset` and `root` [G] int32."""
    what = "tune_pitch"
    if tuning is not None and not isinstance(tuning, TuningStatistics):
        raise ValueError(f"{what}: tuning must be a TuningStatistics or None, got {type(tuning).__name__}")
    forced = _root(root, what)
    mask = scale_mask(scale, what) if scale is not None else (tuning.mask if tuning is not None else SCALES["major"])
    for name, x in (("min_note_frames", min_note_frames), ("glide", glide)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 0:
            raise ValueError(f"{what}: {name} must be a non-negative int, got {x!r}")
    if isinstance(hysteresis, bool) or not isinstance(hysteresis, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(hysteresis) <= MAX_HYSTERESIS:
        raise ValueError(f"{what}: hysteresis must be 0 .. {MAX_HYSTERESIS:g} cents, got {hysteresis!r}")
    h_units = int(round(float(hysteresis) * 65536.0))
    silence, confidence = (tuning.silence, tuning.confidence) if tuning is not None else (None, 0.0)
    n, f0, h, l, voiced = _inputs(z, what, None, silence, True)
    B, T = n.shape[:2]
    if T >= 1 << 24 or B * T >= 1 << 31:
        raise ValueError(f"{what}: {B} x {T} frames: a row takes fewer than 2^24 frames, a call fewer than 2^31")
    rows = None
    if isinstance(amount, torch.Tensor):
        if amount.numel() != B or amount.device != n.device:
            raise ValueError(f"{what}: an amount tensor must hold one value per row ({B}) on {n.device}")
        rows = amount.detach().float().reshape(B).contiguous()
    elif not 0.0 <= float(np.float32(amount)) <= 1.0:
        raise ValueError(f"{what}: amount must lie in [0, 1], got {amount!r}")
    if tuning is None:
        stats_z = dict(z, normalized_cents=n) if "normalized_cents" not in z else z
        tuning = tuning_statistics(stats_z, per_row=True, scale=mask, root=root)
    if tuning.groups not in (1, B):
        raise ValueError(f"{what}: tuning has {tuning.groups} groups, the batch {B} rows: expected 1 or {B}")
    if tuning.device != n.device:
        raise ValueError(f"{what}: tuning is on {tuning.device}, the controls on {n.device}: move it once with .to()")
    flags = (_VIBRATO if vibrato else 0) | (_CONCERT if concert else 0)
    root_info = tuning.root if forced < 0 else torch.full_like(tuning.root, forced)
    if n.is_cuda:
        dev = n.device
        L = _lib.lib()
        nc, fc = n.detach().float().contiguous(), f0.detach().float().contiguous()
        hc = h.detach().float().contiguous() if h is not None else None
        lc = l.detach().float().contiguous() if l is not None else None
        vc = voiced.contiguous().view(torch.uint8) if voiced is not None else None
        out = torch.empty((2, B, T, 1), device=dev, dtype=torch.float32)
        info = torch.empty((2, B, T), device=dev, dtype=torch.int32) if return_info else None
        nbytes = L.ddsp_tuning_workspace_bytes(B, T)
        work = torch.empty(nbytes // 8, device=dev, dtype=torch.int64) if nbytes else None
        ptr = lambda x: x.data_ptr() if x is not None else None            # noqa: E731
        with torch.cuda.device(dev):
            rc = L.ddsp_tuning_apply(fc.data_ptr(), nc.data_ptr(), ptr(hc), ptr(lc), ptr(vc), tuning.offset.data_ptr(),
                                     tuning.root.data_ptr(), ptr(rows), out[0].data_ptr(), out[1].data_ptr(),
                                     info[0].data_ptr() if return_info else None, info[1].data_ptr() if return_info else None,
                                     ptr(work), B, T, tuning.groups, mask, forced, h_units, int(min_note_frames), int(glide), flags,
                                     0.0 if rows is not None else float(np.float32(amount)), 0.0 if silence is None else silence,
                                     confidence, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_tuning_apply")
        new = dict(z, f0=out[0], normalized_cents=out[1])
        if not return_info:
            return new
        return new, dict(notes=info[0], correction=info[1], correction_cents=info[1].double() / 65536.0, offset=tuning.offset,
                         root=root_info)
    flat = lambda x: None if x is None else x.detach().float().numpy().reshape(B, T)       # noqa: E731
    nn_, fn = flat(n), flat(f0)
    on = _on_host(nn_, flat(h), flat(l), None if voiced is None else voiced.numpy().reshape(B, T), silence, confidence)
    offs, roots = tuning.offset.numpy(), root_info.numpy()
    mix = rows.numpy() if rows is not None else np.full(B, np.float32(amount), dtype=np.float32)
    res = [_snap_row_host(nn_[b], fn[b], on[b], offs[b if tuning.groups > 1 else 0], roots[b if tuning.groups > 1 else 0], mask, h_units,
                          int(min_note_frames), int(glide), bool(vibrato), bool(concert), mix[b]) for b in range(B)]
    shape = tuple(n.shape)
    new = dict(z, f0=torch.from_numpy(np.stack([r[3] for r in res])).reshape(shape),
               normalized_cents=torch.from_numpy(np.stack([r[2] for r in res])).reshape(shape))
    if not return_info:
        return new
    corr = torch.from_numpy(np.stack([r[1] for r in res]))
    return new, dict(notes=torch.from_numpy(np.stack([r[0] for r in res])), correction=corr, correction_cents=corr.double() / 65536.0,
                     offset=tuning.offset, root=root_info)
