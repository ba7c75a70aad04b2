"""Conditioning statistics and auto-adjust for timbre transfer (csrc/ddsp_condition.hip).

A decoder has only seen the register and the loudness distribution of its training set.  `conditioning_statistics` measures
both on a set of frames -- the training set (pooled), or each row of a foreign performance --, and `fit_conditioning` brings
one performance into the other's range: a shift by whole octaves towards the target's mean pitch, and a quantile map of
loudness onto the target's loudness distribution.

  ConditioningStatistics      loudness_quantiles [G, Q + 1], mean_pitch, mean_loudness, frames [G] and the options they were
                              measured with; to_dict() / from_dict() for a checkpoint's side, .to(device)
  conditioning_statistics     a dict with loudness, normalized_cents, harmonicity [R, T, 1] -> ConditioningStatistics
  fit_conditioning            a control dict, a target (and a source) -> the dict with f0, normalized_cents, loudness adjusted

CUDA tensors run the three kernels of csrc/ddsp_condition.hip; CPU tensors run the same definitions as numpy operations, to
the same bits (tests/conditioning_reference.py has them as plain loops)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .encoder import _refuse_grad

MAX_BINS, MAX_QUANTILES, MAX_OCTAVES = 8192, 1024, 32              # DDSP_CONDITION_MAX_* of include/ddsp_hip.h
VALUE_LIMIT = np.float32(1 << 15)                                  # a frame at or beyond this magnitude is not counted
MAX_GROUP_FRAMES = 1 << 24                                         # frames of one statistic
_FIXED = np.float32(1 << 24)
_OCTAVES_OFF, _OCTAVES_AUTO, _OCTAVES_FORCED = 0, 1, 2


class ConditioningStatistics:
    """What `conditioning_statistics` measured, or tables made by hand: `loudness_quantiles` [G, Q + 1] fp32 (non-decreasing
    along k; quantile k / Q of the note-on frames' loudness), `mean_pitch` and `mean_loudness` [G] fp64 (normalized cents and
    LoudnessEncoder units), `frames` [G] int64 (the note-on frames counted), and the options of the measurement: `lo`, `hi`,
    `bins`, `silence`, `confidence`.  G = 1 for pooled statistics, else one group per row."""

    def __init__(self, loudness_quantiles, mean_pitch, mean_loudness=None, frames=None, lo: float = -4.0, hi: float = 2.0,
                 bins: int = 4096, silence=None, confidence: float = 0.0):
        q = torch.as_tensor(loudness_quantiles, dtype=torch.float32)
        if q.dim() == 1:
            q = q[None]
        if q.dim() != 2 or q.shape[0] < 1 or not 2 <= q.shape[1] <= MAX_QUANTILES + 1:
            raise ValueError(f"ConditioningStatistics: loudness_quantiles must be [G, Q + 1] with 1 <= Q <= {MAX_QUANTILES}, "
                             f"got {tuple(q.shape)}")
        G, dev = q.shape[0], q.device
        self.loudness_quantiles = q.contiguous()
        self.mean_pitch = torch.as_tensor(mean_pitch, dtype=torch.float64, device=dev).reshape(-1).contiguous()
        if mean_loudness is None:
            mean_loudness = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
        self.mean_loudness = torch.as_tensor(mean_loudness, dtype=torch.float64, device=dev).reshape(-1).contiguous()
        if frames is None:                                      # hand-made tables count as well measured
            frames = torch.full((G,), MAX_GROUP_FRAMES, dtype=torch.int64, device=dev)
        self.frames = torch.as_tensor(frames, dtype=torch.int64, device=dev).reshape(-1).contiguous()
        for name in ("mean_pitch", "mean_loudness", "frames"):
            if getattr(self, name).shape[0] != G:
                raise ValueError(f"ConditioningStatistics: {name} must hold {G} values, got {getattr(self, name).shape[0]}")
        self.lo, self.hi, self.bins = float(lo), float(hi), int(bins)
        self.silence = None if silence is None else float(silence)
        self.confidence = float(confidence)

    @property
    def groups(self) -> int:
        return self.loudness_quantiles.shape[0]

    @property
    def quantiles(self) -> int:
        return self.loudness_quantiles.shape[1] - 1

    @property
    def device(self):
        return self.loudness_quantiles.device

    def options(self) -> dict:
        return dict(lo=self.lo, hi=self.hi, bins=self.bins, silence=self.silence, confidence=self.confidence)

    def to(self, device) -> "ConditioningStatistics":
        return ConditioningStatistics(self.loudness_quantiles.to(device), self.mean_pitch.to(device), self.mean_loudness.to(device),
                                      self.frames.to(device), **self.options())

    def to_dict(self) -> dict:
        """Plain tensors (on the CPU) and floats: what torch.save writes next to a checkpoint."""
        return dict(loudness_quantiles=self.loudness_quantiles.cpu(), mean_pitch=self.mean_pitch.cpu(),
                    mean_loudness=self.mean_loudness.cpu(), frames=self.frames.cpu(), **self.options())

    @classmethod
    def from_dict(cls, d: dict) -> "ConditioningStatistics":
        return cls(d["loudness_quantiles"], d["mean_pitch"], d["mean_loudness"], d["frames"], lo=d["lo"], hi=d["hi"], bins=d["bins"],
                   silence=d["silence"], confidence=d["confidence"])


def _cells(lo, hi, bins, what):
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if not isinstance(bins, (int, np.integer)) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"{what}: bins must be 1 .. {MAX_BINS}, got {bins!r}")
    if not (np.isfinite(lo32) and np.isfinite(hi32) and hi32 > lo32):
        raise ValueError(f"{what}: the histogram's range needs lo < hi, got {lo!r} and {hi!r}")
    with np.errstate(all="ignore"):
        scale = np.float32(bins) / np.float32(hi32 - lo32)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"{what}: the range [{lo!r}, {hi!r}) is too narrow for fp32 cells")
    return lo32, hi32, scale


def _rows(z, keys, what):
    """the [R, T, 1] tensors of z under `keys`, checked against the first"""
    out = []
    for k in keys:
        if k not in z:
            raise ValueError(f"{what}: the dict has no {k!r}")
        x = z[k]
        if x.dim() != 3 or x.shape[-1] != 1 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"{what}: {k} must be [R, T, 1] with R, T >= 1, got {tuple(x.shape)}")
        if out and (x.shape != out[0].shape or x.device != out[0].device):
            raise ValueError(f"{what}: {k} is {tuple(x.shape)} on {x.device}, {keys[0]} is {tuple(out[0].shape)} on {out[0].device}")
        _refuse_grad(x, what)
        out.append(x)
    return out


def _histogram_host(l, n, h, v, per_row, bins, lo32, scale, silence, confidence):
    """numpy [R, T] -> counts [G, bins] int64, sums [G, 2] int64"""
    with np.errstate(all="ignore"):
        on = (np.abs(l) < VALUE_LIMIT) & (np.abs(n) < VALUE_LIMIT) & (h >= np.float32(confidence))
        if silence is not None:
            on &= l > np.float32(silence)
        if v is not None:
            on &= v
        x = (l - lo32) * scale                                  # fp32, two roundings
        cell = np.where(x >= np.float32(bins), bins - 1, np.where(x >= 0, np.floor(x), 0)).astype(np.int64)
        fixed_n = np.rint(np.where(on, n, np.float32(0)) * _FIXED).astype(np.int64)
        fixed_l = np.rint(np.where(on, l, np.float32(0)) * _FIXED).astype(np.int64)
    groups = [slice(r, r + 1) for r in range(l.shape[0])] if per_row else [slice(None)]
    counts = np.stack([np.bincount(cell[g][on[g]], minlength=bins) for g in groups]).astype(np.int64)
    sums = np.array([[fixed_n[g].sum(), fixed_l[g].sum()] for g in groups], dtype=np.int64)
    return counts, sums


def _tables_host(counts, sums, Q, lo32, hi32):
    """counts [G, bins], sums [G, 2] int64 -> tables [G, Q + 1] fp32, mean_pitch, mean_loudness [G] fp64, frames [G] int64"""
    G, bins = counts.shape
    width = (float(hi32) - float(lo32)) / bins
    tables = np.full((G, Q + 1), np.nan, dtype=np.float32)
    means = np.full((G, 2), np.nan, dtype=np.float64)
    frames = counts.sum(axis=1)
    k = np.arange(Q + 1, dtype=np.int64)
    for g in range(G):
        N = int(frames[g])
        if N == 0:
            continue
        cum = np.cumsum(counts[g])
        b = np.searchsorted(Q * cum, np.maximum(k * N, 1), side="left")   # the first cell that reaches the quantile holds a frame
        below = np.where(b > 0, cum[np.maximum(b - 1, 0)], 0)
        c = cum[b] - below
        f = np.clip((k * N - Q * below).astype(np.float64) / (Q * c).astype(np.float64), 0.0, 1.0)
        tables[g] = (float(lo32) + (b.astype(np.float64) + f) * width).astype(np.float32)
        means[g] = [float(int(sums[g, 0])) / (float(N) * float(_FIXED)), float(int(sums[g, 1])) / (float(N) * float(_FIXED))]
    return tables, means[:, 0].copy(), means[:, 1].copy(), frames.astype(np.int64)


def conditioning_statistics(z: dict, per_row: bool = False, quantiles: int = 64, silence=None, confidence: float = 0.0, voiced=None,
                            lo: float = -4.0, hi: float = 2.0, bins: int = 4096, return_histogram: bool = False):
    """The loudness distribution and the mean pitch of the note-on frames of `z`: any dict with `loudness`,
    `normalized_cents` and `harmonicity` as [R, T, 1] (an Encoder's output, PLHDataset's feature dict, DeviceBatches'
    tensors).  Pooled (per_row=False) all rows make one statistic (G = 1: a training set); per_row=True gives one per row.

    A frame is on when loudness and normalized_cents are finite (and of magnitude below 2^15), loudness > `silence` (None: no
    gate), harmonicity >= `confidence`, and `voiced` (a bool [R, T, 1]; None: z['voiced'] where the dict has one) is true.
    The defaults -- silence=None, confidence=0.0, no mask -- count every finite frame; they are not tuned here.

    The on frames' loudness is counted in `bins` (at most 8192) equal cells over [lo, hi), frames outside going to the first
    and the last cell, and `quantiles` + 1 (Q at most 1024) table entries are read off the cumulative counts, linear inside a
    cell.  The means come from two int64 sums of llrintf(value * 2^24).  Everything accumulated is an integer, so the result is
    the same bits whatever the order of the rows, and from run to run.  An int64 sum cannot overflow: a counted value is below
    2^15 in magnitude (larger ones are not on) and one statistic takes at most 2^24 frames -- R T pooled, T per row; more is
    refused with a ValueError, as is R T >= 2^32 -- so that |sum| < 2^15 2^24 2^24 = 2^63.  A statistic without a single on
    frame has NaN tables and means, and frames = 0.

    -> ConditioningStatistics; with return_histogram=True, (statistics, counts [G, bins] int64, sums [G, 2] int64).
    On the device: one statistics launch (behind one memset when pooled) and one tables launch, no host synchronisation."""
    what = "conditioning_statistics"
    l, n, h = _rows(z, ("loudness", "normalized_cents", "harmonicity"), what)
    R, T = l.shape[:2]
    if voiced is None:
        voiced = z.get("voiced")
    if voiced is not None and (voiced.shape != l.shape or voiced.device != l.device or voiced.dtype != torch.bool):
        raise ValueError(f"{what}: voiced must be a bool tensor {tuple(l.shape)} on {l.device}")
    if not isinstance(quantiles, (int, np.integer)) or not 1 <= quantiles <= MAX_QUANTILES:
        raise ValueError(f"{what}: quantiles must be 1 .. {MAX_QUANTILES}, got {quantiles!r}")
    lo32, hi32, scale = _cells(lo, hi, bins, what)
    if silence is not None and np.isnan(np.float32(silence)) or np.isnan(np.float32(confidence)):
        raise ValueError(f"{what}: silence and confidence must not be NaN")
    if R * T >= 1 << 32 or (T if per_row else R * T) > MAX_GROUP_FRAMES:
        raise ValueError(f"{what}: {R} x {T} frames: one statistic takes at most 2^24 frames (the int64 fixed-point sums), "
                         "a call fewer than 2^32")
    Q, G = int(quantiles), (R if per_row else 1)
    opts = dict(lo=float(lo32), hi=float(hi32), bins=int(bins), silence=silence, confidence=float(np.float32(confidence)))
    if l.is_cuda:
        dev = l.device
        L = _lib.lib()
        lc, nc, hc = (x.detach().float().contiguous() for x in (l, n, h))
        vc = voiced.contiguous().view(torch.uint8) if voiced is not None else None
        nbytes = L.ddsp_condition_accum_bytes(G, bins)
        accum = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
        tables = torch.empty((G, Q + 1), device=dev, dtype=torch.float32)
        means = torch.empty((2, G), device=dev, dtype=torch.float64)
        frames = torch.empty(G, device=dev, dtype=torch.int64)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            rc = L.ddsp_condition_stats(lc.data_ptr(), nc.data_ptr(), hc.data_ptr(), vc.data_ptr() if vc is not None else None,
                                        accum.data_ptr(), R, T, 0 if per_row else 1, bins, float(lo32), float(hi32),
                                        float("-inf") if silence is None else float(np.float32(silence)), opts["confidence"], stream)
            _lib.check(rc, "ddsp_condition_stats")
            rc = L.ddsp_condition_tables(accum.data_ptr(), tables.data_ptr(), means[0].data_ptr(), means[1].data_ptr(),
                                         frames.data_ptr(), G, bins, Q, float(lo32), float(hi32), stream)
            _lib.check(rc, "ddsp_condition_tables")
        stats = ConditioningStatistics(tables, means[0], means[1], frames, **opts)
        if not return_histogram:
            return stats
        cells = (G * bins * 4 + 7) // 8                                       # int64 words of the counts
        counts = accum[:cells].view(torch.int32)[:G * bins].view(G, bins).to(torch.int64) & 0xFFFFFFFF
        return stats, counts, accum[cells:cells + 2 * G].view(G, 2).clone()
    ln, nn_, hn = (x.detach().float().numpy().reshape(R, T) for x in (l, n, h))
    vn = voiced.numpy().reshape(R, T) if voiced is not None else None
    counts, sums = _histogram_host(ln, nn_, hn, vn, per_row, int(bins), lo32, scale, silence, confidence)
    tables, mean_pitch, mean_loudness, frames = _tables_host(counts, sums, Q, lo32, hi32)
    stats = ConditioningStatistics(torch.from_numpy(tables), torch.from_numpy(mean_pitch), torch.from_numpy(mean_loudness),
                                   torch.from_numpy(frames), **opts)
    return (stats, torch.from_numpy(counts), torch.from_numpy(sums)) if return_histogram else stats


def _octave_mode(octaves, max_octaves, what):
    if not isinstance(max_octaves, (int, np.integer)) or isinstance(max_octaves, bool) or not 0 <= max_octaves <= MAX_OCTAVES:
        raise ValueError(f"{what}: max_octaves must be 0 .. {MAX_OCTAVES}, got {max_octaves!r}")
    if octaves is True:
        return _OCTAVES_AUTO, 0
    if octaves is False or octaves is None:
        return _OCTAVES_OFF, 0
    if not isinstance(octaves, (int, np.integer)) or abs(int(octaves)) > MAX_OCTAVES:
        raise ValueError(f"{what}: octaves must be a bool or an int within +-{MAX_OCTAVES}, got {octaves!r}")
    return _OCTAVES_FORCED, int(octaves)


def _map_host(l, S, Tt, strength):
    """one row [T] fp32 through the tables S and Tt [Q + 1] (no NaN): every operation fp32, none fused"""
    Q = len(S) - 1
    out = l.copy()
    fin = np.isfinite(l)
    x = l[fin]
    with np.errstate(all="ignore"):
        k = np.clip(np.searchsorted(S, x, side="right") - 1, 0, Q - 1)      # the largest k with S[k] <= x
        d = S[k + 1] - S[k]
        w = np.where(d > 0, (x - S[k]) / np.where(d > 0, d, np.float32(1)), np.float32(0.5)).astype(np.float32)
        mapped = Tt[k] + w * (Tt[k + 1] - Tt[k])
        mapped = np.where(x < S[0], x + (Tt[0] - S[0]), np.where(x >= S[Q], x + (Tt[Q] - S[Q]), mapped)).astype(np.float32)
        out[fin] = x + strength * (mapped - x)
    return out


def fit_conditioning(z: dict, target: ConditioningStatistics, source=None, octaves=True, max_octaves: int = 2, strength=1.0,
                     min_frames: int = 8, return_info: bool = False):
    """Bring the controls `z` (f0, normalized_cents, loudness as [B, T, 1]) into the range of `target` (G = 1, or one group per
    row): -> a new dict with those three replaced, every other key the same object.

    source=None measures each row of z itself (`conditioning_statistics(z, per_row=True)` with the target's quantile count
    and options; z then needs `harmonicity`): the offline, whole-clip use.  A given `source` (G = 1 or B, the target's
    quantile count) is used as is: calibrate once on a few seconds of the player, then map block after block -- one launch,
    no host synchronisation, no allocation after the outputs, so the call can be captured in a graph.

    Pitch: k = rint((target.mean_pitch - source.mean_pitch) 7180 / 1200) octaves (ties to even) clamped to +-max_octaves;
    f0 is scaled by 2^k exactly and normalized_cents moved by fl32(k 1200 / 7180).  octaves=False: no shift; an int: that k.
    Loudness: below the source's first quantile and from its last one on, a shift by the difference of the two tables' ends;
    between, linear from source quantile to target quantile; the result is l + strength (mapped - l), `strength` a float or a
    per-row tensor [B].  The map is continuous and monotone; a loudness that is not finite passes through.
    A row whose source counted fewer than `min_frames` on frames, or whose tables hold a NaN, is returned as it came; that is
    decided on the device.  return_info=True adds a dict of `octaves` [B] int32 and `frames` [B] int64 (the source's)."""
    what = "fit_conditioning"
    f0, n, l = _rows(z, ("f0", "normalized_cents", "loudness"), what)
    B, T = l.shape[:2]
    if not isinstance(target, ConditioningStatistics):
        raise ValueError(f"{what}: target must be a ConditioningStatistics, got {type(target).__name__}")
    mode, forced = _octave_mode(octaves, max_octaves, what)
    if not isinstance(min_frames, (int, np.integer)) or min_frames < 0:
        raise ValueError(f"{what}: min_frames must be a non-negative int, got {min_frames!r}")
    if B * T >= 1 << 32:
        raise ValueError(f"{what}: {B} x {T} frames: a call takes fewer than 2^32")
    if source is None:
        source = conditioning_statistics(z, per_row=True, quantiles=target.quantiles, **target.options())
    elif not isinstance(source, ConditioningStatistics):
        raise ValueError(f"{what}: source must be a ConditioningStatistics or None, got {type(source).__name__}")
    for name, s in (("target", target), ("source", source)):
        if s.groups not in (1, B):
            raise ValueError(f"{what}: {name} has {s.groups} groups, the batch {B} rows: expected 1 or {B}")
        if s.device != l.device:
            raise ValueError(f"{what}: {name} is on {s.device}, the controls on {l.device}: move it once with .to()")
    if source.quantiles != target.quantiles:
        raise ValueError(f"{what}: source has {source.quantiles} quantiles, target {target.quantiles}")
    rows = None
    if isinstance(strength, torch.Tensor):
        if strength.numel() != B or strength.device != l.device:
            raise ValueError(f"{what}: a strength tensor must hold one value per row ({B}) on {l.device}")
        rows = strength.detach().float().reshape(B).contiguous()
    elif np.isnan(np.float32(strength)):
        raise ValueError(f"{what}: strength must not be NaN")
    Q = target.quantiles
    if l.is_cuda:
        dev = l.device
        L = _lib.lib()
        fc, nc, lc = (x.detach().float().contiguous() for x in (f0, n, l))
        out = torch.empty((3, B, T, 1), device=dev, dtype=torch.float32)
        octs = torch.empty(B, device=dev, dtype=torch.int32) if return_info else None
        have = torch.empty(B, device=dev, dtype=torch.int64) if return_info else None
        with torch.cuda.device(dev):
            rc = L.ddsp_condition_apply(fc.data_ptr(), nc.data_ptr(), lc.data_ptr(), source.loudness_quantiles.data_ptr(),
                                        source.mean_pitch.data_ptr(), source.frames.data_ptr(), target.loudness_quantiles.data_ptr(),
                                        target.mean_pitch.data_ptr(), rows.data_ptr() if rows is not None else None,
                                        out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                        octs.data_ptr() if return_info else None, have.data_ptr() if return_info else None, B, T,
                                        source.groups, target.groups, Q, mode, forced, int(max_octaves),
                                        0.0 if rows is not None else float(np.float32(strength)), int(min_frames),
                                        torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ddsp_condition_apply")
        new = dict(z, f0=out[0], normalized_cents=out[1], loudness=out[2])
        return (new, dict(octaves=octs, frames=have)) if return_info else new
    fn, nn_, ln = (x.detach().float().numpy().reshape(B, T) for x in (f0, n, l))
    S, Tt = source.loudness_quantiles.numpy(), target.loudness_quantiles.numpy()
    sm, tm, sf = source.mean_pitch.numpy(), target.mean_pitch.numpy(), source.frames.numpy()
    mix = rows.numpy() if rows is not None else np.full(B, np.float32(strength), dtype=np.float32)
    out_f, out_n, out_l = fn.copy(), nn_.copy(), ln.copy()
    octs, have = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int64)
    for r in range(B):
        gs, gt = (r if source.groups > 1 else 0), (r if target.groups > 1 else 0)
        have[r] = sf[gs]
        if sf[gs] < min_frames or np.isnan(S[gs]).any() or np.isnan(Tt[gt]).any():
            continue
        k = 0
        if mode == _OCTAVES_FORCED:
            k = forced
        elif mode == _OCTAVES_AUTO:
            with np.errstate(all="ignore"):
                x = np.rint((tm[gt] - sm[gs]) * 7180.0 / 1200.0)
            k = int(np.clip(x, -max_octaves, max_octaves)) if np.isfinite(x) else 0
        octs[r] = k
        with np.errstate(all="ignore"):
            out_f[r] = np.ldexp(fn[r], k)
            out_n[r] = nn_[r] + np.float32(k * 1200.0 / 7180.0)
        out_l[r] = _map_host(ln[r], S[gs], Tt[gt], mix[r])
    shape = tuple(l.shape)
    new = dict(z, f0=torch.from_numpy(out_f).reshape(shape), normalized_cents=torch.from_numpy(out_n).reshape(shape),
               loudness=torch.from_numpy(out_l).reshape(shape))
    return (new, dict(octaves=torch.from_numpy(octs), frames=torch.from_numpy(have))) if return_info else new
