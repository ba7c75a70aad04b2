"""TEST INFRASTRUCTURE ONLY -- the overlap-add filtered noise as a stream (include/ddsp_hip.h: ddsp_noise_ola_stream; DESIGN.md
section 5a, "Live") in numpy, on top of noise_ola_reference: block by block with a carried state, in fp64 and in the arithmetic of
csrc/ddsp_noise_ola.hip (`fp32=True`: the offline emulation's tables, every chain continued from the tail's value).

With P = F - 1, M = 2 P, D = P - 1 and y the offline definition over all integer n (sources m >= 0 of the concatenated blocks):
    stream[i] = y[i - D] + dry[i - D]            (dry[< 0] = 0)
    state per row: M - 2 of tail (the partial sums of the next M - 2 stream samples), then D of dry history
Nothing under ddsp-pytorch_amd/ may import this module.
"""
from __future__ import annotations

import numpy as np

import noise_ola_reference as ref

# (B, T, hop, F, T_b): T frames streamed in blocks of T_b (the last one shorter where T_b does not divide T)
HOST_SHAPES = [(2, 6, 16, 9, 2), (1, 7, 7, 5, 3), (1, 9, 2, 9, 1), (2, 4, 64, 17, 1), (1, 3, 16, 2, 1), (1, 5, 3, 33, 2), (1, 4, 128, 65, 1)]
GPU_SHAPES = [(2, 6, 128, 65, 2),      # block longer than tail
              (1, 8, 64, 65, 1),       # tail spans two blocks
              (1, 7, 50, 33, 3),       # hop not a multiple of 8, last block shorter
              (1, 9, 2, 65, 2),        # tail spans 32 blocks
              (2, 3, 512, 195, 1),     # the reference's default bands
              (1, 4, 16, 2, 1),        # no state
              (1, 2, 1024, 257, 1),    # the range's end
              (1, 12, 512, 65, 6)]     # two output tiles per block


def delay(F):
    return max(F - 2, 0)


def state_floats(F):
    return max(3 * F - 6, 0)


def flush_frames(hop, F):
    """Silent frames after which the tail of M - 2 samples has left the stream."""
    return -(-(2 * F - 4) // hop) if F > 2 else 0


def lead_frames(hop, F):
    """Silent frames in front of an offline clip that make room for the pre-ring of D samples."""
    return -(-delay(F) // hop)


def blocks_of(T, Tb):
    return [(t, min(t + Tb, T)) for t in range(0, T, Tb)]


class Stream:
    """One stream of B rows.  `block(H, x, dry)` -> the next T hop samples [B, T hop] as fp64 values (of fp32 numbers with
    fp32=True); in fp64 `yard` then holds their yardstick Yf, carried the same way.  `state()` is the layout of the C ABI."""

    def __init__(self, B, F, hop, fp32=False, ulps=0):
        self.B, self.F, self.hop, self.fp32, self.ulps = B, F, hop, fp32, ulps
        self.tail = np.zeros((B, max(2 * F - 4, 0)))
        self.ytail = np.zeros_like(self.tail)
        self.hist = np.zeros((B, delay(F)))
        self.yard = None

    def state(self):
        return np.concatenate([self.tail, self.hist], axis=1)

    def block(self, H, x, dry=None):
        B, F, hop = self.B, self.F, self.hop
        T = H.shape[1]
        P, D, L, N = F - 1, delay(F), self.tail.shape[1], T * hop
        x = np.asarray(x, dtype=np.float64).reshape(B, N)
        rnd = ref._f32 if self.fp32 else (lambda v: v)
        if self.fp32:
            hh = ref.responses_fp32(np.asarray(H, dtype=np.float32), self.ulps)              # [B, T, P], d = |e|
            tap = lambda fr, e: hh[:, fr, abs(e)]                                             # noqa: E731
        else:
            h = ref.responses(H)                                                             # [B, T, 2P - 1]
            tap = lambda fr, e: h[:, fr, e + P - 1]                                           # noqa: E731
            A = (np.abs(np.asarray(H, dtype=np.float64)) * ref.ck(F)).sum(-1) / (2 * P)
            w = ref.window(F)
        buf = np.zeros((B, N + L))
        buf[:, :L] = self.tail
        ybuf = np.zeros((B, N + L))
        ybuf[:, :L] = self.ytail
        m = np.arange(N)
        with np.errstate(invalid="ignore"):
            for e in range(P - 1, -P, -1):                       # for every stream sample i = m + e + D: m ascending
                i = m + e + D
                buf[:, i] = rnd(buf[:, i] + tap(m // hop, e) * x)
                if not self.fp32:
                    ybuf[:, i] += w[e + P - 1] * A[:, m // hop] * np.abs(x)
        out = buf[:, :N]
        self.tail, self.ytail, self.yard = buf[:, N:], ybuf[:, N:], ybuf[:, :N]
        if dry is not None:
            dry = np.asarray(dry, dtype=np.float32).astype(np.float64).reshape(B, N)
            line = np.concatenate([self.hist, dry], axis=1)       # dry[block start - D ...]
            out = rnd(out + line[:, :N])
            self.hist = line[:, N:]
        else:
            self.hist = np.concatenate([self.hist, np.zeros((B, N))], axis=1)[:, N:]
        return out


def run(H, hop, Tb, x, dry=None, flush=True, fp32=False):
    """H [B, T, F], x [B, T, hop] (and dry [B, T hop]) streamed in blocks of Tb frames, then silent blocks of Tb frames until the
    tail has left -> (stream [B, (T + Z) hop], yard or None, Z)."""
    B, T, F = H.shape
    Z = -(-flush_frames(hop, F) // Tb) * Tb if flush else 0
    Hz = np.concatenate([H, np.zeros((B, Z, F), H.dtype)], axis=1)
    xz = np.concatenate([x, np.zeros((B, Z, hop), x.dtype)], axis=1)
    dz = None if dry is None else np.concatenate([dry, np.zeros((B, Z * hop), dry.dtype)], axis=1)
    s = Stream(B, F, hop, fp32=fp32)
    outs, yards = [], []
    for a, b in blocks_of(T + Z, Tb):
        outs.append(s.block(Hz[:, a:b], xz[:, a:b], None if dz is None else dz[:, a * hop:b * hop]))
        yards.append(s.yard)
    return np.concatenate(outs, axis=1), (None if fp32 else np.concatenate(yards, axis=1)), Z


def padded(a, lead, Z):
    """[B, T, ...] -> [B, lead + T + Z, ...] with zero frames around."""
    pad = [(0, 0), (lead, Z)] + [(0, 0)] * (a.ndim - 2)
    return np.pad(a, pad)


def shifted(y_off, lead, hop, F, n):
    """An offline result on a clip with `lead` silent frames in front -> the first n stream samples: stream[i] = y[i - D]."""
    start = lead * hop - delay(F)
    assert start >= 0 and start + n <= y_off.shape[-1]
    return y_off[..., start:start + n]
