"""Wavetable synthesis (include/ddsp_hip.h: ddsp_wavetable_*) as plain numpy in fp64: the forward, the analytic
gradients, and per-element error bounds with the kernels' roundings counted.

What is fp32 BY DEFINITION is emulated as fp32: the upsampling weights (F.interpolate's own fp32 expression), g = fl32(f0 / sr) and
the per-sample increment u = fl32(fma(w0, g[i0], fl32(w1 g[i1]))).  Everything after that is fp64; the phase is accumulated in
extended precision and rounded once, so that the reference's own phase error stays far below the 2^-50 (P + 1) cycles the bound allows.

Where the bounds are wider than the form the feature was specified with (forward (N + r) 2^-24 A[n] + E_phase with the LOCAL table
slope; gradients (S + N + r) 2^-24 sum |terms| and nothing else), each by a term of order 2^-50 (P + 1) L:
  * E_phase takes the largest slope over the entries j - 1, j and j + 1, not the slope at j alone.  Where pos lands on an integer
    (f0 = sample_rate / L m) a phase that differs in its last fp64 bits reads the neighbouring entry, whose slope then applies.
  * the gradient bounds add the same phase effect (ph_a, ph_c, ph_W below), which the specified form leaves out: the gradients
    re-walk phases that carry the forward's 2^-50 (P + 1) error, so s_k (grad_c, grad_a) and the scatter weights 1 - fr and fr
    (grad_W, at the entries j - 1 .. j + 2 the weight can move to) are off by that much times the slope.
The fp32 parts of every bound are the specified ones.
"""
import numpy as np

EPS = 2.0 ** -24            # unit roundoff of fp32
PHASE_EPS = 2.0 ** -50      # allowed fp64 phase error, relative to P + 1 (cycles)

# The forward's counted roundings beside the N fused multiply-adds of the sum over the tables (each rounds a partial sum that is at
# most sum |terms|), in units of 2^-24 A[n]:
#   the interpolated entry s_k, relative to max(|W[k,j]|, |W[k,j+1]|): the difference W[k,j+1] - W[k,j] (<= 2), its product with fr inside
#   the fma and the fma's own rounding (1), fr rounded to fp32 from fp64 (fr |difference| <= 2)                      5
#   sum_k c rounded from fp64 to fp32 (1), the division A / S (1)                                                     2
#   w1 (A1 / S1) and the fma with w0 (A0 / S0)                                                                        2
#   up(a): w1 a[i1] and the fma                                                                                       2
#   the product up(a) M                                                                                               1
# 12, and 2 more for the second-order terms of all of these compounded (N <= 1024: (N + 12)^2 2^-24 < 2 (N + 12) / 16).
R_FORWARD = 14
# The gradients: an element sums S sample terms (S roundings of the partial sums, the finish's two additions of the three partials
# among them).  N covers what a term inherits from a sum over the tables: grad_a's M is the forward's sum, grad_c's normalisation
# is a dot product over the tables, grad_W's mix weight m_k needs no sum (its two divisions and fma are 4).  Beside that, per term:
#   s_k as in the forward, against max |W| (grad_c, grad_a)                                                          5
#   grad_y up(a) (up(a): 2, the product: 1), times the frame weight (1), times s_k or m_k (the fma into the sum: in S)  4
#   sum_k c to fp32 and the division(s) by it; the subtraction of the normalisation's dot product                    4
#   second-order terms                                                                                                3
# 16, the most the bound's form allows.
R_BACKWARD = 16


def upsample_plan(T, hop):
    """-> i0, i1 (int), w0, w1 (fp32 values as fp64) of F.interpolate(scale_factor=hop, mode='linear', align_corners=False)"""
    n = np.arange(T * hop, dtype=np.float64)
    scale = np.float64(np.float32(1.0) / np.float32(hop))
    src = (scale * (n + 0.5) - 0.5).astype(np.float32)          # one rounding: the product is exact in fp64
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(src.astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    w1 = np.clip(src - i0.astype(np.float32), np.float32(0.0), np.float32(1.0)).astype(np.float32)
    w0 = (np.float32(1.0) - w1).astype(np.float32)
    return i0, i1, w0.astype(np.float64), w1.astype(np.float64)


def increments(f0, hop, sample_rate):
    """f0 [B, T] fp32 -> u [B, T hop]: the fp32 increments (cycles per sample), as fp64 values"""
    B, T = f0.shape
    i0, i1, w0, w1 = upsample_plan(T, hop)
    g = (f0.astype(np.float32) / np.float32(sample_rate)).astype(np.float32)
    v = (w1.astype(np.float32)[None] * g[:, i1]).astype(np.float32)
    return (w0[None] * g[:, i0].astype(np.float64) + v.astype(np.float64)).astype(np.float32).astype(np.float64)


def phases_from_increments(u, P0=None):
    """u [B, n] (fp32 values) -> P [B, n] fp64 (cycles): P0 + the inclusive sum, accumulated in extended precision, rounded once"""
    u = np.asarray(u, np.float64).astype(np.longdouble)
    start = np.zeros(u.shape[0], np.longdouble) if P0 is None else np.asarray(P0, np.float64).astype(np.longdouble)
    return (start[:, None] + np.cumsum(u, axis=1)).astype(np.float64)


def phases(f0, hop, sample_rate, P0=None):
    return phases_from_increments(increments(f0, hop, sample_rate), P0)


def positions(P, L):
    pos = (P - np.floor(P)) * L
    j = np.clip(np.floor(pos).astype(np.int64), 0, L - 1)
    return j, (j + 1) % L, pos - j


def _setup(f0, c, a, W, hop, sample_rate, P0):
    f0 = np.asarray(f0, np.float32).reshape(c.shape[0], c.shape[1])
    c64, a64, W64 = np.asarray(c, np.float64), np.asarray(a, np.float64).reshape(f0.shape), np.asarray(W, np.float64)
    B, T, N = c64.shape
    i0, i1, w0, w1 = upsample_plan(T, hop)
    P = phases(f0, hop, sample_rate, P0)
    j, j1, fr = positions(P, W64.shape[1])
    S = c64.sum(-1)
    wn = c64 / S[..., None]
    m = w0[None, :, None] * wn[:, i0] + w1[None, :, None] * wn[:, i1]              # up(wn) [B, n, N]
    au = w0[None] * a64[:, i0] + w1[None] * a64[:, i1]                              # up(a)  [B, n]
    k = np.arange(N)[None, None, :]
    Wj, Wj1 = W64[k, j[..., None]], W64[k, j1[..., None]]                           # [B, n, N]
    s = Wj + fr[..., None] * (Wj1 - Wj)
    return dict(B=B, T=T, N=N, L=W64.shape[1], i0=i0, i1=i1, w0=w0, w1=w1, P=P, j=j, j1=j1, fr=fr, S=S, wn=wn, m=m, au=au, Wj=Wj, Wj1=Wj1,
                s=s, W=W64)


def _slope(d):
    """max |W[k, e + 1] - W[k, e]| over e = j - 1, j, j + 1: what a small phase error can multiply (the entry may change)"""
    W, L = d["W"], d["L"]
    diff = np.abs(np.roll(W, -1, axis=1) - W)                                       # [N, L]: entry e -> e + 1
    k = np.arange(d["N"])[None, None, :]
    j = d["j"][..., None]
    return np.maximum(np.maximum(diff[k, (j - 1) % L], diff[k, j]), diff[k, (j + 1) % L])


def forward(f0, c, a, W, hop, sample_rate, P0=None):
    """-> (y [B, T hop] fp64, bound [B, T hop], end phase [B] fp64 in [0, 1))"""
    d = _setup(f0, c, a, W, hop, sample_rate, P0)
    y = d["au"] * (d["m"] * d["s"]).sum(-1)
    smax = np.maximum(np.abs(d["Wj"]), np.abs(d["Wj1"]))
    A = np.abs(d["au"]) * (np.abs(d["m"]) * smax).sum(-1)
    delta = PHASE_EPS * (np.abs(d["P"]) + 1.0) * d["L"]                             # entries
    E = np.abs(d["au"]) * (np.abs(d["m"]) * _slope(d)).sum(-1) * delta
    end = d["P"][:, -1] - np.floor(d["P"][:, -1])
    return y, (d["N"] + R_FORWARD) * EPS * A + E, end


def backward(grad_y, f0, c, a, W, hop, sample_rate, P0=None):
    """-> dict(grad_c, grad_a, grad_W: fp64; bound_c, bound_a, bound_W) for y's gradient grad_y [B, T hop]"""
    d = _setup(f0, c, a, W, hop, sample_rate, P0)
    B, T, N, L = d["B"], d["T"], d["N"], d["L"]
    gy = np.asarray(grad_y, np.float64)
    i0, i1, w0, w1 = d["i0"], d["i1"], d["w0"], d["w1"]
    q = gy * d["au"]
    smax = np.maximum(np.abs(d["Wj"]), np.abs(d["Wj1"]))
    delta = PHASE_EPS * (np.abs(d["P"]) + 1.0) * L
    slope = _slope(d)
    rows = np.arange(B)[:, None]

    def to_frames(x):
        """x [B, n, ...] -> [B, T, ...]: every sample's share to its two frames"""
        out = np.zeros((B, T) + x.shape[2:])
        shape = (1, -1) + (1,) * (x.ndim - 2)
        np.add.at(out, (rows, i0[None]), x * w0.reshape(shape))
        np.add.at(out, (rows, i1[None]), x * w1.reshape(shape))
        return out

    reach = np.zeros((B, T))
    np.add.at(reach, (rows, np.broadcast_to(i0[None], (B, T * hop))), 1.0)
    np.add.at(reach, (rows, np.broadcast_to(i1[None], (B, T * hop))), 1.0)         # samples summed into a frame, <= 2 hop

    M = (d["m"] * d["s"]).sum(-1)
    grad_a = to_frames(gy * M)
    abs_a = to_frames(np.abs(gy) * (np.abs(d["m"]) * smax).sum(-1))
    ph_a = to_frames(np.abs(gy) * (np.abs(d["m"]) * slope).sum(-1) * delta)
    bound_a = (reach + N + R_BACKWARD) * EPS * abs_a + ph_a

    G = to_frames(q[..., None] * d["s"])
    absG = to_frames(np.abs(q)[..., None] * smax)
    phG = to_frames((np.abs(q) * delta)[..., None] * slope)
    S, wn = d["S"][..., None], d["wn"]
    grad_c = (G - (G * wn).sum(-1, keepdims=True)) / S
    abs_c = (absG + (absG * np.abs(wn)).sum(-1, keepdims=True)) / np.abs(S)
    ph_c = (phG + (phG * np.abs(wn)).sum(-1, keepdims=True)) / np.abs(S)
    bound_c = (reach[..., None] + N + R_BACKWARD) * EPS * abs_c + ph_c

    grad_W, abs_W, ph_W, touch = (np.zeros((N, L)) for _ in range(4))
    k = np.broadcast_to(np.arange(N)[None, None, :], d["m"].shape)
    qm = q[..., None] * d["m"]
    for idx, wgt in ((d["j"], 1.0 - d["fr"]), (d["j1"], d["fr"])):
        e = np.broadcast_to(idx[..., None], d["m"].shape)
        np.add.at(grad_W, (k, e), qm * wgt[..., None])
        np.add.at(abs_W, (k, e), np.abs(qm) * wgt[..., None])
        np.add.at(touch, (k, e), 1.0)
    # a phase error moves weight between an entry and its neighbour, and at pos = integer it changes the entry itself
    for off in (-1, 0, 1, 2):
        e = np.broadcast_to(((d["j"] + off) % L)[..., None], d["m"].shape)
        np.add.at(ph_W, (k, e), np.abs(qm) * delta[..., None])
    bound_W = (touch + N + R_BACKWARD) * EPS * abs_W + ph_W
    return dict(grad_c=grad_c, grad_a=grad_a.reshape(B, T, 1), grad_W=grad_W, bound_c=bound_c, bound_a=bound_a.reshape(B, T, 1),
                bound_W=bound_W)
