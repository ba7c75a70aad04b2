"""The inharmonic sinusoid bank (include/ddsp_hip.h: ddsp_sinusoids_*) as plain numpy in fp64: the forward, the
analytic gradients, and per-element error bounds with the kernels' roundings counted.

What is fp32 BY DEFINITION is emulated as fp32: the upsampling weights of a and of the normalised weights (F.interpolate's own fp32
expression, `upsample_plan`).  Everything else is fp64, and the phase -- the inclusive sum of the linearly interpolated
g = f / sample_rate taken in REAL arithmetic (`ideal_plan`) -- is evaluated through its closed form per segment in longdouble and
rounded once.

Phase bound, E_P = (T + 8) 2^-53 (|P| + 1) turns.  The device keeps Phi, the phase at a segment's start, by a sequential fp64
prefix of T + 1 non-negative terms (head g[0], then one total per segment), each addition rounding to 2^-53 of a partial sum that
is at most P, or at most 1 + the term where the prefix is kept modulo 1: T.  A term itself (hop g[s] and its FMA with d / (2 hop)),
the correctly rounded divisions f / sample_rate and d / (2 hop), the subtraction d, the two FMAs inside the segment and the
reduction modulo 1 are 8 more roundings, none larger than 2^-53 (|P| + 1).

The sine: e_sin = EPS_SIN + 2 pi (2^-25 + E_P) -- the hardware's v_sin_f32 / v_cos_f32 (harmonic_analysis_reference.EPS_SIN), the
reduced phase in [-1/2, 1/2] rounded to fp32 (2^-25 turns), and the phase error.
"""
import numpy as np

from harmonic_analysis_reference import EPS_SIN

EPS = 2.0 ** -24            # unit roundoff of fp32
EPS64 = 2.0 ** -53

# The forward's counted roundings beside the K fused multiply-adds of the sum over the partials (each rounds a partial sum that is
# at most sum_k |A_k|), in units of 2^-24 |A_k|:
#   the weights' sum rounded from fp64 to fp32 (1), the division w / S (1)                      2
#   up(wn): w1 wn[i1] and the fma with w0 wn[i0]                                                2
#   up(a): w1 a[i1] and the fma                                                                 2
#   the product up(a) * sum                                                                     1
# 7, and 1 more for the second-order terms of all of these compounded (K <= 1024: (K + 7)^2 2^-24 < (K + 7) / 16).
R_FORWARD = 8
# The gradients: an element sums S sample terms (S roundings of the partial sums; the finish's additions of the four partials are
# among them).  K covers what a term inherits from a sum over the partials (grad_a's sum over k, grad_c's normalisation dot
# product).  Beside that, per term:
#   up(a) (2), grad_y up(a) (1), the frame weight w0 / w1 or the coefficient's product inside the fma (1)         4
#   wn (2) and up(wn) (2): grad_a and grad_f                                                                      4
#   grad_c: S to fp32, wn for the dot product (2), the subtraction, the division                                  (5, instead of the 4 above)
#   grad_f: fl32(2 pi) and its product (2), the products with up(wn) and the cosine (2), the coefficient
#           (j + 1) (j + e) / (2 hop): a division, a product, and the subtraction from j + 1 (3)                   7
#   the result rounded to fp32 from the fp64 combination (grad_f)                                                 1
# 16 for grad_f; the others are below and share the constant.
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


def ideal_plan(T, hop):
    """The same interpolation in real arithmetic: i0, i1 and w0, w1 as longdouble (src 2 hop = 2 n + 1 - hop is an integer)."""
    n = np.arange(T * hop, dtype=np.int64)
    num = np.maximum(2 * n + 1 - hop, 0)
    i0 = np.minimum(num // (2 * hop), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    w1 = np.minimum((num - i0 * 2 * hop).astype(np.longdouble) / np.longdouble(2 * hop), np.longdouble(1.0))
    return i0, i1, np.longdouble(1.0) - w1, w1


def frame_terms(f, c, sample_rate, normalize=True, cast=True):
    """f, c [B, T, K] -> dict(valid, mask, g, w, S, wn), fp64.  `cast=False` takes the inputs as the fp64 values they are (for
    finite differences) instead of as the fp32 values the kernels are given."""
    f32 = np.asarray(f, np.float32 if cast else np.float64)
    c64 = np.asarray(c, np.float32 if cast else np.float64).astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(f32) & (f32 >= 0)
        mask = valid & ~(f32 > np.float32(sample_rate // 2))
    g = np.where(valid, np.where(valid, f32, 0).astype(np.float64) / np.float64(sample_rate), 0.0)
    w = np.where(mask, c64, 0.0)
    S = w.sum(-1, keepdims=True)
    if normalize:
        with np.errstate(divide="ignore", invalid="ignore"):
            wn = np.where(S != 0, w / np.where(S != 0, S, 1.0), 0.0)
    else:
        wn = w
    return dict(valid=valid, mask=mask, g=g, w=w, S=S, wn=wn)


def phases_closed_form(g, hop, P0=None):
    """g [B, T, K] fp64 -> P [B, T hop, K] fp64 (turns), through the closed form in longdouble, rounded once"""
    B, T, K = g.shape
    gl = g.astype(np.longdouble)
    head, e = hop // 2, 1 - hop % 2
    d = np.concatenate([gl[:, 1:] - gl[:, :-1], np.zeros((B, 1, K), np.longdouble)], axis=1)
    tot = hop * (gl + d * np.longdouble(hop - 1 + e) / np.longdouble(2 * hop))
    Phi = head * gl[:, :1] + np.cumsum(tot, axis=1) - tot                       # exclusive
    n = np.arange(T * hop, dtype=np.int64)
    m = n - head
    s = np.clip(m // hop, 0, T - 1)
    j = m - s * hop
    frac = ((j + e).astype(np.longdouble) / np.longdouble(2 * hop))[None, :, None]
    P = Phi[:, s] + (j + 1).astype(np.longdouble)[None, :, None] * (gl[:, s] + d[:, s] * frac)
    P = np.where((m < 0)[None, :, None], (n + 1).astype(np.longdouble)[None, :, None] * gl[:, :1], P)
    if P0 is not None:
        P = P + np.asarray(P0, np.float64).astype(np.longdouble)[:, None, :]
    return P.astype(np.float64)


def phases_running_sum(g, hop, P0=None):
    """The definition itself: a longdouble running sum of the exactly interpolated increments"""
    B, T, K = g.shape
    i0, i1, w0, w1 = ideal_plan(T, hop)
    gl = g.astype(np.longdouble)
    u = w0[None, :, None] * gl[:, i0] + w1[None, :, None] * gl[:, i1]
    P = np.cumsum(u, axis=1)
    if P0 is not None:
        P = P + np.asarray(P0, np.float64).astype(np.longdouble)[:, None, :]
    return P.astype(np.float64)


def _setup(f, c, a, hop, sample_rate, P0, normalize, cast=True):
    fr = frame_terms(f, c, sample_rate, normalize, cast)
    B, T, K = fr["g"].shape
    a64 = np.asarray(a, np.float32 if cast else np.float64).astype(np.float64).reshape(B, T)
    i0, i1, w0, w1 = upsample_plan(T, hop)
    P = phases_closed_form(fr["g"], hop, P0)
    wv = w0[None, :, None] * fr["wn"][:, i0] + w1[None, :, None] * fr["wn"][:, i1]       # up(wn) [B, n, K]
    au = w0[None] * a64[:, i0] + w1[None] * a64[:, i1]                                     # up(a)  [B, n]
    E_P = (T + 8) * EPS64 * (np.abs(P) + 1.0)
    e_sin = EPS_SIN + 2.0 * np.pi * (2.0 ** -25 + E_P)
    fr.update(B=B, T=T, K=K, i0=i0, i1=i1, w0=w0, w1=w1, P=P, wv=wv, au=au, E_P=E_P, e_sin=e_sin)
    return fr


def forward(f, c, a, hop, sample_rate, P0=None, normalize=True, cast=True):
    """-> dict(y [B, T hop] fp64, bound, bound_fp32 (the bound without the sine's term), end [B, K] the carried phase in [0, 1),
    E_end [B, K] its allowance)"""
    d = _setup(f, c, a, hop, sample_rate, P0, normalize, cast)
    with np.errstate(invalid="ignore"):
        y = d["au"] * (d["wv"] * np.sin(2.0 * np.pi * (d["P"] - np.floor(d["P"])))).sum(-1)
    A = np.abs(d["au"])[..., None] * np.abs(d["wv"])
    fp32 = (d["K"] + R_FORWARD) * EPS * A.sum(-1)
    bound = (A * d["e_sin"]).sum(-1) + fp32
    end = d["P"][:, -1] - np.floor(d["P"][:, -1])
    return dict(y=y, bound=bound, bound_fp32=fp32, end=end, E_end=d["E_P"][:, -1], P=d["P"])


def backward(grad_y, f, c, a, hop, sample_rate, P0=None, normalize=True, cast=True):
    """-> dict(grad_f, grad_c, grad_a: fp64; bound_f, bound_c, bound_a) for y's gradient grad_y [B, T hop]"""
    d = _setup(f, c, a, hop, sample_rate, P0, normalize, cast)
    B, T, K = d["B"], d["T"], d["K"]
    gy = np.asarray(grad_y, np.float64)
    i0, i1, w0, w1 = d["i0"], d["i1"], d["w0"], d["w1"]
    rows = np.arange(B)[:, None]
    ph = 2.0 * np.pi * (d["P"] - np.floor(d["P"]))
    sn, cs = np.sin(ph), np.cos(ph)

    def to_frames(x):
        """x [B, n, ...] -> [B, T, ...]: every sample's share to its two frames (the fp32 weights)"""
        out = np.zeros((B, T) + x.shape[2:])
        shape = (1, -1) + (1,) * (x.ndim - 2)
        np.add.at(out, (rows, i0[None]), x * w0.reshape(shape))
        np.add.at(out, (rows, i1[None]), x * w1.reshape(shape))
        return out

    reach = np.zeros((B, T))
    np.add.at(reach, (rows, np.broadcast_to(i0[None], (B, T * hop))), 1.0)
    np.add.at(reach, (rows, np.broadcast_to(i1[None], (B, T * hop))), 1.0)             # samples summed into a frame, <= 2 hop

    grad_a = to_frames(gy * (d["wv"] * sn).sum(-1))
    abs_a = to_frames(np.abs(gy) * np.abs(d["wv"]).sum(-1))
    sin_a = to_frames(np.abs(gy) * (np.abs(d["wv"]) * d["e_sin"]).sum(-1))
    bound_a = sin_a + (reach + K + R_BACKWARD) * EPS * abs_a

    q0 = gy * d["au"]
    G = to_frames(q0[..., None] * sn)
    absG = to_frames(np.broadcast_to(np.abs(q0)[..., None], sn.shape))
    sinG = to_frames(np.abs(q0)[..., None] * d["e_sin"])
    if normalize:
        S, wn = d["S"], d["wn"]
        ok = S != 0
        Sx = np.where(ok, S, 1.0)
        grad_w = np.where(ok, (G - (G * wn).sum(-1, keepdims=True)) / Sx, 0.0)
        abs_c = np.where(ok, (absG + (absG * np.abs(wn)).sum(-1, keepdims=True)) / np.abs(Sx), 0.0)
        sin_c = np.where(ok, (sinG + (sinG * np.abs(wn)).sum(-1, keepdims=True)) / np.abs(Sx), 0.0)
    else:
        grad_w, abs_c, sin_c = G, absG, sinG
    grad_c = np.where(d["mask"], grad_w, 0.0)
    bound_c = np.where(d["mask"], sin_c + (reach[..., None] + K + R_BACKWARD) * EPS * abs_c, 0.0)

    # grad_f: sum_n q[n] D[n, t] with D[n, t] = sum_{m <= n} (w0(m) [i0(m) = t] + w1(m) [i1(m) = t]) in real arithmetic, i.e. every
    # sample m hands the sum of q behind it (itself included) to its two frames
    x0, x1, v0, v1 = ideal_plan(T, hop)
    v0, v1 = v0.astype(np.float64), v1.astype(np.float64)
    absq = np.abs(q0)[..., None] * np.abs(d["wv"]) * 2.0 * np.pi
    q = q0[..., None] * d["wv"] * 2.0 * np.pi * cs

    def adjoint(x):
        behind = np.cumsum(x[:, ::-1], axis=1)[:, ::-1]
        out = np.zeros((B, T, K))
        np.add.at(out, (rows, x0[None]), behind * v0[None, :, None])
        np.add.at(out, (rows, x1[None]), behind * v1[None, :, None])
        return out

    grad_f = np.where(d["valid"], adjoint(q) / sample_rate, 0.0)
    bound_f = np.where(d["valid"], (adjoint(absq * d["e_sin"]) + (hop + K + R_BACKWARD) * EPS * adjoint(absq)) / sample_rate, 0.0)
    return dict(grad_f=grad_f, grad_c=grad_c, grad_a=grad_a.reshape(B, T, 1), bound_f=bound_f, bound_c=bound_c,
                bound_a=bound_a.reshape(B, T, 1))
