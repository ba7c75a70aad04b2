"""Band-limited wavetables (include/ddsp_hip.h: ddsp_wavetable_mip_*, ddsp_wavetable_*_bl) as plain numpy in
fp64, on top of tests/wavetable_reference.py: the Dirichlet kernels, the mip levels and their adjoint, the level rule, the forward,
the analytic gradients, and per-element error bounds with the kernels' roundings counted.

fp32 BY DEFINITION, and emulated as fp32: everything wavetable_reference.py emulates (the increment u among it), the kernels
D = fl32(D64), and the level rule -- r = L u (exact: L is a power of two), r = m 2^e, q = e, t = 2 m - 1 (both exact).

The bounds.
  build     (L + 2) 2^-24 sum_i |W[k,i]| |D[q,(j-i) mod L]|: L fused multiply-adds, each rounding a partial sum that is at most the
            sum of the absolute terms, and 2 for their second order.  Level 0 is a copy: bound 0.
  adjoint   (L + Q + 2) 2^-24 sum |terms|: the L multiply-adds of a level, the Q additions of the levels' sums to grad_M[0].
  forward   wavetable_reference's (N + 14) 2^-24 A[n] + E_phase becomes (2 N + 16) 2^-24 A[n] + E_phase: every table contributes two
            interpolated entries (2 N table terms), and the blend s_k = fma(t, l1, fl((1 - t) l0)) adds two roundings to the twelve
            of the unlimited forward (1 - t is exact).  A[n] takes (1 - t) max|M[q] entries| + t max|M[q+1] entries| for |s_k|, and
            E_phase the same blend of the two levels' slopes.
  backward  (S + N + 18) 2^-24 sum |terms| + the phase terms: R_BACKWARD's sixteen, the blend's two roundings in s_k (grad_c, grad_a)
            or the product of the scatter weight with 1 - t or t and its own rounding (grad_M).
"""
import numpy as np

import wavetable_reference as ref

EPS = ref.EPS
R_FORWARD_BL = ref.R_FORWARD + 2
R_BACKWARD_BL = ref.R_BACKWARD + 2
MIN_SIZE, MAX_SIZE = 16, 4096


def levels_of(L):
    """Q + 1 for a power of two 16 <= L <= 4096, else ValueError"""
    if L < MIN_SIZE or L > MAX_SIZE or L & (L - 1):
        raise ValueError(f"band-limited tables need a power of two 16 <= L <= 4096, got {L}")
    return int(L).bit_length()


def top_harmonic(q, L):
    """H_q: the highest harmonic level q >= 1 keeps"""
    return L >> (q + 1)


def dirichlet64(L):
    """D64 [Q + 1, L] fp64; row 0 is zero (unused)"""
    n = levels_of(L)
    j = np.arange(L, dtype=np.float64)
    D = np.zeros((n, L))
    for q in range(1, n):
        h = np.arange(1, top_harmonic(q, L) + 1, dtype=np.float64)[:, None]
        D[q] = (1.0 + 2.0 * np.cos(2.0 * np.pi * h * j[None, :] / L).sum(0)) / L
    return D


def dirichlet(L):
    """D [Q + 1, L]: what the kernel is given, fp32"""
    return dirichlet64(L).astype(np.float32)


def _circulant(row):
    """C[j, i] = row[(j - i) mod L]"""
    L = row.shape[0]
    idx = (np.arange(L)[:, None] - np.arange(L)[None, :]) % L
    return row[idx]


def build(W, D=None):
    """W [N, L] fp32 -> (M [Q+1, N, L] fp64 from the fp32 kernels D, bound [Q+1, N, L])"""
    W = np.asarray(W, np.float64)
    N, L = W.shape
    D = np.asarray(dirichlet(L) if D is None else D, np.float64)
    n = D.shape[0]
    M, bound = np.zeros((n, N, L)), np.zeros((n, N, L))
    M[0] = W
    for q in range(1, n):
        C = _circulant(D[q])
        M[q] = W @ C.T
        bound[q] = (L + 2) * EPS * (np.abs(W) @ np.abs(C).T)
    return M, bound


def adjoint(G, D=None):
    """G [Q+1, N, L] -> (grad_W [N, L] fp64, bound [N, L])"""
    G = np.asarray(G, np.float64)
    n, N, L = G.shape
    D = np.asarray(dirichlet(L) if D is None else D, np.float64)
    out, mag = G[0].copy(), np.abs(G[0])
    for q in range(1, n):
        C = _circulant(D[q])                    # out[i] += sum_j G[q, j] D[q, (j - i) mod L] = G[q] @ C
        out += G[q] @ C
        mag += np.abs(G[q]) @ np.abs(C)
    return out, (L + (n - 1) + 2) * EPS * mag


def rfft_levels(W):
    """The exact projections: level q keeps the mean and the harmonics h <= H_q (q >= 1); level 0 is W"""
    W = np.asarray(W, np.float64)
    N, L = W.shape
    n = levels_of(L)
    M = np.zeros((n, N, L))
    M[0] = W
    F = np.fft.rfft(W, axis=1)
    for q in range(1, n):
        keep = F.copy()
        keep[:, top_harmonic(q, L) + 1:] = 0.0
        M[q] = np.fft.irfft(keep, n=L, axis=1)
    return M


def build_fp32_model(W, D=None):
    """The direct sum as the kernel runs it: fp32, i ascending, one rounding (a fused multiply-add) per step"""
    W32 = np.asarray(W, np.float32)
    N, L = W32.shape
    D = np.asarray(dirichlet(L) if D is None else D, np.float32)
    n = D.shape[0]
    M = np.zeros((n, N, L), np.float32)
    M[0] = W32
    j = np.arange(L)
    for q in range(1, n):
        acc = np.zeros((N, L), np.float64)
        for i in range(L):
            acc = (acc + W32[:, i:i + 1].astype(np.float64) * D[q][(j - i) % L].astype(np.float64)[None, :]).astype(np.float32).astype(np.float64)
        M[q] = acc.astype(np.float32)
    return M


def level_weights(u, L):
    """u: fp32 increments (as fp64 values) -> (q, q1, t): the two levels of every sample and the weight of the upper one"""
    n = levels_of(L)
    top = n - 1
    r = np.asarray(u, np.float64) * L                           # exact
    q = np.zeros(r.shape, np.int64)
    t = np.zeros(r.shape)
    on = r > 0.5                                                # (False for NaN)
    with np.errstate(invalid="ignore"):
        high = on & ~(r < L / 2)                                # e >= Q is r >= 2^(Q-1); an infinite r too
    m, e = np.frexp(np.where(on & ~high, r, 1.0))               # r = m 2^e, m in [0.5, 1)
    q[on] = e[on]
    t[on] = 2.0 * m[on] - 1.0
    q[high] = top
    t[high] = 0.0
    q1 = np.where(on, np.minimum(q + 1, top), 1)
    return q, q1, t


def _setup(f0, c, a, M, hop, sample_rate, P0):
    M64 = np.asarray(M, np.float64)
    d = ref._setup(f0, c, a, M64[0], hop, sample_rate, P0)
    L, N = d["L"], d["N"]
    f0 = np.asarray(f0, np.float32).reshape(c.shape[0], c.shape[1])
    u = ref.increments(f0, hop, sample_rate)
    q, q1, t = level_weights(u, L)
    k = np.arange(N)[None, None, :]
    j, j1, fr = d["j"][..., None], d["j1"][..., None], d["fr"][..., None]

    def read(lv):
        lo, hi = M64[lv[..., None], k, j], M64[lv[..., None], k, j1]
        diff = np.abs(np.roll(M64, -1, axis=2) - M64)
        slope = np.maximum(np.maximum(diff[lv[..., None], k, (j - 1) % L], diff[lv[..., None], k, j]), diff[lv[..., None], k, (j + 1) % L])
        return lo + fr * (hi - lo), np.maximum(np.abs(lo), np.abs(hi)), slope

    l0, max0, slope0 = read(q)
    l1, max1, slope1 = read(q1)
    tt = t[..., None]
    d.update(q=q, q1=q1, t=t, s=(1.0 - tt) * l0 + tt * l1, smax=(1.0 - tt) * max0 + tt * max1, slope=(1.0 - tt) * slope0 + tt * slope1,
             levels=M64.shape[0])
    return d


def forward(f0, c, a, M, hop, sample_rate, P0=None):
    """M [Q+1, N, L] fp32 (the levels the kernel is given) -> (y [B, T hop] fp64, bound, end phase [B])"""
    d = _setup(f0, c, a, M, hop, sample_rate, P0)
    y = d["au"] * (d["m"] * d["s"]).sum(-1)
    A = np.abs(d["au"]) * (np.abs(d["m"]) * d["smax"]).sum(-1)
    delta = ref.PHASE_EPS * (np.abs(d["P"]) + 1.0) * d["L"]
    E = np.abs(d["au"]) * (np.abs(d["m"]) * d["slope"]).sum(-1) * delta
    end = d["P"][:, -1] - np.floor(d["P"][:, -1])
    return y, (2 * d["N"] + R_FORWARD_BL) * EPS * A + E, end


def backward(grad_y, f0, c, a, M, hop, sample_rate, P0=None):
    """-> dict(grad_c, grad_a, grad_M [Q+1, N, L]: fp64; bound_c, bound_a, bound_M)"""
    d = _setup(f0, c, a, M, hop, sample_rate, P0)
    B, T, N, L, n = d["B"], d["T"], d["N"], d["L"], d["levels"]
    gy = np.asarray(grad_y, np.float64)
    i0, i1, w0, w1 = d["i0"], d["i1"], d["w0"], d["w1"]
    qv = gy * d["au"]
    smax, slope = d["smax"], d["slope"]
    delta = ref.PHASE_EPS * (np.abs(d["P"]) + 1.0) * L
    rows = np.arange(B)[:, None]

    def to_frames(x):
        out = np.zeros((B, T) + x.shape[2:])
        shape = (1, -1) + (1,) * (x.ndim - 2)
        np.add.at(out, (rows, i0[None]), x * w0.reshape(shape))
        np.add.at(out, (rows, i1[None]), x * w1.reshape(shape))
        return out

    reach = np.zeros((B, T))
    np.add.at(reach, (rows, np.broadcast_to(i0[None], (B, T * hop))), 1.0)
    np.add.at(reach, (rows, np.broadcast_to(i1[None], (B, T * hop))), 1.0)
    R = N + R_BACKWARD_BL

    Mix = (d["m"] * d["s"]).sum(-1)
    grad_a = to_frames(gy * Mix)
    abs_a = to_frames(np.abs(gy) * (np.abs(d["m"]) * smax).sum(-1))
    ph_a = to_frames(np.abs(gy) * (np.abs(d["m"]) * slope).sum(-1) * delta)
    bound_a = (reach + R) * EPS * abs_a + ph_a

    G = to_frames(qv[..., None] * d["s"])
    absG = to_frames(np.abs(qv)[..., None] * smax)
    phG = to_frames((np.abs(qv) * delta)[..., None] * slope)
    S, wn = d["S"][..., None], d["wn"]
    grad_c = (G - (G * wn).sum(-1, keepdims=True)) / S
    abs_c = (absG + (absG * np.abs(wn)).sum(-1, keepdims=True)) / np.abs(S)
    ph_c = (phG + (phG * np.abs(wn)).sum(-1, keepdims=True)) / np.abs(S)
    bound_c = (reach[..., None] + R) * EPS * abs_c + ph_c

    grad_M, abs_M, ph_M, touch = (np.zeros((n, N, L)) for _ in range(4))
    k = np.broadcast_to(np.arange(N)[None, None, :], d["m"].shape)
    qm = qv[..., None] * d["m"]
    for lv, lw in ((d["q"], 1.0 - d["t"]), (d["q1"], d["t"])):
        lvb = np.broadcast_to(lv[..., None], d["m"].shape)
        for idx, wgt in ((d["j"], 1.0 - d["fr"]), (d["j1"], d["fr"])):
            e = np.broadcast_to(idx[..., None], d["m"].shape)
            w = (wgt * lw)[..., None]
            np.add.at(grad_M, (lvb, k, e), qm * w)
            np.add.at(abs_M, (lvb, k, e), np.abs(qm) * w)
            np.add.at(touch, (lvb, k, e), 1.0)
        for off in (-1, 0, 1, 2):
            e = np.broadcast_to(((d["j"] + off) % L)[..., None], d["m"].shape)
            np.add.at(ph_M, (lvb, k, e), np.abs(qm) * (delta * lw)[..., None])
    bound_M = (touch + N + R_BACKWARD_BL) * EPS * abs_M + ph_M
    return dict(grad_c=grad_c, grad_a=grad_a.reshape(B, T, 1), grad_M=grad_M, bound_c=bound_c, bound_a=bound_a.reshape(B, T, 1),
                bound_M=bound_M)
