"""fp64 reference, fp32 restatements, cases, inputs, bounds and device launchers for the six entry points of the reverb
(csrc/ddsp_reverb.hip: ddsp_reverb_impulse, ddsp_reverb_impulse_backward, ddsp_spectral_mul, ddsp_spectral_mul_backward,
ddsp_reverb_live with ddsp_reverb_live_scratch_bytes) and for the module path around rocFFT (reverb._ReverbFunction).  Used by
tests/test_gpu_reverb_stages.py (on the device) and tests/test_reverb_reference_host.py (the reference, the restatements and the
bounds themselves, without a device).

The reference is numpy in float64 / complex128 computed FROM the fp32 inputs the device is given; nothing in it is an FFT: the
convolutions, correlations and their gradients are direct sums.  Every reference value comes with a COMPANION, the same sum with
every term replaced by its absolute value, and every check is

    |got - ref| <= K * U * S + FLOOR        per element, U = 2^-24, S the element's own companion (never a global maximum)

so a kernel that is wrong only where the signal is small is out of bound there.  FLOOR = 2^-109 is 2^17 times the smallest
normal fp32 number: a product that underflows may be flushed (at most 2^-126 each), and no sum here has more than 2^17 terms.

What an envelope tap costs.  env = exp(arg), arg = ((-softplus(-decay)) * t) * 500: a relative error e of arg is an error
|arg| e of env.  So wherever a tap enters, its companion carries the weight (1 + |arg|): S = |imp| (1 + |arg|) for the impulse,
and the same weight on the taps inside the sums of the other stages.

K.  The arithmetic part of K is counted below; the ulp error of the device's expf / log1pf and of rocFFT's fp32 transforms is not
known here and is neither assumed nor fitted to the device.  Instead every stage is restated in numpy float32 in the kernel's
order of operations (the FFT path: torch's CPU fp32 transforms at the same length, reverb.fft_length), and the host test measures
the restatement's worst error over exactly the cases the GPU test runs, in units of U * S.  Then

    K = max(derived, 4 * measured)

(4: device math functions and rocFFT may differ from glibc / numpy / the CPU transforms by a few ulp per call).  The measured
column below is asserted by the host test to be at least what it measures (recorded with some headroom, as numpy's float32 exp /
log1p differ between CPU generations); the GPU tests print the device's own figure beside K (`pytest -s`).

  derived counts (each rounded operation at most U of its result, results at most the companion):
    impulse      on the |arg| part: the two products of arg (2); on the rest: exp's result, noise * env, * sg, and the
                 sigmoid's add and divide (4, plus the library's share)  ->  4 of S = |imp| (1 + |arg|)
    bwd_noise    g * env, * sg, sg's add and divide: 4, and 2 on the |arg| part  ->  4
    bwd_decay    per term g * noise, * env, * sg, t * 500 (4), the fp64 sum (nothing), dsp's add and divide and the final
                 product rounded to fp32 (3), 2 on the |arg| part  ->  8 (7 rounded up)
    bwd_wet      per term g * noise, * env (2), sg's add and divide (2) which 1 - sg sees magnified by sg / (1 - sg) = e^wet
                 <= 1.35 at the wets used (3), the subtraction, the product sg (1 - sg) and the final rounding (3)  ->  8
    mul, bwd_gk  a complex product: two products and one addition per component, (1 + U)^2 - 1 < 2.01 U  ->  4
    bwd_s        per row two products and an addition (2 U of the row's terms), then `rows` sequential additions onto the
                 accumulator (at most rows U of the whole)  ->  rows + 3
    live         128 sequential FMAs per chain (128), 2 combining additions, `chunks` additions in the finish kernel, plus
                 the taps' own relative error K(impulse) on S = sum |imp| (1 + |arg|) |window|  ->  130 + chunks + K(impulse)
    mod_*        the module path: impulse, rfft, spectral product, irfft (and back).  The transforms' error is normwise, not
                 elementwise, so nothing is derived beyond the spectral arithmetic (4, rows + 3); the measured column decides.

---- table: stage, derived, measured (units of U * S, rounded up by a quarter or so), K ----
    impulse          4            5.5       22
    bwd_noise        4            6.0       24
    bwd_decay        8            1.25      8
    bwd_wet          8            1.0       8
    mul              4            2.01      4
    bwd_gk           4            2.01      4
    bwd_s            rows+3       7.0       rows+3
    live             152+chunks   5.5       152+chunks
    mod_y            4            14.0      56
    mod_grad_x       4            10.5      42
    mod_grad_noise   rows+3       16.0      64
    mod_grad_decay   rows+3       0.1       rows+3
    mod_grad_wet     rows+3       0.05      rows+3
---- end of table ----
(measured on the host: impulse 4.26, bwd_noise 4.70, bwd_decay 0.95, bwd_wet 0.81, mul 1.95, bwd_gk 1.98, bwd_s 6.66 at 33 rows,
live 4.23, mod_y 10.84, mod_grad_x 8.01, mod_grad_noise 12.53, mod_grad_decay 0.05, mod_grad_wet 0.02.  mul, bwd_gk and bwd_s
call no library: their K is the derived count alone, and the restatement, all IEEE operations, must stay within it.  The impulse
figures above 4 come from the extreme decays, where |arg| reaches 87 and softplus's own error joins the two products of arg.)

Parameter sets (PARAMS).  Every case uses a decay at which every tap counts: the envelope at the last tap (t -> 1) is
    name          decay  wet    envelope at t = 1     sigmoid(wet)
    slow_wet      8      0.3    0.85                  0.57
    slow_dry      8      -2     0.85                  0.12
    default_wet   5      0.3    0.035                 0.57     (5: the reference's default)
    default_dry   5      -2     0.035                 0.12
EXTREME_DECAY and EXTREME_WET (both softplus branches, the far ends of the sigmoid, underflowing taps) are used only by the
impulse kernel's test and, the decays, by the impulse backward's.  The noise taps are +-[0.25, 1): none is small, so a dropped tap
is always visible against its neighbours."""
import math
import re

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -109
TILE_J, TILE_M = 256, 512                    # reverb_live_partial_kernel: outputs by taps per workgroup
CAP_IMPULSE = CAP_SPECTRAL_BWD = 4096        # workgroups of 256 threads beyond which the kernels stride
CAP_SPECTRAL_MUL = 8192
CAP_LIVE_FINISH = 256
EINVAL, ERANGE = -1, -2
GUARD = 64                                   # floats behind every output that no kernel may touch
SENTINEL = 0x7FA5A5A5                        # (a NaN with a payload: no kernel produces it)

PARAMS = {"slow_wet": (8.0, 0.3), "slow_dry": (8.0, -2.0), "default_wet": (5.0, 0.3), "default_dry": (5.0, -2.0)}
EXTREME_DECAY = (-100.0, -25.0, -20.0, 0.0, 5.0, 8.0, 20.0, 25.0, 100.0)
EXTREME_WET = (-30.0, -2.0, 0.3, 30.0)

f32 = np.float32


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _table():
    body = __doc__.split("---- table:")[1].split("---- end of table ----")[0]
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"^\s{4}(\w+)\s+\S+\s+([0-9.]+)\s+\S+\s*$", body, re.M)}


MEASURED = _table()
STAGES = ("impulse", "bwd_noise", "bwd_decay", "bwd_wet", "mul", "bwd_gk", "bwd_s", "live", "mod_y", "mod_grad_x", "mod_grad_noise",
          "mod_grad_decay", "mod_grad_wet")


def derived(stage, rows=1, chunks=1):
    """The counted part of K (module docstring)."""
    if stage in ("impulse", "bwd_noise", "mul", "bwd_gk", "mod_y", "mod_grad_x"):
        return 4.0
    if stage in ("bwd_decay", "bwd_wet"):
        return 8.0
    if stage in ("bwd_s", "mod_grad_noise", "mod_grad_decay", "mod_grad_wet"):
        return rows + 3.0
    if stage == "live":
        return 130.0 + chunks + K("impulse")
    raise KeyError(stage)


def K(stage, rows=1, chunks=1):
    if stage in ("mul", "bwd_gk", "bwd_s"):                      # no library call
        return derived(stage, rows, chunks)
    return max(derived(stage, rows, chunks), 4.0 * MEASURED[stage])


def figure(got, ref, S):
    """The worst (|got - ref| - FLOOR)+ / (U S) over the elements: the check `|got - ref| <= K U S + FLOOR` is `figure <= K`.
    inf where S == 0 and the error is above the floor; nan (which fails every comparison) where `got` is not finite."""
    got, ref, S = np.asarray(got), np.asarray(ref), np.asarray(S)
    if np.iscomplexobj(ref):
        got = np.ascontiguousarray(got, dtype=np.complex128).view(np.float64)
        ref = np.ascontiguousarray(ref, dtype=np.complex128).view(np.float64)
        S = np.ascontiguousarray(S, dtype=np.complex128).view(np.float64)
    over = np.maximum(np.abs(f64(got) - f64(ref)) - FLOOR, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(over == 0.0, 0.0, over / (U * f64(S)))
    return float(np.max(r, initial=0.0))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the reference ----------------------------------------------------------------------------------------------------------
def softplus(x):
    """ATen: x above the threshold 20, log1p(exp(x)) otherwise."""
    x = float(x)
    return x if x > 20.0 else math.log1p(math.exp(x))


def sigmoid(x):
    return 1.0 / (1.0 + math.exp(-float(x)))


def envelope(decay, t):
    """(exp(arg), arg), arg[i] = -softplus(-decay) * t[i] * 500."""
    arg = -softplus(-float(decay)) * f64(t) * 500.0
    return np.exp(arg), arg


def impulse(noise, decay, wet, t, n_out):
    """-> (impulse [n_out], arg [length]): noise * envelope * sigmoid(wet), tap 0 forced to 1, zero-padded or cropped."""
    env, arg = envelope(decay, t)
    imp = f64(noise) * env * sigmoid(wet)
    imp[0] = 1.0
    out = np.zeros(n_out)
    m = min(n_out, imp.shape[0])
    out[:m] = imp[:m]
    return out, arg


def tap_weights(imp, arg):
    """|imp| (1 + |arg|) on the taps imp has: the companion of the impulse, and the taps' weight in every sum over them."""
    m = min(imp.shape[0], arg.shape[0])
    w = np.abs(f64(imp)).copy()
    w[:m] *= 1.0 + np.abs(arg[:m])
    return w


def impulse_backward(g, noise, decay, wet, t, n_used):
    """-> dict(noise [length], decay, wet, S_noise [length], A_decay, A_wet): the analytic gradient of impulse()[:n_used] under
    the cotangent g [n_used], and the companions (absolute terms, each with the tap's weight 1 + |arg|)."""
    noise = f64(noise)
    length = noise.shape[0]
    env, arg = envelope(decay, t)
    sg = sigmoid(wet)
    gg = np.zeros(length)
    gg[1:n_used] = f64(g)[1:n_used]                              # tap 0 is the constant 1; taps >= n_used were cropped away
    wgt = 1.0 + np.abs(arg)
    d_noise = gg * env * sg
    tw = gg * noise * env
    dsp = 1.0 if -float(decay) > 20.0 else sigmoid(-float(decay))
    td = tw * sg * f64(t) * 500.0
    return dict(noise=d_noise, decay=dsp * td.sum(), wet=sg * (1.0 - sg) * tw.sum(), S_noise=np.abs(d_noise) * wgt,
                A_decay=dsp * (np.abs(td) * wgt).sum(), A_wet=sg * (1.0 - sg) * (np.abs(tw) * wgt).sum())


def _products(a, b):
    """a * b in complex128 and the componentwise sums of absolute products, packed as a complex array (re: |ar br| + |ai bi|,
    im: |ar bi| + |ai br|; the same for a conj(b))."""
    ar, ai, br, bi = np.abs(a.real), np.abs(a.imag), np.abs(b.real), np.abs(b.imag)
    return (ar * br + ai * bi) + 1j * (ar * bi + ai * br)


def spectral_mul(X, Kf):
    """-> (Y, S): Y[r, f] = X[r, f] K[f]."""
    X, Kf = np.asarray(X, dtype=np.complex128), np.asarray(Kf, dtype=np.complex128)
    return X * Kf[None], _products(X, Kf[None])


def spectral_mul_backward(G, X, Kf):
    """-> (GK, S, A_GK, A_S): GK[r, f] = G[r, f] conj(K[f]); S[f] = sum_r G[r, f] conj(X[r, f]) (X None: no S)."""
    G, Kf = np.asarray(G, dtype=np.complex128), np.asarray(Kf, dtype=np.complex128)
    GK, A_GK = G * np.conj(Kf)[None], _products(G, Kf[None])
    if X is None:
        return GK, None, A_GK, None
    X = np.asarray(X, dtype=np.complex128)
    return GK, (G * np.conj(X)).sum(axis=0), A_GK, _products(G, X).sum(axis=0)


def slide(x, hist):
    """The slid window [hist[n:], x] in the inputs' own dtype (fp32 in, the exact fp32 values out)."""
    return np.concatenate([np.asarray(hist)[np.asarray(x).shape[0]:], np.asarray(x)])


def live(x, hist, imp, weights=None):
    """-> (y [n], A [n], window [L]): y[j] = sum_m imp[m] window[L - n + j - m] by direct sums; A the same with |imp| (or
    `weights`, the taps' tap_weights) and |window|; window the slid history, exact."""
    n, L = np.asarray(x).shape[0], np.asarray(hist).shape[0]
    window = slide(x, hist)
    w, imp = f64(window), f64(imp)
    wa, ia = np.abs(w), np.abs(imp) if weights is None else f64(weights)
    y, A = np.zeros(n), np.zeros(n)
    for j in range(n):
        i = L - n + j
        y[j] = imp[:i + 1] @ w[i::-1]
        A[j] = ia[:i + 1] @ wa[i::-1]
    return y, A, window


def forward(x, imp_used, weights=None):
    """-> (y [rows, n], A): the first n samples of x * imp_used, tap by tap."""
    x, k = f64(x), f64(imp_used)
    ka = np.abs(k) if weights is None else f64(weights)
    n = x.shape[1]
    y, A = np.zeros(x.shape), np.zeros(x.shape)
    for m in range(min(k.shape[0], n)):
        y[:, m:] += k[m] * x[:, :n - m]
        A[:, m:] += ka[m] * np.abs(x[:, :n - m])
    return y, A


def forward_grad_x(g, imp_used, weights=None):
    """-> (grad_x [rows, n], A): grad_x[r, j] = sum_m imp[m] g[r, j + m], the correlation with the taps."""
    g, k = f64(g), f64(imp_used)
    ka = np.abs(k) if weights is None else f64(weights)
    n = g.shape[1]
    gx, A = np.zeros(g.shape), np.zeros(g.shape)
    for m in range(min(k.shape[0], n)):
        gx[:, :n - m] += k[m] * g[:, m:]
        A[:, :n - m] += ka[m] * np.abs(g[:, m:])
    return gx, A


def forward_grad_imp(g, x, used):
    """-> (grad_imp [used], A): grad_imp[m] = sum_r sum_j g[r, j + m] x[r, j], the row-summed correlation with x."""
    g, x = f64(g), f64(x)
    n = x.shape[1]
    gi, A = np.zeros(used), np.zeros(used)
    for m in range(used):
        gi[m] = (g[:, m:] * x[:, :n - m]).sum()
        A[m] = np.abs(g[:, m:] * x[:, :n - m]).sum()
    return gi, A


def module_reference(x, w, noise, decay, wet, t):
    """The module path y = forward(x), loss = sum(y w), in fp64 by direct sums -> dict of (value, companion) per stage mod_*.
    The companions of the parameter gradients carry the companion of grad_imp, not |grad_imp|: grad_imp comes out of the
    transforms with an error relative to its terms, whatever cancels in their sum."""
    n, used = x.shape[1], min(noise.shape[0], x.shape[1])
    imp, arg = impulse(noise, decay, wet, t, used)
    tw = tap_weights(imp, arg)
    gi, A_gi = forward_grad_imp(w, x, used)
    b = impulse_backward(gi, noise, decay, wet, t, used)
    c = impulse_backward(A_gi, np.abs(f64(noise)), decay, wet, t, used)
    return dict(mod_y=forward(x, imp, tw), mod_grad_x=forward_grad_x(w, imp, tw), mod_grad_noise=(b["noise"], c["S_noise"]),
                mod_grad_decay=(b["decay"], c["A_decay"]), mod_grad_wet=(b["wet"], c["A_wet"]), imp=imp, n=n, used=used)


# ---- the fp32 restatements (numpy float32, the kernels' order of operations) --------------------------------------------------
def softplus_f32(x):
    x = f32(x)
    return x if x > f32(20.0) else np.log1p(np.exp(x))


def sigmoid_f32(x):
    with np.errstate(over="ignore"):
        return f32(1.0) / (f32(1.0) + np.exp(-f32(x)))


def envelope_f32(decay, t):
    neg_sp = -softplus_f32(-f32(decay))
    with np.errstate(under="ignore"):
        return np.exp((neg_sp * np.asarray(t, dtype=f32)) * f32(500.0))


def impulse_f32(noise, decay, wet, t, n_out):
    with np.errstate(under="ignore"):
        imp = (np.asarray(noise, dtype=f32) * envelope_f32(decay, t)) * sigmoid_f32(wet)
    imp[0] = 1.0
    out = np.zeros(n_out, f32)
    m = min(n_out, imp.shape[0])
    out[:m] = imp[:m]
    return out


def impulse_backward_f32(g, noise, decay, wet, t, n_used):
    """-> (grad_noise [length], grad_decay, grad_wet) as the kernel forms them: fp32 terms, fp64 sums, one rounding at the end."""
    noise, t = np.asarray(noise, dtype=f32), np.asarray(t, dtype=f32)
    length = noise.shape[0]
    env, sg = envelope_f32(decay, t), sigmoid_f32(wet)
    gg = np.zeros(length, f32)
    gg[1:n_used] = np.asarray(g, dtype=f32)[1:n_used]
    with np.errstate(under="ignore"):
        gn = gg * env * sg
        gne = gg * noise * env
        s_wet = f64(gne).sum()
        s_dec = (f64(gne * sg) * f64(t * f32(500.0))).sum()
    d = f32(decay)
    dsp = f32(1.0) if -d > f32(20.0) else sigmoid_f32(-d)
    return gn, f32(s_dec * float(dsp)), f32(s_wet * float(sg * (f32(1.0) - sg)))


def _c64_parts(a):
    a = np.asarray(a, dtype=np.complex64)
    return a.real.astype(f32), a.imag.astype(f32)


def spectral_mul_f32(X, Kf):
    xr, xi = _c64_parts(X)
    kr, ki = _c64_parts(np.asarray(Kf)[None])
    return ((xr * kr - xi * ki) + 1j * (xr * ki + xi * kr)).astype(np.complex64)


def spectral_mul_backward_f32(G, X, Kf):
    """-> (GK, S) (S None without X); the rows of S summed in order, as the kernel's loop does."""
    gr, gi = _c64_parts(G)
    kr, ki = _c64_parts(np.asarray(Kf)[None])
    GK = ((gr * kr + gi * ki) + 1j * (gi * kr - gr * ki)).astype(np.complex64)
    if X is None:
        return GK, None
    xr, xi = _c64_parts(X)
    sr, si = np.zeros(gr.shape[1], f32), np.zeros(gr.shape[1], f32)
    for r in range(gr.shape[0]):
        sr = sr + (gr[r] * xr[r] + gi[r] * xi[r])
        si = si + (gi[r] * xr[r] - gr[r] * xi[r])
    return GK, (sr + 1j * si).astype(np.complex64)


def live_f32(x, hist, imp32):
    """-> y [n] float32: per chunk of 512 taps four FMA chains over the taps m = 0, 1, 2, 3 (mod 4), combined as (a0 + a1) +
    (a2 + a3); the chunks added in order.  (The FMA is one fp64 product-and-add rounded to fp32: the product is exact in fp64.)"""
    window = slide(x, hist)
    n, L = np.asarray(x).shape[0], window.shape[0]
    chunks = -(-L // TILE_M)
    off = chunks * TILE_M
    wpad = np.zeros(off + L)
    wpad[off:] = window
    i = off + L - n + np.arange(n)
    imp = f64(imp32)
    y = np.zeros(n, f32)
    for c in range(chunks):
        acc = np.zeros((4, n), f32)
        for m in range(c * TILE_M, min(L, (c + 1) * TILE_M)):
            acc[m % 4] = (imp[m] * wpad[i - m] + acc[m % 4]).astype(f32)
        y = y + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return y


def module_f32(x, w, noise, decay, wet, t, nfft):
    """reverb._ReverbFunction forward and backward with torch's CPU fp32 transforms at `nfft` and the restated stages between
    them -> dict(mod_y, mod_grad_x, mod_grad_noise, mod_grad_decay, mod_grad_wet)."""
    import torch
    n, used = x.shape[1], min(noise.shape[0], x.shape[1])

    def rfft(a):
        return torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(a, dtype=f32)), n=nfft).numpy()

    def irfft(a):
        return torch.fft.irfft(torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex64)), n=nfft).numpy()

    ks, xs, gs = rfft(impulse_f32(noise, decay, wet, t, used)), rfft(x), rfft(w)
    y = irfft(spectral_mul_f32(xs, ks))[:, :n]
    gk, s = spectral_mul_backward_f32(gs, xs, ks)
    gn, gd, gw = impulse_backward_f32(irfft(s)[:used], noise, decay, wet, t, used)
    return dict(mod_y=y, mod_grad_x=irfft(gk)[:, :n], mod_grad_noise=gn, mod_grad_decay=gd, mod_grad_wet=gw)


# ---- cases and inputs -------------------------------------------------------------------------------------------------------
def reverb_parameters(length, seed):
    """-> (noise, t) float32 [length]: taps +-[0.25, 1), t = i / length as the module's buffer holds it."""
    rng = np.random.default_rng(seed)
    noise = (rng.choice([-1.0, 1.0], length) * (0.25 + 0.75 * rng.random(length))).astype(f32)
    return noise, (np.arange(length, dtype=f32) / f32(length))


def _impulse_shapes():
    out = []
    for length in (1, 2, 255, 256, 257, 1000):
        for n_out in (1, length - 1, length, length + 1, 3 * length):
            if n_out >= 1 and (length, n_out) not in out:
                out.append((length, n_out))
    return out + [(1000, CAP_IMPULSE * 256 + 300)]               # beyond the grid: the first 300 threads walk a second tap


IMPULSE_SHAPES = _impulse_shapes()
IMPULSE_EXTREMES = [(d, w) for d in EXTREME_DECAY for w in EXTREME_WET]     # at length 1000, n_out 1000
IMPULSE_BWD_SHAPES = [(1, 1), (1000, 1), (1000, 999), (1000, 1000), (1025, 300), (2049, 2049), (48000, 48000)]
IMPULSE_BWD_DECAYS = (-100.0, -25.0, -20.0, 20.0, 100.0)         # both sides of `-decay > 20`; wet 0.3; every shape
SPECTRAL_SHAPES = [(1, 1), (1, 2), (3, 257), (32, 1025), (33, CAP_SPECTRAL_MUL * 8 + 1)]       # the last: 33 * 65537 > 8192 * 256
SPECTRAL_BWD_SHAPES = SPECTRAL_SHAPES + [(1, CAP_SPECTRAL_BWD * 256 + 5)]
LIVE_SHAPES = [(1, 1), (2, 1), (511, 255), (512, 256), (513, 257), (1000, 77), (1025, 1025), (1536, 300), (2049, 513), (70000, 300)]
MODULE_SHAPES = [(512, 300, 3), (512, 512, 1), (512, 700, 2), (500, 1, 2), (1000, 1001, 1)]      # (sr, n, rows), decay 8
GRAD_CONFIGS = ("both", "x", "params", "none")


def impulse_cases(length, n_out):
    """(decay, wet) of one impulse shape: the four named sets; at (1000, 1000) the extremes as well."""
    return list(PARAMS.values()) + (IMPULSE_EXTREMES if (length, n_out) == (1000, 1000) else [])


def impulse_backward_cases(length, n_used):
    """(decay, wet) of one backward shape: the four named sets and both sides of the softplus threshold."""
    return list(PARAMS.values()) + [(d, 0.3) for d in IMPULSE_BWD_DECAYS]


def param_set(k):
    name = list(PARAMS)[k % len(PARAMS)]
    return (name,) + PARAMS[name]


def cotangent(n, seed):
    """A gradient with magnitudes spread over four decades."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-2.0, 2.0, n)).astype(f32)


def spectral_inputs(rows, bins, seed):
    """-> (G, X, K) complex64: rows with magnitudes spread over 1e-6 .. 1e6 (X ascending, G descending), a decade either way from
    bin to bin, K over four decades."""
    rng = np.random.default_rng(seed)

    def c(shape, lo, hi):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 10.0 ** rng.uniform(lo, hi, shape)

    scale = 10.0 ** (np.linspace(-6.0, 6.0, rows) if rows > 1 else np.zeros(1))[:, None]
    X = (c((rows, bins), -1.0, 1.0) * scale).astype(np.complex64)
    G = (c((rows, bins), -1.0, 1.0) * scale[::-1]).astype(np.complex64)
    return G, X, c((bins,), -2.0, 2.0).astype(np.complex64)


def live_inputs(L, n, seed):
    """-> (hist0 [L], [x_0, x_1, x_2]) float32.  The last tap meets one sample of one output per callback: window[0] under
    y[n - 1], which is sample (k + 1) n of the stream [hist0, x_0, x_1, x_2] in callback k.  Those three samples are loud
    (+-[1, 2)) on a quiet background (history 1e-3, blocks 1e-2), with sixteen more loud clicks scattered over the history -- so
    one dropped tap stands far above the bound of that output.  x_2 is scaled by 1e-6 as a whole: a quiet block after loud
    ones, whose outputs are bound relative to their own terms.  n == L: no history sample survives: hist0 is NaN."""
    rng = np.random.default_rng(seed)

    def loud(k):
        return rng.choice([-1.0, 1.0], k) * (1.0 + rng.random(k))

    stream = np.concatenate([1e-3 * rng.standard_normal(L), 1e-2 * rng.standard_normal(3 * n)])
    clicks = rng.integers(0, L, 16)
    stream[clicks] = loud(16)
    stream[[n, 2 * n, 3 * n]] = loud(3)
    stream[L + 2 * n:] *= 1e-6
    if n == L:
        stream[:L] = np.nan
    stream = stream.astype(f32)
    return stream[:L], [stream[L + k * n:L + (k + 1) * n] for k in range(3)]


def module_inputs(sr, n, rows, seed):
    """-> (x, w [rows, n], noise, t [sr]) float32: x and the loss weights w (loss = sum y w) dense noise at 0.1 with a loud first
    column of x and last column of w (the samples the tap at the crop boundary meets)."""
    rng = np.random.default_rng(seed)
    x, w = 0.1 * rng.standard_normal((rows, n)), 0.1 * rng.standard_normal((rows, n))
    x[:, 0] = rng.choice([-1.0, 1.0], rows) * (1.0 + rng.random(rows))
    w[:, -1] = rng.choice([-1.0, 1.0], rows) * (1.0 + rng.random(rows))
    noise, t = reverb_parameters(sr, seed + 1)
    return x.astype(f32), w.astype(f32), noise, t


# ---- the checks, on the device's output or on a restatement's ---------------------------------------------------------------
class Figures(dict):
    """stage -> the worst figure seen, and the K it was held to."""

    def take(self, stage, fig, k):
        old = self.get(stage, (0.0, k))
        self[stage] = (fig if not fig <= old[0] else old[0], max(k, old[1]))     # (nan sticks)
        return fig <= k

    def line(self, tag):
        return f"RVB {tag}: " + ", ".join(f"{s} {v[0]:.2f} (K {v[1]:g})" for s, v in self.items())


def check_impulse(run, figs, length, n_out, decay, wet, seed=0):
    """run(noise, decay, wet, t, n_out) -> impulse.  Tap 0 exactly 1, the padding exactly +0, the rest in bound."""
    noise, t = reverb_parameters(length, 100 + length + seed)
    got = np.asarray(run(noise, f32(decay), f32(wet), t, n_out))
    ref, arg = impulse(noise, f32(decay), f32(wet), t, n_out)
    ok = got.shape == (n_out,) and got[0] == 1.0 and bool(np.all(bits(got[length:]) == 0))
    return figs.take("impulse", figure(got, ref, tap_weights(ref, arg)), K("impulse")) and ok


def check_impulse_backward(run, figs, length, n_used, decay, wet):
    """run(g, noise, decay, wet, t, n_used) -> (grad_noise, grad_decay, grad_wet).  The exact zeros, then the bounds."""
    noise, t = reverb_parameters(length, 200 + length)
    g = cotangent(n_used, 300 + length + n_used)
    gn, gd, gw = run(g, noise, f32(decay), f32(wet), t, n_used)
    r = impulse_backward(g, noise, f32(decay), f32(wet), t, n_used)
    gn = np.asarray(gn)
    ok = gn.shape == (length,) and bits(gn[:1])[0] == 0 and bool(np.all(bits(gn[n_used:]) == 0))
    ok &= figs.take("bwd_noise", figure(gn, r["noise"], r["S_noise"]), K("bwd_noise"))
    ok &= figs.take("bwd_decay", figure(gd, r["decay"], r["A_decay"]), K("bwd_decay"))
    ok &= figs.take("bwd_wet", figure(gw, r["wet"], r["A_wet"]), K("bwd_wet"))
    return bool(ok)


def check_spectral_mul(run, figs, rows, bins):
    """run(X, K) -> Y"""
    _, X, Kf = spectral_inputs(rows, bins, 400 + rows + bins)
    ref, S = spectral_mul(X, Kf)
    return figs.take("mul", figure(run(X, Kf), ref, S), K("mul"))


def check_spectral_mul_backward(run, figs, rows, bins):
    """run(G, X, K) -> (GK, S)"""
    G, X, Kf = spectral_inputs(rows, bins, 500 + rows + bins)
    GK, S = run(G, X, Kf)
    rGK, rS, A_GK, A_S = spectral_mul_backward(G, X, Kf)
    ok = figs.take("bwd_gk", figure(GK, rGK, A_GK), K("bwd_gk"))
    return bool(ok & figs.take("bwd_s", figure(S, rS, A_S), K("bwd_s", rows=rows)))


def live_case(L, n):
    """The inputs and the reference of the three callbacks of one live case (the parameter sets by turns) -> dict(noise, t,
    decay, wet, hist0, xs, ref: per callback (y, S, window), imp, tw, chunks)."""
    _, decay, wet = param_set(LIVE_SHAPES.index((L, n)))
    noise, t = reverb_parameters(L, 600 + L)
    hist, xs = live_inputs(L, n, 700 + L + n)
    imp, arg = impulse(noise, f32(decay), f32(wet), t, L)
    tw = tap_weights(imp, arg)
    ref, h = [], hist
    for x in xs:
        y, S, h = live(x, h, imp, tw)
        ref.append((y, S, h))
    return dict(noise=noise, t=t, decay=f32(decay), wet=f32(wet), hist0=hist, xs=xs, ref=ref, imp=imp, tw=tw, chunks=-(-L // TILE_M))


def check_live(run, figs, case):
    """run(x, hist, noise, decay, wet, t) -> y, callback by callback from the reference's (exact) history."""
    ok, h = True, case["hist0"]
    for x, (y, S, window) in zip(case["xs"], case["ref"]):
        got = run(x, h, case["noise"], case["decay"], case["wet"], case["t"])
        ok &= figs.take("live", figure(got, y, S), K("live", chunks=case["chunks"]))
        h = window
    return bool(ok)


def module_case(sr, n, rows):
    """-> (x, w, noise, t, wet, module_reference(...)) of one module shape: decay 8, the two wets by turns."""
    k = MODULE_SHAPES.index((sr, n, rows))
    wet = f32((0.3, -2.0)[k % 2])
    x, w, noise, t = module_inputs(sr, n, rows, 800 + k)
    return x, w, noise, t, wet, module_reference(x, w, noise, f32(8.0), wet, t)


def check_module(got, figs, ref, rows):
    """got: dict stage -> array (or None: not asked for) against module_reference's."""
    ok = True
    for stage in ("mod_y", "mod_grad_x", "mod_grad_noise", "mod_grad_decay", "mod_grad_wet"):
        if got.get(stage) is not None:
            ok &= figs.take(stage, figure(got[stage], *ref[stage]), K(stage, rows=rows))
    return bool(ok)


# ---- launching the entry points (needs a device) ------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


class Guarded:
    """`floats` fp32 of output on the device, every word of it and of the GUARD floats behind it set to SENTINEL."""

    def __init__(self, floats):
        torch = _torch()
        self.floats = floats
        self.buf = torch.full((floats + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.floats:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def numpy(self, dtype=np.float32):
        return self.buf[:self.floats].cpu().numpy().view(dtype)


def dev(a):
    """numpy -> a contiguous CUDA tensor of the same dtype (complex64 as interleaved floats); None stays None."""
    torch = _torch()
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    return torch.from_numpy(a.reshape(-1).copy()).cuda()


def _lib():
    import ddsp_pytorch_amd as ddsp
    return ddsp._lib.lib()


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _scalar(v):
    return dev(np.array([v], dtype=np.float32))


def device_impulse(noise, decay, wet, t, n_out):
    """-> (impulse float32 [n_out], guard intact)"""
    a, out = [dev(noise), _scalar(decay), _scalar(wet), dev(t)], Guarded(n_out)
    rc = _lib().ddsp_reverb_impulse(*[v.data_ptr() for v in a], out.ptr(), len(noise), n_out, _stream())
    assert rc == 0, rc
    _torch().cuda.synchronize()
    return out.numpy(), out.intact()


def device_impulse_backward(g, noise, decay, wet, t, n_used):
    """-> (grad_noise [length], grad_decay, grad_wet, guards intact)"""
    a = [dev(g), dev(noise), _scalar(decay), _scalar(wet), dev(t)]
    gn, gd, gw = Guarded(len(noise)), Guarded(1), Guarded(1)
    rc = _lib().ddsp_reverb_impulse_backward(*[v.data_ptr() for v in a], gn.ptr(), gd.ptr(), gw.ptr(), len(noise), n_used, _stream())
    assert rc == 0, rc
    _torch().cuda.synchronize()
    return gn.numpy(), gd.numpy()[0], gw.numpy()[0], gn.intact() and gd.intact() and gw.intact()


def device_spectral_mul(X, Kf):
    """-> (Y complex64 [rows, bins], guard intact)"""
    rows, bins = X.shape
    a, out = [dev(X), dev(Kf)], Guarded(2 * rows * bins)
    rc = _lib().ddsp_spectral_mul(a[0].data_ptr(), a[1].data_ptr(), out.ptr(), rows, bins, _stream())
    assert rc == 0, rc
    _torch().cuda.synchronize()
    return out.numpy(np.complex64).reshape(rows, bins), out.intact()


def device_spectral_mul_backward(G, X, Kf, want_gk=True, want_s=True):
    """-> (GK or None, S or None, guards intact).  X may be None when S is not wanted."""
    rows, bins = G.shape
    a = [dev(G), dev(X), dev(Kf)]
    gk = Guarded(2 * rows * bins) if want_gk else None
    s = Guarded(2 * bins) if want_s else None
    rc = _lib().ddsp_spectral_mul_backward(a[0].data_ptr(), None if a[1] is None else a[1].data_ptr(), a[2].data_ptr(),
                                           None if gk is None else gk.ptr(), None if s is None else s.ptr(), rows, bins, _stream())
    assert rc == 0, rc
    _torch().cuda.synchronize()
    ok = (gk is None or gk.intact()) and (s is None or s.intact())
    return (None if gk is None else gk.numpy(np.complex64).reshape(rows, bins)), (None if s is None else s.numpy(np.complex64)), ok


class LiveDevice:
    """One reverb on the device with two history buffers used in turn, the scratch sized by ddsp_reverb_live_scratch_bytes
    exactly (its guard behind it), y with its guard."""

    def __init__(self, noise, decay, wet, t, n):
        self.L, self.n = len(noise), n
        self.par = [dev(noise), _scalar(decay), _scalar(wet), dev(t)]
        self.hist = [Guarded(self.L), Guarded(self.L)]
        nbytes = _lib().ddsp_reverb_live_scratch_bytes(self.L, n)
        assert nbytes == 4 * (-(-self.L // TILE_M)) * n, nbytes
        self.scratch = Guarded(nbytes // 4)
        self.turn = 0

    def set_history(self, hist):
        self.hist[self.turn].buf[:self.L] = _torch().from_numpy(np.ascontiguousarray(hist, dtype=np.float32).view(np.int32)).cuda()

    def call(self, x):
        """-> (y float32 [n], history_out float32 [L] as written, guards intact); the written history is the next input."""
        torch = _torch()
        xd, y = dev(x), Guarded(self.n)
        hin, hout = self.hist[self.turn], self.hist[1 - self.turn]
        hout.buf[:] = SENTINEL
        rc = _lib().ddsp_reverb_live(xd.data_ptr(), hin.ptr(), hout.ptr(), *[v.data_ptr() for v in self.par], y.ptr(),
                                     self.scratch.ptr(), self.L, self.n, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        self.turn = 1 - self.turn
        return y.numpy(), hout.numpy(), y.intact() and hout.intact() and hin.intact() and self.scratch.intact()
