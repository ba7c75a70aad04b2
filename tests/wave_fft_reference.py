"""fp64 reference, form table and error bounds for the shared one-wavefront FFT (csrc/ddsp_wave_fft.h), as the test hook
ddsp_wfft_probe (csrc/ddsp_wfft_probe.hip, include/ddsp_hip.h) runs it.  Used by tests/test_gpu_wave_fft.py (on the device) and
tests/test_wave_fft_reference_host.py (the reference and the bounds themselves, without a device).

Everything here is float64 / complex128.  Every bound is a function whose docstring holds its derivation from the unit roundoff
`U` = 2^-24 and counted operations; errors of complex numbers are absolute values of complex differences ("normwise")."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32: fl(x) = x (1 + d), |d| <= U; half an ulp of a value in [1, 2)
SINCOSPI_ULP = 2.0             # OCML's documented accuracy of sincospi (fp32), in ulps of each component (the ROCm headers
                               # and documents installed with the toolchain state no other figure); measured: 0.83
CPU_FACTOR = 3.0               # the sharp criterion: at most this many times the CPU fp32 library transform's error

# ---- the forms of ddsp_wfft_probe (include/ddsp_hip.h) ---------------------------------------------------------------------
PAIR_FWD, PAIR_INV = 0, 5
WAVE8_FWD, WAVE8_INV, WAVE8_HALFZERO, WAVE16_FWD, WAVE16_INV, WAVE16_HALFZERO = 10, 11, 12, 13, 14, 15
REAL2048_FWD, REAL2048_INV, TWIDDLES, SCALE, WAVEMAX = 16, 17, 18, 19, 20
TWIDDLE_COUNT = 88
EINVAL, EPERM = -1, -3

# a complex transform form: `n` points, `bt` transforms per unit, `n_in` input points per transform (n / 2: HALFZERO)
Form = namedtuple("Form", "name id n bt inverse n_in")
PAIR_SIZES = (64, 128, 256, 512, 1024)
PAIR_BT = {64: 8, 128: 4, 256: 2, 512: 1, 1024: 1}
COMPLEX_FORMS = tuple(
    [Form(f"pair{n}_{'inv' if inv else 'fwd'}", (PAIR_INV if inv else PAIR_FWD) + i, n, PAIR_BT[n], bool(inv), n)
     for inv in (0, 1) for i, n in enumerate(PAIR_SIZES)]
    + [Form("wave8_fwd", WAVE8_FWD, 512, 1, False, 512), Form("wave8_inv", WAVE8_INV, 512, 1, True, 512),
       Form("wave8_halfzero", WAVE8_HALFZERO, 512, 1, False, 256),
       Form("wave16_fwd", WAVE16_FWD, 1024, 1, False, 1024), Form("wave16_inv", WAVE16_INV, 1024, 1, True, 1024),
       Form("wave16_halfzero", WAVE16_HALFZERO, 1024, 1, False, 512)])
FORM_BY_NAME = {f.name: f for f in COMPLEX_FORMS}
# the full-input form a HALFZERO form must equal bit for bit on zero-padded data
HALFZERO_OF = {"wave8_halfzero": "wave8_fwd", "wave16_halfzero": "wave16_fwd"}


def unit_floats(form_id):
    """(floats of `in` per unit, floats of `out` per unit, floats in front of the units) of every form the probe knows."""
    for f in COMPLEX_FORMS:
        if f.id == form_id:
            return 2 * f.bt * f.n_in, 2 * f.bt * f.n, 0
    return {REAL2048_FWD: (2048, 2 * 1025, 0), REAL2048_INV: (2 * 1025, 2048, 0), TWIDDLES: (0, 2 * 64 * TWIDDLE_COUNT, 0),
            SCALE: (1, 2, 2), WAVEMAX: (64, 64, 0)}[form_id]


ALL_FORM_IDS = tuple(f.id for f in COMPLEX_FORMS) + (REAL2048_FWD, REAL2048_INV, TWIDDLES, SCALE, WAVEMAX)


# ---- the reference transforms ----------------------------------------------------------------------------------------------
def dft(x, inverse=False):
    """Unnormalised DFT along the last axis in complex128: sum_n x[n] W^(+-nk); the inverse is N * ifft."""
    x = np.asarray(x, dtype=np.complex128)
    return np.fft.ifft(x, axis=-1) * x.shape[-1] if inverse else np.fft.fft(x, axis=-1)


def dft_form(form, x):
    """Reference of a complex form on `x` [..., n_in]: HALFZERO zero-pads to n."""
    x = np.asarray(x, dtype=np.complex128)
    if form.n_in != form.n:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (form.n - form.n_in,), np.complex128)], axis=-1)
    return dft(x, form.inverse)


def rfft2048(x):
    return np.fft.rfft(np.asarray(x, dtype=np.float64), n=2048, axis=-1)


def irfft2048_unnormalised(X):
    """The header's contract for the real inverse: 2048 * irfft."""
    return 2048.0 * np.fft.irfft(np.asarray(X, dtype=np.complex128), n=2048, axis=-1)


def twiddle(j, n):
    """The forward twiddle W_n^j = exp(-2 pi i j / n), from the integer j mod n: exact 0 and +-1 at multiples of n / 4."""
    j = np.asarray(j, dtype=np.int64) % n
    c = np.cos(2.0 * np.pi * j / n)
    s = np.sin(2.0 * np.pi * j / n)
    q = (4 * j) % n == 0                                # a multiple of a quarter turn: no rounding residue of pi
    quarter = (4 * j) // n
    c = np.where(q, np.array([1.0, 0.0, -1.0, 0.0])[quarter % 4], c)
    s = np.where(q, np.array([0.0, 1.0, 0.0, -1.0])[quarter % 4], s)
    return c - 1j * s


def expected_twiddles():
    """[64 lanes, TWIDDLE_COUNT] complex128: what DDSP_WFFT_TWIDDLES dumps (order: include/ddsp_hip.h), and per column the
    bound kind: 's' a sincospif value, 'p' a twiddle2048 product."""
    lane = np.arange(64)[:, None]
    cols, kinds = [], []

    def add(block, kind="s"):
        cols.append(block)
        kinds.extend(kind * block.shape[1])

    for r1 in (8, 16):                                  # make_twiddles<R1>
        n = 64 * r1
        add(twiddle(lane * np.arange(r1)[None, :], n))
        for d in range(r1 // 8):
            n3 = lane // r1 + (64 // r1) * d
            add(twiddle(n3 * np.arange(8)[None, :], 64))
    add(twiddle(lane * np.arange(2)[None, :], 128))     # PairFft<128>::t1s
    add(twiddle(lane * np.arange(4)[None, :], 256))     # PairFft<256>::t1s
    for _ in range(3):                                  # PairFft<64, 128, 256>::tw.t2[0]
        add(twiddle((lane >> 3) * np.arange(8)[None, :], 64))
    add(twiddle(lane, 2048))                            # lane_w2048
    add(twiddle(lane + 64 * np.arange(9)[None, :], 2048), "p")      # twiddle2048(wbase, it)
    out = np.concatenate(cols, axis=1)
    assert out.shape == (64, TWIDDLE_COUNT)
    return out, "".join(kinds)


def ulp32(x):
    """Spacing of fp32 at |x| (x in float64; normal range)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def frame_scale_model(m, c_in, c_out):
    """ddsp_wfft::frame_scale_of in exact arithmetic, results rounded to fp32: e = the frexp exponent of a positive finite m
    (0 otherwise), clamped to +-100; in = c_in 2^-e; out = 0 for m == 0 (either sign), else c_out 2^e."""
    m = float(np.float32(m))
    e = 0
    if m > 0.0 and m < math.inf:
        e = math.frexp(m)[1]
    e = max(-100, min(100, e))
    s_in = np.float32(math.ldexp(float(np.float32(c_in)), -e))
    s_out = np.float32(0.0) if m == 0.0 else np.float32(math.ldexp(float(np.float32(c_out)), e))
    return s_in, s_out


# ---- the bounds -------------------------------------------------------------------------------------------------------------
def twiddle_component_ulps():
    """A sincospif component: SINCOSPI_ULP ulps of the true value (OCML's documented accuracy; the argument 2 j / N is exact in
    fp32 for a power-of-two N) plus the half ulp by which the fp64 reference value's own fp32 neighbourhood is resolved -- no
    more than 1e-7 of an ulp here, written as a relative slack of 2^-20."""
    return SINCOSPI_ULP * (1.0 + 2.0 ** -20)


def twiddle_error():
    """|w^ - w| of a sincospif twiddle.  Each component is below 1 in magnitude wherever it is inexact, so its ulp is at most U
    and its error at most SINCOSPI_ULP * U; two components: sqrt(2) * SINCOSPI_ULP * U = 2.83 U."""
    return math.sqrt(2.0) * SINCOSPI_ULP * U


def constant_error():
    """|w^ - w| of a literal constant (W8, W16, W32 tables): both components correctly rounded values below 1, half an ulp
    <= U / 2 each: U / sqrt(2) = 0.71 U."""
    return U / math.sqrt(2.0)


def fma_product_error():
    """|fl(a w) - a w| / (|a| |w|) of the header's complex product (one FMA and one product per component): 2 U (Jeannerod,
    Kornerup, Louvet, Muller 2017, the FMA form of the complex product).  mul_w8_1/3, (a.x +- a.y) * r, has one rounded addition
    and one rounded product per component: 2 U as well."""
    return 2.0 * U


def twiddle_product_bound():
    """One product with a sincospif twiddle: |a w^ (1 + d) - a w| <= (twiddle_error + fma_product_error) |a| to first order;
    the cross term is kept: (1 + t)(1 + p) - 1 = 4.83 U."""
    return (1.0 + twiddle_error()) * (1.0 + fma_product_error()) - 1.0


def constant_product_bound():
    """One product with a literal constant (the radix-8 and radix-16 butterflies' W8^j, W16^j): 2.71 U."""
    return (1.0 + constant_error()) * (1.0 + fma_product_error()) - 1.0


def impulse_factors(n):
    """(constant products, twiddle products) on the longest path of a unit impulse through the N-point transform.  An impulse
    meets no non-trivial addition (every butterfly adds zeros), only products:
      step 1, radix R1 = N / 64: R1 = 16: W16^j, then a W8 constant inside its radix-8 half (2); R1 = 8: one W8 constant;
              R1 <= 4: +-1, +-i only (0);  then t1 = W_N^(lane k1) for R1 > 1;
      step 2, radix 8: one W8 constant, then t2 = W_64^(n3 k2);  step 3, radix 8: one W8 constant."""
    r1 = n // 64
    return {1: 0, 2: 0, 4: 0, 8: 1, 16: 2}[r1] + 2, (1 if r1 > 1 else 0) + 1


def impulse_bound(n):
    """|X^_k - W_N^(+-n0 k)| for a unit impulse (1 or i) at n0: the product of the factors' (1 + bound), minus 1."""
    nc, nt = impulse_factors(n)
    return (1.0 + constant_product_bound()) ** nc * (1.0 + twiddle_product_bound()) ** nt - 1.0


def twiddle2048_bound():
    """|twiddle2048(wbase, it) - W_2048^k|, k = lane + 64 it: the base W_2048^lane (twiddle_error), half an ulp per component
    of the W_32^it table constant (constant_error), one FMA product (fma_product_error): 5.54 U.  The REAL2048 impulse at
    n0 = 1 reads exactly this number out (Fe = 0, Fo = 1: X_k = the twiddle, no further rounding), so this is its bound too; it
    lies below the 8 U of the running-product defect that the fuzz sweep once met."""
    return (1.0 + twiddle_error()) * (1.0 + constant_error()) * (1.0 + fma_product_error()) - 1.0


def real2048_impulse_bound():
    """|X^_k - W_2048^(n0 k)| of the real 2048-point form for a unit impulse at any n0.  Z_k and conj Z_(M-k) are two results of
    the 1024-point impulse path, each within b = impulse_bound(1024) of the same unit-modulus number (n0 even) or of opposite
    ones (n0 odd).  Halving is exact, so of Fe and Fo one is within b of that number and the other within b of zero; T = W^k Fo
    adds the twiddle2048 product ((1 + twiddle2048_bound)(1 + fma_product_error) - 1 on a modulus <= 1 + b); Fe + T is one
    rounded addition per component of a result of modulus <= 1 (2 U covers both):  2 b + (1 + b) (product) + 2 U = 50 U."""
    b = impulse_bound(1024)
    product = (1.0 + twiddle2048_bound()) * (1.0 + fma_product_error()) - 1.0
    return 2.0 * b + (1.0 + b) * product + 2.0 * U


def fft_ceiling(n):
    """||X^ - X||_2 / ||X||_2 of an fp32 Cooley-Tukey FFT of n = 2^t points: t eta / (1 - t eta), eta = mu + gamma_4 (sqrt(2) +
    mu), mu the twiddles' absolute error, gamma_4 = 4 U / (1 - 4 U) (Higham, Accuracy and Stability of Numerical Algorithms,
    2nd ed., Theorem 24.2).  The radix-8 and radix-16 butterflies are radix-2 stages whose twiddles are the literal constants
    (error below mu = twiddle_error()), and the header's FMA product is more accurate than the theorem's.  About 85 U at 1024:
    it only says "not broken"."""
    t = math.log2(n)
    mu = twiddle_error()
    g4 = 4.0 * U / (1.0 - 4.0 * U)
    eta = mu + g4 * (math.sqrt(2.0) + mu)
    return t * eta / (1.0 - t * eta)


def fft_ceiling_max(n):
    """max_k |X^_k - X_k| / ||x||_2 <= ||X^ - X||_2 / ||x||_2 = sqrt(n) ||X^ - X||_2 / ||X||_2 (Parseval)."""
    return math.sqrt(n) * fft_ceiling(n)


def real2048_ceiling():
    """The real form is a 1024-point complex transform and one more stage (split or pack) with the twiddle2048 product, whose
    error is below 2 twiddle_error(): bounded by a 2048-point transform with twiddles of that error, i.e. one more stage and mu
    doubled in Higham's eta."""
    mu = twiddle2048_bound()
    g4 = 4.0 * U / (1.0 - 4.0 * U)
    eta = mu + g4 * (math.sqrt(2.0) + mu)
    return 11.0 * eta / (1.0 - 11.0 * eta)


def round_trip_ceiling(n):
    """||inverse(forward(x)) / n - x||_2 / ||x||_2: two transforms, (1 + c)^2 - 1; the division by the power of two n is exact."""
    return (1.0 + fft_ceiling(n)) ** 2 - 1.0


# ---- error measures ---------------------------------------------------------------------------------------------------------
def e2(got, ref):
    """||got - ref||_2 / ||ref||_2 per transform (last axis)."""
    return np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def einf(got, ref, x):
    """max_k |got_k - ref_k| / ||x||_2 per transform, x the transform's input."""
    return np.max(np.abs(got - ref), axis=-1) / np.linalg.norm(x, axis=-1)
