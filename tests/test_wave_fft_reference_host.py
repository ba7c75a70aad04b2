"""The fp64 reference and the bounds of tests/wave_fft_reference.py checked on their own, and the argument validation of the
test hook ddsp_wfft_probe -- all without a device (nothing here launches a kernel)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ddsp_pytorch_amd as ddsp

import wave_fft_reference as R

U = R.U


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("inverse", [False, True])
def test_reference_dft_against_a_longdouble_matrix_product(n, inverse):
    """numpy.fft in complex128 against the definition, sum_n x[n] exp(-+2 pi i n k / N), as an O(N^2) product in longdouble.
    The twiddles' angles are reduced in integers (n k mod N) so that the matrix itself is good to longdouble's epsilon."""
    rng = np.random.default_rng(n + inverse)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    nk = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    ang = 2 * np.pi * nk.astype(np.longdouble) / np.longdouble(n)     # (pi itself only to double: 1e-16 relative, below the check)
    sign = 1 if inverse else -1
    wr, wi = np.cos(ang), sign * np.sin(ang)
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    Xr, Xi = wr @ xr - wi @ xi, wr @ xi + wi @ xr
    got = R.dft(x, inverse)
    err = np.sqrt(((got.real - Xr) ** 2 + (got.imag - Xi) ** 2).astype(np.float64))
    # fp64 FFT: log2(N) stages of about one double epsilon each; 2^-53 * 8 * log2 N relative to ||x||_2 is generous for it and
    # still nine decimal digits below fp32's U
    assert err.max() <= 8 * math.log2(n) * 2.0 ** -53 * np.linalg.norm(x)


def test_reference_rfft_of_impulses_in_closed_form():
    k = np.arange(1025)
    for n0 in (0, 1, 2, 3, 511, 1024, 1025, 2047):
        x = np.zeros(2048)
        x[n0] = 1.0
        want = R.twiddle(n0 * k, 2048)
        # both sides are unit-modulus numbers good to a few double epsilons; 16 of them is still 2^-25 of fp32's U
        assert np.abs(R.rfft2048(x) - want).max() <= 16 * 2.0 ** -53, n0
    # and back: the real inverse's contract is 2048 * irfft
    x = np.random.default_rng(0).standard_normal(2048)
    assert np.abs(R.irfft2048_unnormalised(R.rfft2048(x)) - 2048.0 * x).max() <= 2048 * 64 * 2.0 ** -53


def test_reference_twiddles_are_exact_at_quarter_turns_and_unit_modulus():
    for n in (64, 128, 256, 512, 1024, 2048):
        j = np.arange(-n, 2 * n)
        w = R.twiddle(j, n)
        assert np.abs(np.abs(w) - 1.0).max() <= 2.0 ** -52
        assert np.array_equal(w[j % (n // 4) == 0], np.array([1, -1j, -1, 1j])[(j[j % (n // 4) == 0] // (n // 4)) % 4])
    tw, kinds = R.expected_twiddles()
    assert tw.shape == (64, R.TWIDDLE_COUNT) and len(kinds) == R.TWIDDLE_COUNT and kinds.count("p") == 9
    lane0 = np.ones(79, dtype=np.complex128)                               # lane 0: every sincospif twiddle is W^0 ...
    lane0[40:48] = R.twiddle(4 * np.arange(8), 64)                         # ... but Twiddles<16>::t2[1], whose n3 is 4
    assert np.array_equal(tw[0, :79], lane0)
    assert tw[1, 1] == R.twiddle(1, 512) and tw[63, 16 + 15] == R.twiddle(63 * 15, 1024) and tw[5, 78] == R.twiddle(5, 2048)
    assert tw[63, 87] == R.twiddle(63 + 512, 2048)


def test_frame_scale_model_over_all_fp32_exponents():
    for c_in, c_out in ((1.0, 0.5), (0.75, 1.5)):
        for e in range(-149, 128):
            for mant in (1.0, 1.5, 2.0 - 2.0 ** -23):
                m = np.float32(math.ldexp(mant, e))
                if not (m > 0 and np.isfinite(m)):
                    continue
                s_in, s_out = R.frame_scale_model(m, c_in, c_out)
                ee = max(-100, min(100, math.frexp(float(m))[1]))
                assert float(s_in) == c_in * 2.0 ** -ee and float(s_out) == c_out * 2.0 ** ee     # exact powers of two times c
                assert float(s_in) * float(s_out) == c_in * c_out
                if abs(math.frexp(float(m))[1]) <= 100:
                    assert 0.5 <= float(m) * float(s_in) / c_in < 1.0
        for m in (0.0, -0.0):
            assert R.frame_scale_model(m, c_in, c_out) == (np.float32(c_in), np.float32(0.0))
        for m in (math.inf, math.nan, -1.0, -math.inf):                    # e = 0; only m == 0 zeroes `out`
            assert R.frame_scale_model(m, c_in, c_out) == (np.float32(c_in), np.float32(c_out))


def test_bounds_lie_below_the_sensitivities_they_are_meant_to_keep():
    """Every bound at every size, in units of U, against what the device tests must be able to tell apart."""
    assert U == 2.0 ** -24 and R.CPU_FACTOR == 3.0
    # a twiddle moved by 4 ulp must leave the read-out's tolerance whatever its own (<= 2 ulp) error was
    assert R.twiddle_component_ulps() <= 2.0 + 1e-5 and 4.0 - R.SINCOSPI_ULP >= R.twiddle_component_ulps() - 1e-5
    assert R.constant_error() < R.twiddle_error() < R.twiddle_product_bound() < 5.0 * U
    assert 2.7 * U < R.constant_product_bound() < 2.72 * U
    # the running-product twiddle of the 2048-point path was wrong by 8 U
    assert 5.5 * U < R.twiddle2048_bound() < 8.0 * U
    for n in R.PAIR_SIZES:
        nc, nt = R.impulse_factors(n)
        assert nc + nt <= 6 and nt <= 2
        b = R.impulse_bound(n)
        assert (nc * 2.7 + nt * 4.8) * U < b < 21.0 * U
        # exchanged elements: two different bins of an impulse's spectrum differ by at least |1 - W_N| = 2 sin(pi / N)
        assert b < 0.01 * 2.0 * math.sin(math.pi / n)
        # the ceiling: about 10 U per radix-2 stage ("about 100 U at 1024"), and never below the impulse's own bound / sqrt(N)
        t = math.log2(n)
        assert 8.0 * t * U < R.fft_ceiling(n) < 10.0 * t * U
        assert R.fft_ceiling_max(n) == math.sqrt(n) * R.fft_ceiling(n)
        assert R.fft_ceiling(n) < R.round_trip_ceiling(n) < 2.001 * R.fft_ceiling(n)
    assert R.fft_ceiling(1024) < 100.0 * U
    assert R.real2048_impulse_bound() < 52.0 * U and R.real2048_impulse_bound() < 0.01 * 2.0 * math.sin(math.pi / 2048)
    assert R.fft_ceiling(2048) < R.real2048_ceiling() < 160.0 * U


def test_form_table_matches_the_probe_sizes():
    L = ddsp._lib.lib()
    a, b = ctypes.c_long(-1), ctypes.c_long(-1)
    for form in R.ALL_FORM_IDS:
        iu, ou, head = R.unit_floats(form)
        for units in (0, 1, 7):
            assert L.ddsp_wfft_probe_sizes(form, units, ctypes.byref(a), ctypes.byref(b)) == 0
            assert (a.value, b.value) == (head + iu * units, ou * units), (form, units)
    assert sorted(R.ALL_FORM_IDS) == list(range(21))
    for f in R.COMPLEX_FORMS:
        assert f.bt * f.n in (512, 1024) and f.n_in in (f.n, f.n // 2)
    for bad in (-1, 21, 1000):
        assert L.ddsp_wfft_probe_sizes(bad, 1, ctypes.byref(a), ctypes.byref(b)) == R.EINVAL
    assert L.ddsp_wfft_probe_sizes(0, -1, ctypes.byref(a), ctypes.byref(b)) == R.EINVAL
    assert L.ddsp_wfft_probe_sizes(0, 1, None, ctypes.byref(b)) == R.EINVAL


def test_probe_validates_before_it_launches():
    """Unknown form, null pointer, negative units: DDSP_EINVAL; no units: 0.  None of these reaches a launch (there is no device
    here to launch on)."""
    L = ddsp._lib.lib()
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    for form in R.ALL_FORM_IDS:
        assert L.ddsp_wfft_probe(form, p, p, 0, None) == 0
        assert L.ddsp_wfft_probe(form, None, p, 1, None) == R.EINVAL and L.ddsp_wfft_probe(form, p, None, 1, None) == R.EINVAL
        assert L.ddsp_wfft_probe(form, None, None, 0, None) == R.EINVAL
        assert L.ddsp_wfft_probe(form, p, p, -1, None) == R.EINVAL
        assert L.ddsp_wfft_probe(form, p, p, (1 << 20) + 1, None) == R.EINVAL
    for bad in (-1, 21, 1 << 30):
        assert L.ddsp_wfft_probe(bad, p, p, 0, None) == R.EINVAL and L.ddsp_wfft_probe(bad, p, p, 1, None) == R.EINVAL


def test_probe_is_refused_without_opt_in():
    """A test hook: DDSP_EPERM in a process that did not set DDSP_TEST_HOOKS=1 before the library was loaded, whatever the
    arguments (here: valid ones that would otherwise return 0 without a launch)."""
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); w = ctypes.c_uint64(0); p = ctypes.c_void_p(ctypes.addressof(w)); "
            "L.ddsp_wfft_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]; "
            "print(L.ddsp_test_hooks_enabled(), *[L.ddsp_wfft_probe(f, p, p, 0, None) for f in (0, 9, 12, 17, 18, 19, 20, 99)])")
    env = {k: v for k, v in os.environ.items() if k != "DDSP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0"] + ["-3"] * 8, out
    env["DDSP_TEST_HOOKS"] = "1"
    out = subprocess.run([sys.executable, "-c", code, ddsp._lib.SO_PATH], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1"] + ["0"] * 7 + ["-1"], out
