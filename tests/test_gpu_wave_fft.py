"""The shared one-wavefront FFT (csrc/ddsp_wave_fft.h) on its own, through the test hook ddsp_wfft_probe, against the fp64
reference and the derived bounds of tests/wave_fft_reference.py: exact checks (no tolerance), read-outs that single out one
twiddle or one exchange address each, and accuracy against the fp64 DFT -- at every size, direction and form the library
instantiates.  Every test prints the figures it asserts on (`pytest -s`), in units of U = 2^-24."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp

import wave_fft_reference as R

pytestmark = pytest.mark.gpu

U = R.U
GUARD = 256                                                  # floats behind `out` that no kernel may touch
FORMS = R.COMPLEX_FORMS
FORM_IDS = [f.name for f in FORMS]
PAIRS_WITH_NEIGHBOURS = [f for f in FORMS if f.bt > 1]
ROUND_TRIPS = [(f"pair{n}_fwd", f"pair{n}_inv") for n in R.PAIR_SIZES] + [("wave8_fwd", "wave8_inv"), ("wave16_fwd", "wave16_inv")]


# ---- running the probe ------------------------------------------------------------------------------------------------------
def probe(form_id, x, units):
    """`x`: float32 array of the form's input floats -> float32 array of its output floats."""
    L = ddsp._lib.lib()
    a, b = ctypes.c_long(), ctypes.c_long()
    assert L.ddsp_wfft_probe_sizes(form_id, units, ctypes.byref(a), ctypes.byref(b)) == 0
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    assert x.size == a.value, (form_id, x.size, a.value)
    xin = torch.from_numpy(x if x.size else np.zeros(2, np.float32)).cuda()
    out = torch.full((b.value + GUARD,), float("nan"), device="cuda")
    out[b.value:] = 12345.0
    rc = L.ddsp_wfft_probe(form_id, xin.data_ptr(), out.data_ptr(), units, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.all(res[b.value:] == 12345.0), "the probe wrote behind its output"
    return res[:b.value]


def to_floats(z):
    z = np.asarray(z, dtype=np.complex128)
    return np.stack([z.real, z.imag], axis=-1).astype(np.float32)


def to_complex(f):
    f = np.asarray(f, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    return f[:, 0] + 1j * f[:, 1]


def as_fp32_complex(z):
    """z rounded to what the device is given."""
    f = to_floats(z).astype(np.float64)
    return f[..., 0] + 1j * f[..., 1]


def run_bits(form, z):
    """`z` [T, n_in] complex, T a multiple of the form's transforms per unit -> float32 [T, n, 2]."""
    z = np.asarray(z)
    T = z.shape[0]
    assert z.shape == (T, form.n_in) and T % form.bt == 0
    return probe(form.id, to_floats(z), T // form.bt).reshape(T, form.n, 2)


def run(form, z):
    b = run_bits(form, z).astype(np.float64)
    return b[..., 0] + 1j * b[..., 1]


def run_real_fwd(x):
    x = np.asarray(x)
    return to_complex(probe(R.REAL2048_FWD, x, x.shape[0])).reshape(x.shape[0], 1025)


def run_real_inv(X):
    X = np.asarray(X)
    return probe(R.REAL2048_INV, to_floats(X), X.shape[0]).reshape(X.shape[0], 2048).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def normal(seed, *shape):
    rng = np.random.default_rng(seed)
    return as_fp32_complex(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def cpu_fft(form, z):
    """The fp32 library transform on the CPU, on the same (fp32) inputs."""
    t = torch.from_numpy(np.asarray(z)).to(torch.complex64)
    if form.n_in != form.n:
        t = torch.cat([t, torch.zeros(t.shape[0], form.n - form.n_in, dtype=torch.complex64)], dim=-1)
    y = torch.fft.ifft(t, dim=-1, norm="forward") if form.inverse else torch.fft.fft(t, dim=-1)
    return y.numpy().astype(np.complex128)


def report(name, **figs):
    print("WFFT " + name + " " + " ".join(f"{k}={v / U:.2f}U" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def within_cpu_and_ceiling(name, gpu, cpu, ceiling):
    """The two criteria on one figure: at most CPU_FACTOR times the CPU fp32 transform's, and under the derived ceiling."""
    report(name, gpu=float(gpu), cpu=float(cpu), ratio=f"{gpu / cpu if cpu else (0.0 if not gpu else float('inf')):.2f}", ceiling=float(ceiling))
    assert gpu <= R.CPU_FACTOR * cpu, (name, gpu / U, cpu / U)
    assert gpu <= ceiling, (name, gpu / U, ceiling / U)


# ---- exact checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.HALFZERO_OF))
def test_halfzero_is_the_full_transform_of_zero_padded_data_bit_for_bit(name):
    """HALFZERO only skips additions of exact zeros."""
    half, full = R.FORM_BY_NAME[name], R.FORM_BY_NAME[R.HALFZERO_OF[name]]
    z = normal(1, 64, half.n_in)
    padded = np.concatenate([z, np.zeros_like(z)], axis=-1)
    assert np.array_equal(bits(run_bits(half, z)), bits(run_bits(full, padded)))


@pytest.mark.parametrize("name", FORM_IDS)
def test_zero_transforms_give_exact_zeros_also_beside_loud_neighbours(name):
    form = R.FORM_BY_NAME[name]
    assert np.all(run_bits(form, np.zeros((2 * form.bt, form.n_in))) == 0.0)
    if form.bt > 1:                                          # transforms of one unit share lanes, not values
        z = normal(2, 2 * form.bt, form.n_in) * 2.0 ** 20
        quiet = [1, form.bt + form.bt // 2]
        z[quiet] = 0.0
        got = run_bits(form, z)
        assert np.all(got[quiet] == 0.0)
        assert np.all(np.abs(got[[0, form.bt]]).max(axis=(1, 2)) > 2.0 ** 20)


def test_zero_real_frames_give_exact_zeros():
    assert np.all(run_real_fwd(np.zeros((2, 2048))) == 0.0) and np.all(run_real_inv(np.zeros((2, 1025))) == 0.0)


@pytest.mark.parametrize("name", [f.name for f in PAIRS_WITH_NEIGHBOURS])
def test_a_transform_does_not_see_its_neighbours_in_the_unit(name):
    form = R.FORM_BY_NAME[name]
    z = normal(3, form.bt, form.n_in)
    base = bits(run_bits(form, z))
    for b in range(form.bt):
        other = normal(4 + b, form.bt, form.n_in) * 2.0 ** 6
        other[b] = z[b]
        assert np.array_equal(bits(run_bits(form, other))[b], base[b]), b


@pytest.mark.parametrize("name", FORM_IDS + ["real2048_fwd", "real2048_inv"])
def test_runs_repeat_and_units_do_not_depend_on_the_grid(name):
    if name.startswith("real2048"):
        fwd = name.endswith("fwd")
        x = normal(5, 7, 2048).real if fwd else hermitian_spectra(5, 7)
        one = (lambda v: bits(probe(R.REAL2048_FWD if fwd else R.REAL2048_INV, v if fwd else to_floats(v), v.shape[0])).reshape(v.shape[0], -1))
        a, b, c = one(x), one(x), one(x[6:7])
    else:
        form = R.FORM_BY_NAME[name]
        z = normal(5, 7 * form.bt, form.n_in)
        a, b, c = bits(run_bits(form, z)), bits(run_bits(form, z)), bits(run_bits(form, z[6 * form.bt:]))
    assert np.array_equal(a, b)
    assert np.array_equal(a[-c.shape[0]:], c)                # unit 6 of 7 == the same data as unit 0 of 1


@pytest.mark.parametrize("k", [-20, 20])
@pytest.mark.parametrize("name", FORM_IDS + ["real2048_fwd", "real2048_inv"])
def test_a_power_of_two_scales_every_output_exactly(name, k):
    """No hidden absolute constant anywhere between the load and the store."""
    if name == "real2048_fwd":
        x = normal(6, 4, 2048).real
        a, b = run_real_fwd(x), run_real_fwd(x * 2.0 ** k)
    elif name == "real2048_inv":
        X = hermitian_spectra(6, 4)
        a, b = run_real_inv(X), run_real_inv(X * 2.0 ** k)
    else:
        form = R.FORM_BY_NAME[name]
        z = normal(6, 4 * form.bt, form.n_in)
        a, b = run(form, z), run(form, z * 2.0 ** k)
    assert np.array_equal(a * 2.0 ** k, b)


def scale_grid():
    ms = [np.float32(np.ldexp(mant, e)) for e in range(-149, 128) for mant in (1.0, 1.5, 2.0 - 2.0 ** -23)]
    ms = [m for m in ms if m > 0 and np.isfinite(m)]
    ms += [np.float32(v) for v in (0.0, -0.0, np.inf, np.nan, -1.0, -np.inf, 2.0 ** 101, 2.0 ** -101, 2.0 ** 100, 2.0 ** -100,
                                   1.99 * 2.0 ** 99, 2.0 ** 127, 2.0 ** -149, 2.0 ** -126)]
    return np.array(ms, dtype=np.float32)


@pytest.mark.parametrize("c_in,c_out", [(1.0, 0.5), (0.75, 1.5), (1.0, 1.0 / 4096.0)])
def test_frame_scale_equals_the_exact_model_bitwise(c_in, c_out):
    m = scale_grid()
    got = probe(R.SCALE, np.concatenate([np.array([c_in, c_out], np.float32), m]), m.size).reshape(-1, 2)
    want = np.array([R.frame_scale_model(v, c_in, c_out) for v in m], dtype=np.float32)
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, [(float(m[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]
    g = got.astype(np.float64)
    assert np.all(np.isfinite(g)) and np.all(np.abs(g[:, 0]) >= 2.0 ** -126)                 # never denormal, inf or NaN ...
    assert np.all((np.abs(g[:, 1]) >= 2.0 ** -126) | ((g[:, 1] == 0.0) & (m == 0.0)))          # ... `out` zero for m == 0 only
    e = np.array([np.frexp(float(v))[1] if (v > 0 and np.isfinite(v)) else 0 for v in m])
    inside = (m > 0) & np.isfinite(m) & (np.abs(e) <= 100)
    scaled = m[inside].astype(np.float64) * g[inside, 0] / c_in
    assert np.all((scaled >= 0.5) & (scaled < 1.0))
    assert np.all(g[inside, 0] * g[inside, 1] == np.float64(np.float32(c_in)) * np.float64(np.float32(c_out)))
    assert np.all(g[m == 0.0, 1] == 0.0)


def test_wave_max_finds_any_lane_drops_nan_and_keeps_infinity():
    rng = np.random.default_rng(7)
    rows = rng.random((64 + 5, 64)).astype(np.float32)
    for r in range(64):
        rows[r, r] = 3.0 + r                                 # the maximum in each single lane once
    rows[64, 5] = np.nan                                     # a NaN lane is dropped
    rows[65, 9] = np.nan
    rows[65, 40] = np.inf                                    # an infinite lane wins, also beside a NaN
    rows[66, :] = -rng.random(64).astype(np.float32) - 1.0   # all negative
    rows[66, 63] = -np.inf
    rows[67, :] = np.nan                                     # every lane NaN: fmaxf has nothing else to return -- NaN
    rows[68, :] = np.nan
    rows[68, 17] = -2.5                                      # one number among NaNs
    got = probe(R.WAVEMAX, rows, rows.shape[0]).reshape(-1, 64)
    assert np.all(bits(got) == bits(got)[:, :1])             # all 64 lanes report the same bits
    want = np.array([3.0 + r for r in range(64)] + [np.nanmax(rows[64]), np.inf, np.max(rows[66]), np.nan, -2.5], dtype=np.float32)
    assert np.array_equal(got[:, 0], want, equal_nan=True)
    assert np.isnan(got[67]).all()


# ---- read-outs --------------------------------------------------------------------------------------------------------------
def test_every_twiddle_of_every_lane():
    got = to_complex(probe(R.TWIDDLES, np.zeros(0, np.float32), 2)).reshape(2, 64, R.TWIDDLE_COUNT)
    assert np.array_equal(got[0], got[1])
    got = got[0]
    want, kinds = R.expected_twiddles()
    s = np.array([k == "s" for k in kinds])
    # sincospif values: each component within the library's accuracy of the true value; exact 0 and +-1 at exact arguments
    worst = 0.0
    for part in (np.real, np.imag):
        g, w = part(got[:, s]), part(want[:, s])
        exact = (w == 0.0) | (np.abs(w) == 1.0)
        assert np.array_equal(g[exact], w[exact])
        ulps = np.abs(g - w)[~exact] / R.ulp32(w[~exact])
        worst = max(worst, float(ulps.max()))
        assert ulps.max() <= R.twiddle_component_ulps(), ulps.max()
    # twiddle2048: one product of the base with a table constant
    err = np.abs(got[:, ~s] - want[:, ~s])
    report("twiddles", sincospi_ulp=f"{worst:.3f}", twiddle2048=float(err.max()), twiddle2048_bound=R.twiddle2048_bound())
    assert err.max() <= R.twiddle2048_bound()
    assert np.array_equal(got[:, ~s][:, 0], got[:, s][:, -1])                       # it = 0: W_32^0 = 1 leaves the base as it is


@functools.lru_cache(maxsize=None)
def impulse_reference(n):
    k = np.arange(n)
    return R.twiddle((k[:, None] * k[None, :]) % n, n)       # [n0, k] = W_n^(n0 k)


@pytest.mark.parametrize("name", FORM_IDS)
def test_impulses_read_out_every_twiddle_path_and_every_exchange_address(name):
    """1 and i at every input position, one per transform.  An impulse meets products only: bin k is W_N^(+-n0 k) within the
    bound of the factors on its path -- and an exchanged pair of elements anywhere (natural(), store_natural, addr1, addr2) is
    an error of order 1.

    Where every sincospif twiddle on the path is W^0 = 1, the result is a power of W8 made by mul_w8_1 / mul_w8_3 alone,
    (1 + 0) * r and nothing else: each component is exactly 0, +-1 or +-fl32(1 / sqrt 2), the correctly rounded constant.
    R1 >= 8: the impulses at N/8 and 3N/8 (lane 0, n1 = R1/8, 3 R1/8: step 1 makes W8^k1, t1 = W^0, and steps 2, 3 copy), every
    bin.  R1 < 8: the impulses at 8 and 24 (n2 = 1, 3; n3 = 0: t2 = W^0), the bins k = 0 mod R1 (k1 = 0: no t1)."""
    form = R.FORM_BY_NAME[name]
    eye = np.eye(form.n_in)
    one, im = run(form, eye + 0j), run(form, 1j * eye)
    w = impulse_reference(form.n)[:form.n_in]
    w = np.conj(w) if form.inverse else w
    err = max(np.abs(one - w).max(), np.abs(im - 1j * w).max())
    report(f"impulse {name}", err=float(err), bound=R.impulse_bound(form.n))
    assert err <= R.impulse_bound(form.n)

    r1 = form.n // 64
    positions, ks = ((form.n // 8, 3 * form.n // 8), np.arange(form.n)) if r1 >= 8 else ((8, 24), np.arange(0, form.n, r1))
    for n0 in positions:
        w8 = w[n0, ks]
        assert set(np.round(np.abs(np.concatenate([w8.real, w8.imag])), 6)) == {0.0, 0.707107, 1.0}
        for got, want in ((one[n0, ks], w8), (im[n0, ks], 1j * w8)):
            assert np.array_equal(got.real, want.real.astype(np.float32).astype(np.float64)), (n0, "the W8 constant is not fl32(1/sqrt 2)")
            assert np.array_equal(got.imag, want.imag.astype(np.float32).astype(np.float64)), (n0, "the W8 constant is not fl32(1/sqrt 2)")


def test_real2048_impulses_and_the_lone_twiddle2048_at_position_one():
    """(The inverse real form has no impulse read-out: one spectral line of a Hermitian spectrum is a cosine, whose samples
    are sums of two products, not a product alone; its accuracy and round-trip checks are further down.)"""
    k = np.arange(1025)
    n0 = np.arange(2048)
    got = run_real_fwd(np.eye(2048))
    want = R.twiddle((n0[:, None] * k[None, :]) % 2048, 2048)
    err = np.abs(got - want).max(axis=1)
    report("impulse real2048_fwd", err=float(err.max()), bound=R.real2048_impulse_bound(), at_one=float(err[1]), bound_at_one=R.twiddle2048_bound())
    assert err.max() <= R.real2048_impulse_bound()
    # n0 = 1: z = i delta, Z = i in every bin without a rounding, Fe = 0, Fo = 1: X_k is twiddle2048 itself
    assert err[1] <= R.twiddle2048_bound()
    assert R.twiddle2048_bound() < 8.0 * U


def exponentials(form):
    r1 = form.n // 64
    n = form.n
    k0s = sorted({k % n for k in (0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1, 64, r1, 8 * r1)})
    while len(k0s) % form.bt:
        k0s.append(k0s[-1])
    sign = -1 if form.inverse else 1                         # forward of W^(-k0 n), inverse of W^(+k0 n): N delta(k - k0)
    x = np.stack([np.conj(R.twiddle(sign * k0 * np.arange(n), n)) for k0 in k0s])
    return k0s, as_fp32_complex(x)[:, :form.n_in]


@pytest.mark.parametrize("name", FORM_IDS)
def test_single_exponentials_land_in_their_bin_and_leak_no_more_than_the_criterion(name):
    form = R.FORM_BY_NAME[name]
    k0s, x = exponentials(form)
    got, ref, cpu = run(form, x), R.dft_form(form, x), cpu_fft(form, x)
    if form.n_in == form.n:
        assert np.array_equal(np.argmax(np.abs(got), axis=1), k0s)
    within_cpu_and_ceiling(f"tones {name} e2", R.e2(got, ref).max(), R.e2(cpu, ref).max(), R.fft_ceiling(form.n))
    within_cpu_and_ceiling(f"tones {name} einf", R.einf(got, ref, x).max(), R.einf(cpu, ref, x).max(), R.fft_ceiling_max(form.n))


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
def lopsided(seed, shape, k):
    rng = np.random.default_rng(seed)
    return as_fp32_complex(rng.standard_normal(shape) + 1j * rng.standard_normal(shape) * 2.0 ** k)


def hermitian_spectra(seed, count):
    """rfft of real normal frames, rounded to fp32, bins 0 and 1024 real: what a c2r transform is given."""
    X = as_fp32_complex(R.rfft2048(np.random.default_rng(seed).standard_normal((count, 2048))))
    X[:, 0] = X[:, 0].real
    X[:, 1024] = X[:, 1024].real
    return X


@pytest.mark.parametrize("name", FORM_IDS)
def test_random_transforms_against_fp64_and_the_cpu_fp32_transform(name):
    form = R.FORM_BY_NAME[name]
    z = normal(8, 64, form.n_in)
    got, ref, cpu = run(form, z), R.dft_form(form, z), cpu_fft(form, z)
    within_cpu_and_ceiling(f"normal {name} e2", R.e2(got, ref).max(), R.e2(cpu, ref).max(), R.fft_ceiling(form.n))
    within_cpu_and_ceiling(f"normal {name} einf", R.einf(got, ref, z).max(), R.einf(cpu, ref, z).max(), R.fft_ceiling_max(form.n))


def split_halves(Z):
    """(A, B) of Z = FFT(a + i b): the two real signals' spectra."""
    Zr = np.conj(np.roll(Z[:, ::-1], 1, axis=1))             # conj Z[(N - k) mod N]
    return (Z + Zr) / 2, (Z - Zr) / 2j


@pytest.mark.parametrize("k", [-12, 12])
@pytest.mark.parametrize("name", FORM_IDS)
def test_lopsided_pairs_and_what_the_packing_leaks_into_the_quiet_half(name, k):
    form = R.FORM_BY_NAME[name]
    z = lopsided(9, (64, form.n_in), k)
    got, ref, cpu = run(form, z), R.dft_form(form, z), cpu_fft(form, z)
    tag = f"lopsided{k:+d} {name}"
    within_cpu_and_ceiling(f"{tag} e2", R.e2(got, ref).max(), R.e2(cpu, ref).max(), R.fft_ceiling(form.n))
    within_cpu_and_ceiling(f"{tag} einf", R.einf(got, ref, z).max(), R.einf(cpu, ref, z).max(), R.fft_ceiling_max(form.n))
    if not form.inverse:
        # the quiet half's spectrum error against the LOUD half's size; ||dB|| <= ||dZ|| <= ceiling ||Z||
        quiet, loud = (1, 0) if k < 0 else (0, 1)
        halves = [split_halves(v) for v in (got, cpu, ref)]
        size = np.linalg.norm(halves[2][loud], axis=1)
        leak = [np.linalg.norm(h[quiet] - halves[2][quiet], axis=1) / size for h in halves[:2]]
        ceiling = R.fft_ceiling(form.n) * float((np.linalg.norm(ref, axis=1) / size).max())
        within_cpu_and_ceiling(f"{tag} leak", leak[0].max(), leak[1].max(), ceiling)


@pytest.mark.parametrize("fwd,inv", ROUND_TRIPS)
def test_round_trip(fwd, inv):
    f, i = R.FORM_BY_NAME[fwd], R.FORM_BY_NAME[inv]
    z = normal(10, 64, f.n)
    back = run(i, as_fp32_complex(run(f, z))) / f.n
    t = torch.from_numpy(z).to(torch.complex64)
    cpu = torch.fft.ifft(torch.fft.fft(t, dim=-1), dim=-1).numpy().astype(np.complex128)
    within_cpu_and_ceiling(f"roundtrip {fwd} e2", R.e2(back, z).max(), R.e2(cpu, z).max(), R.round_trip_ceiling(f.n))
    within_cpu_and_ceiling(f"roundtrip {fwd} einf", (np.abs(back - z).max(axis=1) / np.linalg.norm(z, axis=1)).max(),
                           (np.abs(cpu - z).max(axis=1) / np.linalg.norm(z, axis=1)).max(), R.round_trip_ceiling(f.n))


def test_real2048_against_fp64_and_the_cpu_fp32_transform():
    x = normal(11, 64, 2048).real
    tones = np.stack([np.cos(2 * np.pi * k0 * np.arange(2048) / 2048) for k0 in (0, 1, 511, 512, 513, 1023, 1024, 64, 16, 128)])
    tones = tones.astype(np.float32).astype(np.float64)
    for tag, v in (("normal", x), ("tones", tones)):
        got, ref = run_real_fwd(v), R.rfft2048(v)
        cpu = torch.fft.rfft(torch.from_numpy(v).float(), dim=-1).numpy().astype(np.complex128)
        within_cpu_and_ceiling(f"{tag} real2048_fwd e2", R.e2(got, ref).max(), R.e2(cpu, ref).max(), R.real2048_ceiling())
        within_cpu_and_ceiling(f"{tag} real2048_fwd einf", R.einf(got, ref, v).max(), R.einf(cpu, ref, v).max(),
                               np.sqrt(2048.0) * R.real2048_ceiling())
    X = hermitian_spectra(12, 64)
    got, ref = run_real_inv(X), R.irfft2048_unnormalised(X)
    cpu = torch.fft.irfft(torch.from_numpy(X).to(torch.complex64), n=2048, dim=-1, norm="forward").numpy().astype(np.float64)
    within_cpu_and_ceiling("normal real2048_inv e2", R.e2(got, ref).max(), R.e2(cpu, ref).max(), R.real2048_ceiling())
    # e_inf is taken against the one-sided spectrum given; the two-sided one of Parseval's identity is at most sqrt(2) larger
    within_cpu_and_ceiling("normal real2048_inv einf", R.einf(got, ref, X).max(), R.einf(cpu, ref, X).max(),
                           np.sqrt(2.0 * 2048.0) * R.real2048_ceiling())
    # round trip
    back = run_real_inv(as_fp32_complex(run_real_fwd(x))) / 2048.0
    t = torch.from_numpy(x).float()
    cpub = torch.fft.irfft(torch.fft.rfft(t, dim=-1), n=2048, dim=-1).numpy().astype(np.float64)
    ceiling = (1.0 + R.real2048_ceiling()) ** 2 - 1.0
    within_cpu_and_ceiling("roundtrip real2048 e2", R.e2(back, x).max(), R.e2(cpub, x).max(), ceiling)
    within_cpu_and_ceiling("roundtrip real2048 einf", (np.abs(back - x).max(axis=1) / np.linalg.norm(x, axis=1)).max(),
                           (np.abs(cpub - x).max(axis=1) / np.linalg.norm(x, axis=1)).max(), ceiling)
