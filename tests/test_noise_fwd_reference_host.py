"""The fp64 reference of the filtered noise's forward (tests/noise_fwd_reference.py) on the host: against the C oracle, against the
reference's own torch output (tests/golden/g8_noise_*.npz), the properties of its yardsticks, and the derivation of the device
tolerances TOL_SAMPLE and TOL_FRAME from the two fp32 evaluations of the same definition.  Every test prints its figures before it
asserts (pytest -s)."""
import functools
import glob
import math
import os

import numpy as np
import pytest

import noise_fwd_reference as R
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (B, T, hop, F): crop (S > hop), pad, S = hop, F = 2, F = 3, an odd hop, hop 1
ORACLE_SHAPES = [(2, 5, 7, 33), (1, 4, 12, 65), (2, 3, 64, 129),          # crop
                 (2, 4, 100, 33), (1, 3, 512, 195), (1, 5, 160, 65),      # pad
                 (2, 5, 128, 65), (1, 2, 512, 257),                       # S = hop
                 (2, 6, 16, 2), (1, 6, 8, 3), (1, 3, 512, 3),             # F = 2, F = 3
                 (1, 3, 441, 129), (3, 4, 3, 5),                          # odd hops
                 (2, 9, 1, 9), (1, 7, 1, 2)]                              # hop 1


@functools.lru_cache(maxsize=None)
def case(shape, seed=0):
    """(H, u, y, Y) of a shape: the device tests' inputs (levels over seven decades, one zero frame), read-only."""
    B, T, hop, F = shape
    H, u = R.gpu_H(B, T, F, 100 + seed), R.gpu_uniform(B, T, hop, 200 + seed)
    y, Y = R.noise_fwd_fp64(H, hop, uniform=u)
    for a in (H, u, y, Y):
        a.setflags(write=False)
    return H, u, y, Y


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_reference_is_the_oracle_to_its_output_rounding(shape):
    """The oracle sums in double and returns fp32: per sample |oracle - y| <= 2^-24 |y| + 1e-12 Yframe."""
    B, T, hop, F = shape
    H, u, y, Y = case(shape)
    got = oracle.noise_forward(H, u, hop).reshape(B, T, hop).astype(np.float64)
    Yf, _ = R.frame_figures(y, Y)
    over = np.abs(got - y) - (2.0 ** -24 * np.abs(y) + 1e-12 * Yf[..., None])
    print(f"{shape}: max |oracle - y| / Yframe = {np.max(np.abs(got - y) / np.where(Yf > 0, Yf, 1.0)[..., None]):.2e}, "
          f"largest excess over the bound {over.max():.2e}")
    assert (over <= 0.0).all()


def test_reference_follows_the_in_kernel_stream():
    B, T, hop, F = 2, 3, 16, 9
    H = R.gpu_H(B, T, F, 5)
    sd, off = 0xDD5B0A7D, 2**32 - 5
    y, Y = R.noise_fwd_fp64(H, hop, seed=sd, offset=off)
    got = oracle.noise_forward(H, None, hop, seed=sd, offset=off).reshape(B, T, hop)
    Yf, _ = R.frame_figures(y, Y)
    assert (np.abs(got - y) <= 2.0 ** -24 * np.abs(y) + 1e-12 * Yf[..., None]).all()
    y2, _ = R.noise_fwd_fp64(H, hop, uniform=oracle.philox_uniform(sd, off, B, T, hop))
    assert np.array_equal(y, y2)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "g8_noise_*.npz"))))
def test_reference_is_the_reference_modules_output(path):
    """The reference module's own fp32 torch output: per frame max |err| <= 2e-6 of the frame's fp64 peak."""
    with np.load(path, allow_pickle=False) as z:
        H, u, want, hop = z["H"], z["uniform"], z["y"], int(z["hop"])
    B, T, F = H.shape
    y, Y = R.noise_fwd_fp64(H, hop, uniform=u)
    _, peak = R.frame_figures(y, Y)
    err = np.abs(want.reshape(B, T, hop) - y).max(axis=-1)
    print(f"{os.path.basename(path)}: worst frame {np.max(err / peak):.2e} of its peak")
    assert (err <= R.FRAME_REL * peak).all()


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_the_yardstick_bounds_the_value_and_vanishes_only_with_it(shape):
    H, u, y, Y = case(shape)
    assert (np.abs(y) <= Y * (1 + 1e-12)).all()
    assert (y[Y == 0.0] == 0.0).all()
    zero = ~H.any(axis=-1)
    assert zero.sum() == (H.shape[0] * H.shape[1] > 1) and (Y[zero] == 0.0).all() and (y[zero] == 0.0).all()
    B, T, hop, F = shape
    if (F - 1) % hop == 0:                                         # the tap at lag 0 is src = S/2 mod hop = 0, hann32[0] == 0: an exact zero
        assert (Y[..., 0] == 0.0).all() and (y[..., 0] == 0.0).all()
    else:
        assert (Y[~zero][:, 0] > 0.0).all()


@pytest.mark.parametrize("shape", [(2, 5, 7, 33), (2, 4, 100, 33), (2, 5, 128, 65), (2, 6, 16, 2)])
def test_scaling_one_frame_scales_that_frame_exactly(shape):
    B, T, hop, F = shape
    H, u, y, Y = case(shape)
    for k in (-20, 7):
        H2 = H.copy()
        H2[1, 2] *= np.float32(2.0 ** k)
        y2, Y2 = R.noise_fwd_fp64(H2, hop, uniform=u)
        assert np.array_equal(y2[1, 2], y[1, 2] * 2.0 ** k) and np.array_equal(Y2[1, 2], Y[1, 2] * 2.0 ** k)
        other = np.ones((B, T), bool)
        other[1, 2] = False
        assert np.array_equal(y2[other], y[other]) and np.array_equal(Y2[other], Y[other])


@pytest.mark.parametrize("shape", [(2, 5, 7, 33), (2, 4, 100, 33), (2, 5, 128, 65), (2, 6, 16, 2), (1, 3, 512, 195)])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_reach_of_a_non_finite_magnitude(shape, value):
    B, T, hop, F = shape
    H, u, y, Y = case(shape)
    H2 = H.copy()
    H2[B - 1, 1, F // 3] = value
    y2, Y2 = R.noise_fwd_fp64(H2, hop, uniform=u)
    bad = np.zeros((B, T), bool)
    bad[B - 1, 1] = True
    assert (~np.isfinite(y2[bad])).all() and (~np.isfinite(Y2[bad])).all()
    assert np.array_equal(y2[~bad], y[~bad]) and np.array_equal(Y2[~bad], Y[~bad])
    want = oracle.noise_forward(H2, u, hop).reshape(B, T, hop)       # the oracle agrees on the reach
    assert (~np.isfinite(want[bad])).all() and np.isfinite(want[~bad]).all()


def one_digit_up(v):
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e


WAVE_SHAPE = (128, 65)          # (hop, F) of the wavefront form, the one direct kernel whose table still holds an fp32 cosine (cospif)


def test_device_bounds():
    """TOL_SAMPLE and TOL_FRAME, from the reference's arithmetic on the CPU and never from the kernels.

    TOL_SAMPLE (Batched, Frame and Wave kernels, per sample against Y[n]): the definition as a chain of fp32 multiply-adds
    (direct_fp32) on the device tests' inputs; its largest deviation from fp64 relative to Y[n], times two because any other summation
    order is as valid, plus the cosines' definitional term: a kernel whose cosine is cospif in fp32 where the reference rounds an fp64
    cosine (the comment above NOISE_BWD_TOL in fuzz_parity.py) may differ by an ulp on every cosine, which moves the result by the
    amount measured here.  Of the forward's direct kernels only the wavefront form (hop 128 / 65 bands, the whole window used) still
    does that; the frame and batched kernels round an fp64 cosine into their table, which is hann32's own.  So the term is measured
    at that one shape.  (Elsewhere it would be no constant share of Y[n]: where a cropped frame uses only the window's edge, one ulp
    on the window's cosine is 2.9e-4 of Y[n] at 1025 bands / hop 1024 and 2.2e-5 at 129 bands / hop 64 -- printed below, not used.)
    TOL_FRAME (every form, per frame against Yframe): the reference module's own fp32 FFT pipeline in torch (fft_fp32), times two.

    Measured here (the shapes of GPU_SHAPES at up to DERIVE_FRAMES frames; fft_fp32 under MKL_CBWR=COMPATIBLE, which
    tests/conftest.py sets; with MKL's default code path on the same host its worst is 2.44e-7, and 2 x that rounds up to 5e-7 too):
      direct_fp32: worst 1.055e-6 of Y[n] (hop 2048 / 1025 bands; 6.1e-7 at hop 512 / 195 bands, 2e-8 .. 5e-7 elsewhere);
                   one ulp on every cosine at hop 128 / 65 bands: 7.67e-8 of Y[n];
                   2 x 1.055e-6 + 7.67e-8 = 2.19e-6 -> TOL_SAMPLE = 3e-6
      fft_fp32:    worst 2.22e-7 of Yframe (hop 512 / 3 bands; 1.4e-7 at 2 bands, <= 8e-8 from 9 bands on, <= 1.2e-8 from 65 on);
                   2 x 2.22e-7 = 4.44e-7 -> TOL_FRAME = 5e-7
      direct_fp32 per frame: at most 8.2e-8 of Yframe, inside TOL_FRAME / 2.
    FRAME_REL = 2e-6 of a frame's own fp64 peak is the project's existing noise contract; no frame of GPU_SHAPES is exempt from it
    (peak < 1e-3 Yframe) apart from the deliberately zero ones and those of hop 1, whose only sample is an exact zero: the smallest
    peak / Yframe is 0.0018 (hop 1024 / 1025 bands)."""
    worst_d = worst_f = def_d = worst_efd = 0.0
    least = np.inf
    for i, full in enumerate(R.GPU_SHAPES):
        B, T, hop, F, fam = R.derive_shape(full)
        H, u = R.gpu_H(B, T, F, 300 + i), R.gpu_uniform(B, T, hop, 400 + i)
        y, Y = R.noise_fwd_fp64(H, hop, uniform=u)
        Yf, peak = R.frame_figures(y, Y)
        live = H.any(axis=-1) & (Yf > 0)
        exempt = live & (peak < R.FRAME_FLOOR * Yf)
        assert not exempt.any(), (full, np.argwhere(exempt))
        low = float((peak[live] / Yf[live]).min()) if live.any() else float("nan")
        least = min(least, low) if live.any() else least
        ef = float(R.ratio(R.fft_fp32(H, hop, uniform=u), y, Yf).max())
        line = f"{full}: fft_fp32 {ef:.3e} of Yframe"
        worst_f = max(worst_f, ef)
        if fam == "direct":
            d = R.direct_fp32(H, hop, uniform=u)
            ed = float(R.ratio(d[..., None], y[..., None], Y).max())
            ud = max(float(R.ratio(R.direct_fp32(H, hop, uniform=u, ulps=s)[..., None], d[..., None], Y).max()) for s in (1, -1))
            efd = float(R.ratio(d, y, Yf).max())
            line += f"; direct_fp32 {ed:.3e} of Y[n] ({efd:.3e} of Yframe), one ulp on every cosine {ud:.3e}"
            worst_d, worst_efd = max(worst_d, ed), max(worst_efd, efd)
            if (hop, F) == WAVE_SHAPE:
                def_d = max(def_d, ud)
        print(line + f"; smallest peak / Yframe {low:.4f}")
    assert def_d > 0.0                                               # the wavefront form's shape is among GPU_SHAPES
    bs, bf = 2 * worst_d + def_d, 2 * worst_f
    print(f"per sample 2 x {worst_d:.3e} + {def_d:.3e} = {bs:.3e} -> TOL_SAMPLE = {R.TOL_SAMPLE:g}; "
          f"per frame 2 x {worst_f:.3e} = {bf:.3e} -> TOL_FRAME = {R.TOL_FRAME:g}; direct_fp32 per frame {worst_efd:.3e}; "
          f"smallest peak / Yframe {least:.4f}")
    assert math.isclose(R.TOL_SAMPLE, one_digit_up(bs), rel_tol=1e-9)
    assert math.isclose(R.TOL_FRAME, one_digit_up(bf), rel_tol=1e-9)
    assert worst_efd <= R.TOL_FRAME / 2                              # the direct class lies inside the frame bound as well
    assert R.TOL_FRAME <= R.FRAME_REL                                # the project's noise contract
    assert least >= R.FRAME_FLOOR
