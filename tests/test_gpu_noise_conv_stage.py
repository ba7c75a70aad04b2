"""The convolution stage of the hop-128 noise kernel on its own (csrc/ddsp_noise_wave.hip: conv_half and stage_acc, 576
v_mfma_f32_4x4x1_16b_f32 per group of 16 frames), through the test hook ddsp_noise_conv_probe, against an fp64 convolution.

y[b][n] = sum_{m <= n} k[b][m] x[b][n - m], one group: k, x, y [16][128].  Every output is one fp32 fused multiply-add chain over its
n + 1 products, so (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: an inner product accumulated in any order)
|y - exact| <= gamma_{n+1} sum |k_m| |x_{n-m}| with gamma_t = t u / (1 - t u), u = 2^-24: the bound asserted is (n + 1) 2^-24 sum |k||x|
times 1 / (1 - 128 u), derived and not tuned."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp

pytestmark = pytest.mark.gpu
FG, N = 16, 128


def probe(k, x):
    L = ddsp._lib.lib()
    kd, xd = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for v in (k, x))
    y = torch.full((FG, N), float("nan"), device="cuda")
    assert L.ddsp_noise_conv_probe(kd.data_ptr(), xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return y.cpu().numpy()


def exact(k, x):
    """-> (fp64 truncated convolution, sum of the products' magnitudes), [16][128] each"""
    k, x = k.astype(np.float64), x.astype(np.float64)
    y = np.stack([np.convolve(k[b], x[b])[:N] for b in range(FG)])
    mag = np.stack([np.convolve(np.abs(k[b]), np.abs(x[b]))[:N] for b in range(FG)])
    return y, mag


@pytest.fixture(scope="module")
def taps():
    return np.random.default_rng(128).standard_normal((FG, N)).astype(np.float32)      # distinct in every frame


@pytest.mark.parametrize("p", [0, 1, 3, 4, 15, 16, 17, 63, 64, 127])
def test_unit_impulse_gives_the_shifted_taps_exactly(taps, p):
    """x = delta_p: every output has ONE non-zero product, k[n - p] * 1, so the result is the taps shifted by p, bit for bit.  Pins
    the lane layout of A, B and D, every window and every boundary of the steps (c = 16 a + mu)."""
    x = np.zeros((FG, N), np.float32)
    x[:, p] = 1.0
    want = np.zeros((FG, N), np.float32)
    want[:, p:] = taps[:, :N - p]
    got = probe(taps, x)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_unit_tap_gives_the_noise_exactly(taps):
    """The mirror image: k = delta_q with a different q in every frame returns that frame's noise shifted by q."""
    k = np.zeros((FG, N), np.float32)
    want = np.zeros((FG, N), np.float32)
    for b in range(FG):
        q = (b * 9) % N
        k[b, q] = 1.0
        want[b, q:] = taps[b, :N - q]
    assert np.array_equal(probe(k, taps), want)


def test_random_frames_within_the_fma_chain_bound_and_independent_of_their_neighbours(taps):
    rng = np.random.default_rng(4)
    x = (rng.random((FG, N), dtype=np.float32) * 2.0 - 1.0).astype(np.float32)
    k = taps.copy()
    k[3] = 0.0                                            # a frame of zeros
    k[7], x[7] = k[6], x[6]                               # frame 7 = frame 6 ...
    got = probe(k, x)
    y, mag = exact(k, x)
    u = 2.0 ** -24
    bound = (np.arange(N) + 1) * u / (1 - N * u) * mag
    err = np.abs(got.astype(np.float64) - y)
    print("worst error / bound:", float(np.max(err[bound > 0] / bound[bound > 0])))
    assert np.all(err <= bound)
    assert not got[3].any() and np.array_equal(got[7], got[6])
    # ... then 2^60 times its neighbours' magnitude: the blocks of the instruction are independent, so frame 7 scales exactly and no
    # other frame changes by a bit
    x2 = x.copy()
    x2[7] = x[7] * np.float32(2.0 ** 60)
    got2 = probe(k, x2)
    others = [b for b in range(FG) if b != 7]
    assert np.array_equal(got2[others], got[others])
    assert np.array_equal(got2[7], got[7] * np.float32(2.0 ** 60))
    y2, mag2 = exact(k, x2)
    assert np.all(np.abs(got2.astype(np.float64) - y2) <= (np.arange(N) + 1) * u / (1 - N * u) * mag2)
