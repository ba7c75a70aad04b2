"""CPU checks of the fp64 filtered-noise gradient reference (tests/noise_grad_reference.py) that tests/test_gpu_noise_backward.py
holds the HIP backward to: against the reference-autograd fixtures G10 / G17, against fp64 autograd of the torch restatement on
shapes that crop, pad, have an even F, F = 2 or an odd hop, the adjoint identity with the oracle's forward, the yardstick's bound,
and the in-kernel draw.  No GPU needed."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import noise_grad_reference as R
from ddsp_pytorch_amd import synthetic as syn
from oracle import oracle
from oracle import torch_restatement as tr


def _case(B, T, F, hop, seed, spread=True):
    rng = np.random.default_rng(seed)
    Hm = syn.controller_range(rng.standard_normal((B, T, F), dtype=np.float32))
    u = rng.random((B, T, hop), dtype=np.float32)
    gy = rng.standard_normal((B, T, hop)).astype(np.float32)
    if spread:                                                  # frame levels over seven decades
        gy *= (10.0 ** rng.uniform(-4, 3, size=(B, T, 1))).astype(np.float32)
    return Hm, u, gy.reshape(B, T * hop)


@pytest.mark.parametrize("name", ["g10_noise_grad_hop128", "g10_noise_grad_hop64", "g17_noise_grad_hop512_f257",
                                  "g17_noise_grad_hop512_f195"])
def test_matches_the_reference_autograd_fixtures(name):
    g = load_golden(name)
    hop, F = int(g["hop"]), g["H"].shape[-1]
    dH, Y = R.noise_grad_fp64(g["g"], F, hop, uniform=g["uniform"])
    assert np.isfinite(dH).all() and (Y > 0).all()
    assert R.ratio(g["grad_H"], dH, Y).max() <= 1e-7


# (F, hop): crop (R < S), pad (R > S), an even F (S/2 odd), F = 2, odd hops, R = S
SHAPES = [(65, 40), (33, 100), (64, 128), (2, 8), (2, 5), (9, 7), (129, 256), (10, 1), (200, 480)]


@pytest.mark.parametrize("F,hop", SHAPES)
def test_matches_fp64_autograd_of_the_restatement(F, hop, monkeypatch):
    B, T = 2, 5
    Hm, u, gy = _case(B, T, F, hop, 10 * F + hop)
    dH, Y = R.noise_grad_fp64(gy, F, hop, uniform=u)

    def grad(window_fp32):
        if window_fp32:     # the oracle's fp32 window (R.hann32): fp64 autograd with that window is the same operation
            monkeypatch.setattr(torch, "hann_window", lambda n, dtype=None: torch.from_numpy(R.hann32(n)).to(dtype))
        H = torch.from_numpy(Hm).double().requires_grad_()
        (tr.filtered_noise(H, hop, uniform=torch.from_numpy(u)) * torch.from_numpy(gy).double()).sum().backward()
        monkeypatch.undo()
        return H.grad.numpy()

    assert R.ratio(grad(True), dH, Y).max() <= 1e-13
    # the restatement as it stands (an fp64 window: short windows differ from the fp32 one by up to ~3e-8 of the yardstick)
    assert R.ratio(grad(False), dH, Y).max() <= 1e-7


@pytest.mark.parametrize("F,hop", [(65, 128), (33, 100), (64, 40), (2, 8), (195, 512)])
def test_adjoint_identity_with_the_oracle_forward(F, hop):
    """sum g . y(H) = sum dH . H: y is linear in H, and dH is its adjoint applied to g.  y is the oracle's fp32 output (fp64 sums)."""
    B, T = 2, 6
    Hm, u, gy = _case(B, T, F, hop, 7 * F + hop, spread=False)
    y = oracle.noise_forward(Hm, u, hop).astype(np.float64)
    dH, _ = R.noise_grad_fp64(gy, F, hop, uniform=u)
    lhs = float((gy.astype(np.float64) * y).sum())
    rhs = float((dH * Hm.astype(np.float64)).sum())
    bound = float((np.abs(gy) * np.abs(y)).sum()) * 2.0 ** -24 + 1e-12 * float(np.abs(dH * Hm).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("F,hop,seed", [(65, 128, 1), (64, 40, 2), (257, 512, 3), (9, 7, 4), (2, 8, 5)])
def test_yardstick_bounds_every_gradient_under_sign_flips(F, hop, seed):
    B, T = 2, 4
    _, u, gy = _case(B, T, F, hop, seed)
    dH, Y = R.noise_grad_fp64(gy, F, hop, uniform=u)
    assert (np.abs(dH) <= Y[..., None]).all()
    rng = np.random.default_rng(seed + 100)
    for _ in range(4):
        flip = gy * rng.choice(np.array([-1.0, 1.0], np.float32), size=gy.shape)
        dHf, Yf = R.noise_grad_fp64(flip, F, hop, uniform=u)
        assert np.array_equal(Yf, Y) or np.allclose(Yf, Y, rtol=1e-13, atol=0.0)
        assert (np.abs(dHf) <= Y[..., None]).all()


@pytest.mark.parametrize("F,hop,offset", [(65, 128, 0), (33, 100, 2**32 - 5), (257, 512, (7 << 32) + 3)])
def test_philox_draw_equals_the_injected_draw(F, hop, offset):
    B, T, seed = 2, 3, 0x1234ABCD5678
    _, _, gy = _case(B, T, F, hop, F)
    u = oracle.philox_uniform(seed, offset, B, T, hop)
    a = R.noise_grad_fp64(gy, F, hop, seed=seed, offset=offset)
    b = R.noise_grad_fp64(gy, F, hop, uniform=u)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_non_finite_gradient_spreads_over_its_frame_only():
    B, T, F, hop = 2, 4, 33, 64
    _, u, gy = _case(B, T, F, hop, 77, spread=False)
    gy[0, 1 * hop + 63] = np.nan                                    # the last sample of a frame: every lag sees it
    gy[1, 2 * hop] = np.inf                                         # the first sample: only lag 0 sees it
    dH, _ = R.noise_grad_fp64(gy, F, hop, uniform=u)
    bad = np.zeros((B, T), bool)
    bad[0, 1] = bad[1, 2] = True
    assert (~np.isfinite(dH[bad])).all()
    assert np.isfinite(dH[~bad]).all()


def test_chunking_does_not_change_the_result(monkeypatch):
    F, hop = 65, 128
    _, u, gy = _case(3, 11, F, hop, 8)
    a = R.noise_grad_fp64(gy, F, hop, uniform=u)
    monkeypatch.setattr(R, "CHUNK_ELEMS", 5 * hop)
    b = R.noise_grad_fp64(gy, F, hop, uniform=u)
    assert np.allclose(a[0], b[0], rtol=0, atol=1e-12 * np.abs(a[0]).max()) and np.allclose(a[1], b[1], rtol=1e-12)
