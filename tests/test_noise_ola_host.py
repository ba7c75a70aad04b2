"""The overlap-add filtered noise (include/ddsp_hip.h: ddsp_noise_ola_*) on the host, in fp64: the
reference of tests/noise_ola_reference.py against a brute-force loop, against the oracle's impulse responses and against
torch.autograd; the statistical claims that motivate the mode, with the oracle's truncated noise as the control that fails them;
the derivation of the device bounds TOL_Y and TOL_DH; the ABI.  Every test prints its figures before it asserts."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import noise_ola_reference as ref
from oracle import torch_restatement as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ddsp_[a-z0-9_]+)\s*\(", text))


def brute_force(H, x, hop):
    """The definition, one term at a time.  H [T, F], x [T hop] -> y [T hop]."""
    T, F = H.shape
    M, N = 2 * (F - 1), T * hop
    y = np.zeros(N)
    for n in range(N):
        for e in range(-M // 2, M // 2):
            m = n - e
            if not 0 <= m < N:
                continue
            t = m // hop
            s = 0.0
            for k in range(F):
                s += (1.0 if k in (0, F - 1) else 2.0) * H[t, k] * math.cos(2 * math.pi * k * e / M)
            y[n] += (0.5 + 0.5 * math.cos(2 * math.pi * e / M)) * s / M * x[m]
    return y


@pytest.mark.parametrize("T,hop,F", [(4, 7, 5), (3, 16, 9)])
def test_reference_is_the_triple_loop(T, hop, F):
    rng = np.random.default_rng(T)
    H = rng.random((1, T, F))
    u = rng.random((1, T, hop), dtype=np.float32)
    y, Y = ref.ola_fp64(H, hop, uniform=u)
    x = ref.draw(1, T, hop, u).astype(np.float64).reshape(-1)
    err = np.abs(y[0] - brute_force(H[0], x, hop)).max()
    print(f"T {T}, hop {hop}, F {F}: |reference - triple loop| = {err:.2e}, max |y| / Yf = {(np.abs(y) / Y).max():.3f}")
    assert err <= 1e-14
    assert (np.abs(y) <= Y * (1 + 1e-12)).all()                  # the yardstick bounds the value


@pytest.mark.parametrize("F,hop", [(33, 100), (65, 128), (195, 512)])
def test_responses_are_the_oracles(F, hop):
    """h of unit vectors against the oracle's amp_to_impulse_response: hop >= M here, so its pad and second roll only place the
    M taps, e at position e mod hop."""
    want = oracle.impulse_response(torch.eye(F, dtype=torch.float64), hop).numpy()            # [F, hop]
    h = ref.responses(np.eye(F))
    P = F - 1
    got = np.zeros((F, hop))
    got[:, np.arange(-P + 1, P) % hop] = h
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"F {F}, hop {hop}: |h - oracle| / max = {err:.2e}")
    assert err <= 1e-12


def torch_ola(H, x, hop):
    """A torch fp64 restatement for autograd: each frame's response convolved with its own hop samples, overlap-added."""
    B, T, F = H.shape
    P = F - 1
    M = 2 * P
    e = torch.arange(-P + 1, P, dtype=torch.float64)
    k = torch.arange(F, dtype=torch.float64)
    c = torch.full((F,), 2.0, dtype=torch.float64)
    c[0] = c[F - 1] = 1.0
    C = torch.cos(2 * math.pi * k[:, None] * e[None, :] / M) * (c / M)[:, None]
    h = (H @ C) * (0.5 + 0.5 * torch.cos(2 * math.pi * e / M))                                # [B, T, 2P - 1]
    y = torch.zeros(B, T * hop + 2 * P - 2, dtype=torch.float64)
    for t in range(T):
        for j in range(hop):
            y[:, t * hop + j:t * hop + j + 2 * P - 1] = y[:, t * hop + j:t * hop + j + 2 * P - 1] + h[:, t] * x[:, t, j:j + 1]
    return y[:, P - 1:P - 1 + T * hop]


@pytest.mark.parametrize("shape", [(2, 4, 7, 5), (1, 3, 16, 9), (1, 5, 8, 17)])
def test_backward_is_autograd(shape):
    B, T, hop, F = shape
    rng = np.random.default_rng(11)
    u = rng.random((B, T, hop), dtype=np.float32)
    g = rng.standard_normal((B, T * hop)).astype(np.float32)
    H = torch.from_numpy(rng.random((B, T, F))).requires_grad_()
    x = torch.from_numpy(ref.draw(B, T, hop, u).astype(np.float64))
    y = torch_ola(H, x, hop)
    fwd = np.abs(y.detach().numpy() - ref.ola_fp64(H.detach().numpy(), hop, uniform=u)[0]).max()
    y.backward(torch.from_numpy(g.astype(np.float64)))
    dH, Yb = ref.ola_grad_fp64(g, F, hop, uniform=u)
    err = ref.ratio(H.grad.numpy(), dH, Yb[..., None])
    print(f"{shape}: torch restatement against the reference {fwd:.2e}; |dH - autograd| / Yb = {err:.2e}; "
          f"max |dH| / Yb = {(np.abs(dH) / Yb[..., None]).max():.3f}")
    assert fwd <= 1e-13
    assert err <= 1e-12
    assert (np.abs(dH) <= Yb[..., None] * (1 + 1e-12)).all()


@functools.lru_cache(maxsize=None)
def statistics():
    """2048 frames of the low-pass H at (65, 128), one fixed draw: (overlap-add figures, the oracle's truncated figures)."""
    F, hop, T = 65, 128, 2048
    Hs = ref.lowpass_H(F)
    u = np.random.default_rng(7).random((1, T, hop))
    H = np.tile(Hs, (1, T, 1))
    y, _ = ref.ola_fp64(H, hop, x=2 * u - 1)
    yt = oracle.filtered_noise(torch.from_numpy(H), hop, uniform=torch.from_numpy(u))[0].numpy()
    return ((ref.position_variance_ratio(y[0], hop), ref.welch_distance(y[0], Hs, hop)),
            (ref.position_variance_ratio(yt, hop), ref.welch_distance(yt, Hs, hop)))


def test_the_noise_floor_is_stationary():
    (ola, _), (trunc, _) = statistics()
    print(f"variance by position in the frame, min / max: overlap-add {ola:.3f}, the oracle's truncated noise {trunc:.3f}")
    assert ola >= 0.8
    assert trunc < 0.8                                            # the control: the truncated form is modulated at the frame rate


def test_the_spectrum_is_the_filters():
    (_, ola), (_, trunc) = statistics()
    print(f"Welch spectrum against 1/3 |DTFT h|^2, relative l2: overlap-add {ola:.4f}, the oracle's truncated noise {trunc:.3f}")
    assert ola <= 0.05
    assert trunc > 0.05


def test_reach_of_a_non_finite_value():
    T, hop, F = 6, 16, 9
    rng = np.random.default_rng(3)
    H = rng.random((1, T, F))
    u = rng.random((1, T, hop), dtype=np.float32)
    H[0, 2, 4] = np.nan
    y, _ = ref.ola_fp64(H, hop, uniform=u)
    lo, hi = ref.reach(2, T, hop, F)
    assert (lo, hi) == (2 * hop - (F - 1) + 1, 3 * hop + (F - 1) - 1)
    assert np.isnan(y[0, lo:hi]).all() and np.isfinite(y[0, :lo]).all() and np.isfinite(y[0, hi:]).all()
    g = rng.standard_normal((1, T * hop)).astype(np.float32)
    g[0, 36] = np.nan
    dH, _ = ref.ola_grad_fp64(g, F, hop, uniform=u)
    hit = np.array([ref.reach(t, T, hop, F)[0] <= 36 < ref.reach(t, T, hop, F)[1] for t in range(T)])
    assert np.isnan(dH[0, hit]).all() and np.isfinite(dH[0, ~hit]).all() and hit.sum() == 2


def one_digit_up(v):
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e


def test_device_bound():
    """TOL_Y and TOL_DH: the definition in the kernels' arithmetic (fp32 cosine table and window, every sum a chain of fp32
    multiply-adds in the kernels' order) on the device tests' own inputs; its largest deviation from fp64 relative to the
    yardsticks, times two because any other summation order is as valid, plus the window's definitional term: the kernels' cosine
    is cospif in fp32, not a rounded fp64 cosine, and one ulp on every cosine moves the result by the amount measured here."""
    worst_y = worst_dh = def_y = def_dh = 0.0
    for shape in ref.GPU_SHAPES:
        B, T, hop, F = shape
        H, u, g = ref.gpu_H(shape), ref.gpu_uniform(shape), ref.gpu_grad(shape)
        y, Yf = ref.ola_fp64(H, hop, uniform=u)
        ye = ref.ola_fp32(H, hop, uniform=u)
        dH, Yb = ref.ola_grad_fp64(g, F, hop, uniform=u)
        de = ref.ola_grad_fp32(g, F, hop, uniform=u)
        ey, ed = ref.ratio(ye, y, Yf), ref.ratio(de, dH, Yb[..., None])
        uy = max(ref.ratio(ref.ola_fp32(H, hop, uniform=u, ulps=s), ye, Yf) for s in (1, -1))
        ud = max(ref.ratio(ref.ola_grad_fp32(g, F, hop, uniform=u, ulps=s), de, Yb[..., None]) for s in (1, -1))
        print(f"{shape}: fp32 emulation against fp64: y {ey:.3e} of Yf (absolute {np.abs(ye - y).max():.2e}, max |y| "
              f"{np.abs(y).max():.2f}), dH {ed:.3e} of Yb; one ulp on every cosine: y {uy:.3e}, dH {ud:.3e}")
        for b, t in ref.zero_frames(H):                           # a zero frame contributes exact zeros in fp32 as well
            if T == 1:
                assert (ye[b] == 0).all()
        worst_y, worst_dh, def_y, def_dh = max(worst_y, ey), max(worst_dh, ed), max(def_y, uy), max(def_dh, ud)
    by, bd = 2 * worst_y + def_y, 2 * worst_dh + def_dh
    print(f"forward 2 x {worst_y:.3e} + {def_y:.3e} = {by:.3e} -> TOL_Y = {ref.TOL_Y:g}; "
          f"backward 2 x {worst_dh:.3e} + {def_dh:.3e} = {bd:.3e} -> TOL_DH = {ref.TOL_DH:g}")
    assert math.isclose(ref.TOL_Y, one_digit_up(by), rel_tol=1e-9)
    assert math.isclose(ref.TOL_DH, one_digit_up(bd), rel_tol=1e-9)
    assert ref.TOL_Y <= 2e-6 and ref.TOL_DH <= 2e-6               # the project's noise contract


def test_abi():
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    new = ("ddsp_noise_ola_workspace_bytes", "ddsp_noise_ola_forward", "ddsp_noise_ola_backward")
    raw = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in new:
        assert name in declared_symbols() and name in ddsp._lib.EXPORTS and hasattr(raw, name), name
    fwd = list(ddsp._lib.SIGNATURES["ddsp_noise_forward_ws"])
    bwd = list(ddsp._lib.SIGNATURES["ddsp_noise_backward_ws"])
    assert list(ddsp._lib.SIGNATURES["ddsp_noise_ola_forward"]) == fwd                       # the argument lists mirror the truncated form's
    assert list(ddsp._lib.SIGNATURES["ddsp_noise_ola_backward"]) == bwd


def test_the_c_entries_validate_before_the_device():
    """No GPU here: every one of these returns before a launch (the pointer is a host address nothing reads)."""
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 40
    fwd = lambda *a: L.ddsp_noise_ola_forward(*a)                 # noqa: E731
    bwd = lambda *a: L.ddsp_noise_ola_backward(*a)                # noqa: E731
    assert fwd(p, None, p, 1, 4, 258, 128, 0, 0, None, 0, p, big, None) == ERANGE
    assert fwd(p, None, p, 1, 4, 65, 1025, 0, 0, None, 0, p, big, None) == ERANGE
    assert fwd(p, None, p, 1, 4, 1, 128, 0, 0, None, 0, p, big, None) == EINVAL
    assert fwd(p, None, p, 1 << 20, 1 << 11, 65, 128, 0, 0, None, 0, p, big, None) == ERANGE       # B T = 2^31
    assert fwd(None, None, p, 1, 4, 65, 128, 0, 0, None, 0, p, big, None) == EINVAL
    assert fwd(p, None, None, 1, 4, 65, 128, 0, 0, None, 0, p, big, None) == EINVAL
    assert fwd(p, None, p, 1, 0, 65, 128, 0, 0, None, 0, p, big, None) == EINVAL
    assert fwd(p, None, p, 1, 4, 65, 0, 0, 0, None, 0, p, big, None) == EINVAL
    assert fwd(p, None, p, 1, 4, 65, 128, 0, 0, None, 0, None, 0, None) == EINVAL                 # the workspace is required
    assert fwd(p, None, p, 1, 4, 65, 128, 0, 0, None, 0, p, 16, None) == EINVAL                   # ... at its full size
    assert fwd(p, p, p, 0, 4, 65, 128, 0, 0, p, 0, None, 0, None) == EINVAL                       # a draw and a counter
    assert fwd(None, None, None, 0, 4, 65, 128, 0, 0, None, 0, None, 0, None) == 0                # an empty batch
    assert bwd(p, None, p, 1, 4, 258, 128, 0, 0, None, p, big, None) == ERANGE
    assert bwd(p, None, p, 1, 4, 65, 1025, 0, 0, None, p, big, None) == ERANGE
    assert bwd(p, None, p, 1, 4, 1, 128, 0, 0, None, p, big, None) == EINVAL
    assert bwd(None, None, p, 1, 4, 65, 128, 0, 0, None, p, big, None) == EINVAL
    assert bwd(p, None, p, 1, 4, 65, 128, 0, 0, None, None, 0, None) == EINVAL
    assert bwd(p, p, p, 0, 4, 65, 128, 0, 0, p, None, 0, None) == EINVAL
    assert bwd(None, None, None, 0, 4, 65, 128, 0, 0, None, None, 0, None) == 0
    ws = L.ddsp_noise_ola_workspace_bytes
    assert ws(2, 5, 65, 128) >= 2 * 5 * 64 * 4 and ws(1, 4, 258, 128) == 0 and ws(1, 4, 65, 1025) == 0 and ws(0, 4, 65, 128) == 0


class Conf:
    def __init__(self, hop_length, **extra):
        self.n_harmonics, self.sample_rate, self.hop_length = 4, 16000, hop_length
        self.__dict__.update(extra)


def test_the_flag_on_the_host():
    """The module reads its flag from the argument, else from the configuration, else it is off; CPU tensors raise."""
    assert ddsp.FilteredNoise(Conf(128)).overlap_add is False
    assert ddsp.FilteredNoise(Conf(128, noise_overlap_add=True)).overlap_add is True
    assert ddsp.FilteredNoise(Conf(128, noise_overlap_add=True), overlap_add=False).overlap_add is False
    assert ddsp.FilteredNoise(Conf(128), overlap_add=True).overlap_add is True
    H = torch.ones(1, 3, 9)
    with pytest.raises(ddsp._lib.DdspHipError):
        ddsp.noise_forward(H, 16, overlap_add=True)
    with pytest.raises(ddsp._lib.DdspHipError):
        ddsp.noise_backward(torch.ones(1, 48), 16, 9, overlap_add=True)
    with pytest.raises(ddsp._lib.DdspHipError):
        ddsp.FilteredNoise(Conf(16), overlap_add=True)({"H": H.requires_grad_()})
