"""Griffin-Lim on the MI355X: the HIP path (csrc/ddsp_griffinlim.hip) against the G27 fixtures per iteration count, against the
device's own stock loop on random shapes, run to run, in convergence, and the stock-loop fallback for n_fft the kernels do
not take.  Tolerance: 4x the fixture's (or the case's) fp32-vs-fp64 spread, the encoder's rule.  These are free-running
comparisons of a chaotic iteration; the three kernels are held to fp64 one at a time, and one teacher-forced step at a time
along the same G27 trajectories, in tests/test_gpu_griffinlim_stages.py."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import spectral

pytestmark = pytest.mark.gpu

CASES = ["n2048_h256", "n1024_h128_p2", "n512_h64", "n512_w400_h100"]
DEV = torch.device("cuda", 0)


def _args(g):
    n_fft, hop, win_length, length = (int(v) for v in g["params"])
    return dict(n_fft=n_fft, hop_length=hop, win_length=win_length, power=float(g["power"]), momentum=float(g["momentum"]),
                length=None if length < 0 else length, rand_init=False)


def _exact64(spec, window, angles, n_fft, hop_length, win_length, power, n_iter, momentum, length):
    """The loop in fp64 throughout, on the device (the yardstick of the spread)."""
    shape = spec.shape
    S = spec.reshape(-1, *shape[-2:]).double().pow(1 / power)
    ang = angles.reshape(S.shape).to(torch.complex128)
    w = window.double()
    kw = dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=w)
    prev = None
    for _ in range(n_iter):
        y = torch.istft(S * ang, length=length, **kw)
        R = torch.stft(y, center=True, pad_mode='reflect', onesided=True, return_complex=True, **kw)
        a = R - (momentum / (1 + momentum)) * prev if (momentum and prev is not None) else R
        ang = a / (a.abs() + 1e-16)
        prev = R
    y = torch.istft(S * ang, length=length, **kw)
    return y.reshape(shape[:-2] + y.shape[-1:])


# Measured on the MI355X, err / spread per iteration count: <= 1.8 everywhere except n2048_h256 (momentum 0.99) from iteration 6
# on, where one near-cancelling bin of R - c R_prev takes a different phase in the HIP run than in the stock fp32 runs and the
# ratio jumps from 0.68 to 10 and then drifts to 14 .. 38.  Those iterations are held to 64x; the spectral
# convergence of the same path is checked separately (test_convergence_no_worse_than_stock).  It is conditioning, not the
# 2048-point kernels: each single step from the fp64 trajectory's state is as accurate on the device as the stock fp32 step
# (tests/test_gpu_griffinlim_stages.py::test_teacher_forced_steps_along_g27; kappa reaches 1.4e4 at iteration 6).
LOOSE = {("n2048_h256", n): 64 for n in range(6, 17)}


@pytest.mark.parametrize("case", CASES)
def test_hip_matches_g27_per_iteration(golden, case):
    """Every iteration count 0 .. 16 against the fp64 loop: within 4x the spread of the stock fp32 loop from the fp64 one, the
    fixture's (CPU) or the device's own, whichever is larger -- with momentum 0.99 the bins whose R - c R_prev nearly cancels
    carry phase errors that grow from one iteration to the next, and one fp32 run is one sample of that growth."""
    g = golden("g27_" + case)
    spec, window, angles = (torch.from_numpy(g[k]).to(DEV) for k in ("spec", "window", "angles"))
    a = _args(g)
    assert spectral.griffinlim_uses_hip(DEV, torch.float32, a["n_fft"], a["win_length"])
    kw = {k: v for k, v in a.items() if k != "rand_init"}
    batch = int(np.prod(spec.shape[:-2]))
    S = spec.reshape(batch, *spec.shape[-2:]).pow(1 / a["power"])
    ang = torch.view_as_real(angles.reshape(S.shape))
    for n in range(17):
        y = ddsp.griffinlim(spec, window, n_iter=n, angles=angles, **a)
        assert y.dtype == torch.float32 and y.device == spec.device
        exact = g[f"exact_{n}"] if f"exact_{n}" in g else _exact64(spec, window, angles, n_iter=n, **kw).cpu().numpy()
        stock = spectral._stock_loop(S, ang, window, a["n_fft"], a["hop_length"], a["win_length"], n, a["momentum"], a["length"])
        spread = float(np.abs(stock.reshape(y.shape).cpu().numpy() - exact).max())
        if f"spread_{n}" in g:
            spread = max(spread, float(g[f"spread_{n}"]))
        assert y.shape == exact.shape
        err = float(np.abs(y.cpu().numpy() - exact).max())
        assert err <= LOOSE.get((case, n), 4) * spread, (case, n, err, spread)


@pytest.mark.parametrize("n_fft,hop,win_length,lead,frames,power,momentum,extra", [
    (2048, 512, 2048, (3,), 19, 1.0, 0.99, 0),
    (1024, 256, 800, (2, 2), 23, 2.0, 0.9, 100),
    (512, 128, 512, (5,), 31, 1.0, 0.0, 0),
    (256, 32, 256, (2, 3), 40, 1.0, 0.99, 31),
    (128, 32, 128, (1,), 65, 2.0, 0.5, 0),
    (64, 16, 64, (4,), 33, 1.0, 0.99, 0),
])
def test_hip_form_matches_device_stock_loop(n_fft, hop, win_length, lead, frames, power, momentum, extra):
    gen = torch.Generator().manual_seed(n_fft + frames)
    F = n_fft // 2 + 1
    spec = (torch.rand(*lead, F, frames, generator=gen) ** 2).to(DEV)
    angles = torch.polar(torch.ones(*lead, F, frames), 2 * np.pi * torch.rand(*lead, F, frames, generator=gen)).to(DEV)
    window = torch.hann_window(win_length, device=DEV)
    length = hop * (frames - 1) + extra if extra else None
    kw = dict(n_fft=n_fft, hop_length=hop, win_length=win_length, power=power, n_iter=8, momentum=momentum, length=length)
    y = ddsp.griffinlim(spec, window, rand_init=False, angles=angles, **kw)
    # the device's stock loop on the same start (the CUDA branch every other case takes)
    batch = int(np.prod(lead))
    S = spec.reshape(batch, F, frames).pow(1 / power)
    ang = torch.view_as_real(angles.reshape(batch, F, frames)).float()
    stock = spectral._stock_loop(S, ang, window, n_fft, hop, win_length, 8, momentum, length).reshape(y.shape)
    exact = _exact64(spec, window, angles, **kw)
    spread = float((stock.double() - exact).abs().max())
    err = float((y.double() - exact).abs().max())
    assert y.shape == tuple(lead) + (length or hop * (frames - 1),)
    assert err <= 4 * spread, (err, spread)


def test_hip_deterministic():
    gen = torch.Generator().manual_seed(3)
    spec = torch.rand(3, 1025, 60, generator=gen).to(DEV)
    w = torch.hann_window(2048, device=DEV)
    a = ddsp.griffinlim(spec, w, 2048, 256, 2048, 1.0, 12, 0.99, None, True, generator=torch.Generator().manual_seed(1))
    b = ddsp.griffinlim(spec, w, 2048, 256, 2048, 1.0, 12, 0.99, None, True, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, b)
    spec = torch.rand(2, 257, 45, generator=gen).to(DEV)
    w = torch.hann_window(512, device=DEV)
    a = ddsp.griffinlim(spec, w, 512, 64, 512, 2.0, 12, 0.99, None, False)
    assert torch.equal(a, ddsp.griffinlim(spec, w, 512, 64, 512, 2.0, 12, 0.99, None, False))


def _clip(seconds=2.0, sr=44100, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * sr)) / sr
    f0 = 220.0 * (1 + 0.05 * np.sin(2 * np.pi * 0.5 * t))
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(0.5 / h * np.sin(h * phase) for h in range(1, 16)) + 0.05 * rng.standard_normal(t.size)
    return torch.from_numpy(x.astype(np.float32))


def test_convergence_no_worse_than_stock():
    n_fft, hop = 2048, 256
    w = torch.hann_window(n_fft, device=DEV)
    x = _clip().to(DEV)
    L = hop * (x.numel() // hop)
    x = x[:L]
    S = torch.stft(x, n_fft, hop, window=w, center=True, pad_mode='reflect', return_complex=True).abs()

    def sc(y):
        R = torch.stft(y, n_fft, hop, window=w, center=True, pad_mode='reflect', return_complex=True).abs()
        return float(torch.linalg.vector_norm(S - R) / torch.linalg.vector_norm(S))

    angles = torch.polar(torch.ones_like(S), 2 * np.pi * torch.rand(S.shape, generator=torch.Generator().manual_seed(9)).to(DEV))
    kw = dict(n_fft=n_fft, hop_length=hop, win_length=n_fft, power=1.0, momentum=0.99, length=L)
    y0 = ddsp.griffinlim(S, w, n_iter=0, rand_init=False, angles=angles, **kw)
    y = ddsp.griffinlim(S, w, n_iter=200, rand_init=False, angles=angles, **kw)
    stock = spectral._stock_loop(S.unsqueeze(0), torch.view_as_real(angles).unsqueeze(0), w, n_fft, hop, n_fft, 200, 0.99, L)[0]
    sc0, sc_hip, sc_stock = sc(y0), sc(y), sc(stock)
    assert sc_hip <= 1.05 * sc_stock, (sc_hip, sc_stock)
    assert sc_hip <= 0.5 * sc0, (sc_hip, sc0)


@pytest.mark.parametrize("n_fft,hop", [(1000, 250), (4096, 1024)])
def test_unsupported_n_fft_runs_stock_loop_on_device(n_fft, hop):
    assert not spectral.griffinlim_uses_hip(DEV, torch.float32, n_fft, n_fft)
    gen = torch.Generator().manual_seed(n_fft)
    spec = torch.rand(2, n_fft // 2 + 1, 12, generator=gen)
    angles = torch.polar(torch.ones_like(spec), 2 * np.pi * torch.rand(spec.shape, generator=gen))
    w = torch.hann_window(n_fft)
    kw = dict(n_fft=n_fft, hop_length=hop, win_length=n_fft, power=1.0, n_iter=4, momentum=0.99, length=None, rand_init=False)
    y_cpu = ddsp.griffinlim(spec, w, angles=angles, **kw)
    y_dev = ddsp.griffinlim(spec.to(DEV), w.to(DEV), angles=angles.to(DEV), **kw)
    assert y_dev.device == DEV and y_dev.dtype == torch.float32
    exact = _exact64(spec, w, angles, **{k: v for k, v in kw.items() if k != "rand_init"})
    tol = 4 * float((y_cpu.double() - exact).abs().max()) + 1e-6
    assert float((y_dev.cpu().double() - exact).abs().max()) <= tol
    # fp64 on the device is the stock loop too
    y64 = ddsp.griffinlim(spec.double().to(DEV), w.double().to(DEV), angles=angles.to(DEV), **kw)
    assert y64.dtype == torch.float64


def test_style_transfer_end_to_end_on_device(golden):
    """1 s content / 2 s style clips of G28, 256 features, 5 LBFGS iterations, 16 Griffin-Lim iterations on the HIP path.  The
    first two closure losses are within 1e-5 (relative) of the reference's CPU run and the third within 1e-2: MIOpen's
    convolution and rocBLAS's Gram GEMM round differently from the CPU's, and the first LBFGS step (a gradient-sized move of
    lr / |g|_1 with beta = 1e13) carries that into the third evaluation (measured: 8e-8, 0, 4e-3)."""
    g = golden("g28_style")
    sr, win, hop, n_feat, ksize = (int(v) for v in g["params"])
    stats = {}
    torch.manual_seed(28)
    y = ddsp.style_transfer(g["content_audio"], g["style_audio"], sample_rate=sr, win_length=win, hop_length=hop, n_features=n_feat,
                            kernel_size=ksize, max_iter=5, gl_iter=16, device=DEV, generator=torch.Generator().manual_seed(4),
                            stats=stats)
    assert y.shape == (int(g["content_length"]),) and np.isfinite(y).all()
    assert float(np.max(np.abs(y))) == 1.0
    ref = g["lbfgs_losses"]
    got = np.array(stats["losses"][:len(ref)])
    assert got.shape == ref.shape, (got, ref)
    assert np.all(np.abs(got[:2] - ref[:2]) <= 1e-5 * np.abs(ref[:2])) and abs(got[2] - ref[2]) <= 1e-2 * abs(ref[2]), (got, ref)
