"""The noise analysis on the device (csrc/ddsp_noise_analysis.hip) against the fp64 definition of
tests/noise_analysis_reference.py, through the real FilteredNoise, and through AutoEncoder.analyse(noise=True).  TOL_H is derived
in tests/test_noise_analysis_host.py; every test prints its observed figures before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import ddsp_pytorch_amd as ddsp
import noise_analysis_reference as ref
import yin_reference
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

TOL_H = ref.TOL_H


def device(x, hop, F, average, iterations):
    """rows [B, N] (numpy fp32) -> (H, p) from one call on the device."""
    H, p = ddsp.noise_analysis(torch.from_numpy(np.ascontiguousarray(x)).cuda(), hop, F, average=average, iterations=iterations,
                               return_power=True)
    assert H.is_cuda and H.dtype == torch.float32 and H.shape == p.shape == (x.shape[0], x.shape[1] // hop, F)
    return H.cpu().numpy(), p.cpu().numpy()


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape, the definition's answer and the device's: computed once, shared, not modified."""
    B, T, hop, F, average, iterations = shape
    x = ref.gpu_rows(shape)
    want = ref.noise_analysis(x.astype(np.float64), hop, F, average, iterations)
    return x, want, device(x, hop, F, average, iterations)


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_kernel_matches_the_definition(shape):
    B, T, hop, F, average, iterations = shape
    x, (Hr, pr), (H, p) = case(shape)
    eH = (np.abs(H - Hr) / np.maximum(Hr.max(axis=-1, keepdims=True), 1e-300)).max()
    eP = (np.abs(p - pr) / np.maximum(pr.max(axis=-1, keepdims=True), 1e-300)).max()
    print(f"{shape}: max |H - fp64| / max_b H = {eH:.3e}, |p - fp64| / max_b p = {eP:.3e} (TOL_H {TOL_H:g})")
    assert np.isfinite(H).all() and (H >= 0).all() and (p >= 0).all()
    silent = Hr.max(axis=-1) == 0
    if T >= 3 and average == 1:
        assert silent.any()                                       # the inputs hold a silent frame
    assert (H[silent] == 0).all() and (p[silent] == 0).all()
    assert (np.abs(H - Hr) <= TOL_H * Hr.max(axis=-1, keepdims=True)).all()
    assert (np.abs(p - pr) <= TOL_H * pr.max(axis=-1, keepdims=True)).all()
    if iterations == 0:
        assert same_bits(H, np.sqrt(p * np.float32(3.0 / hop)))   # H^0


def test_power_is_optional_and_the_module_is_the_function():
    shape = B, T, hop, F, average, iterations = ref.GPU_SHAPES[1]
    x, _, (H, _) = case(shape)
    xt = torch.from_numpy(x).cuda()
    assert same_bits(ddsp.noise_analysis(xt, hop, F, average=average, iterations=iterations).cpu().numpy(), H)
    module = ddsp.NoiseAnalyzer(type("Conf", (), dict(n_noise_filters=F, hop_length=hop))).cuda()
    assert same_bits(module(xt, average=average, iterations=iterations).cpu().numpy(), H)
    assert ddsp.noise_analysis(torch.zeros((0, 4 * hop), device="cuda"), hop, F).shape == (0, 4, F)
    with pytest.raises(RuntimeError):
        ddsp.noise_analysis(xt.clone().requires_grad_(), hop, F)
    with pytest.raises(ValueError):
        ddsp.noise_analysis(xt, hop, hop // 2 + 2)                # hop < 2 (F - 1)
    with pytest.raises(ValueError):
        ddsp.noise_analysis(xt[:, :-1], hop, F)


@pytest.mark.parametrize("shape", [ref.GPU_SHAPES[0], ref.GPU_SHAPES[5]])
def test_deterministic_and_rows_independent(shape):
    B, T, hop, F, average, iterations = shape
    x, _, first = case(shape)
    again = device(x, hop, F, average, iterations)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    for b in range(B):
        alone = device(x[b:b + 1], hop, F, average, iterations)
        assert all(same_bits(a[0], c[b]) for a, c in zip(alone, first)), b
    flipped = device(x[::-1], hop, F, average, iterations)
    assert all(same_bits(a[::-1], c) for a, c in zip(flipped, first))
    # a row of T - 1 frames in front shifts every frame of row 1 into another slot of the kernel's four-frame tiles
    if average == 1:
        short = np.concatenate([x[:1, hop:], x[1:2, hop:]])
        moved = device(short, hop, F, average, iterations)
        assert all(same_bits(a[1], c[1, 1:]) for a, c in zip(moved, first))


def test_nan_sample_reaches_only_the_frames_whose_window_holds_its_frame():
    shape = B, T, hop, F, average, iterations = ref.GPU_SHAPES[5]
    x, _, (H0, p0) = case(shape)
    s = (average - 1) // 2
    bad = x.copy()
    bad[1, 20 * hop + 3] = np.nan
    H, p = device(bad, hop, F, average, iterations)
    near = np.abs(np.arange(T) - 20) <= s
    assert near.sum() == average
    assert np.isnan(H[1, near]).all() and np.isnan(p[1, near]).all()
    assert same_bits(H[1, ~near], H0[1, ~near]) and same_bits(p[1, ~near], p0[1, ~near])
    assert same_bits(H[[0, 2]], H0[[0, 2]]) and same_bits(p[[0, 2]], p0[[0, 2]])


def test_outside_the_kernel_range_runs_the_torch_path_on_the_device():
    """F = 300 > 257: the same stock-op path as CPU tensors take, on the device.  Both are fp32 evaluations of the definition in
    some order, each within TOL_H of it, so within 2 TOL_H of each other; in fp64 they agree to rounding."""
    shape = B, T, hop, F, average, iterations = (1, 3, 600, 300, 1, 2)
    x = torch.from_numpy(ref.gpu_rows(shape))
    assert not ddsp.analysis._noise_in_kernel_range(x.cuda(), hop, F) and ddsp.analysis._noise_in_kernel_range(x.cuda(), 512, 257)
    cpu = ddsp.noise_analysis(x, hop, F, average=average, iterations=iterations)
    dev = ddsp.noise_analysis(x.cuda(), hop, F, average=average, iterations=iterations)
    assert dev.is_cuda and dev.dtype == torch.float32
    scale = cpu.max(dim=-1, keepdim=True).values
    assert (dev.cpu()[scale[..., 0] == 0] == 0).all() and (scale > 0).any()       # the silent frame
    err = float(((dev.cpu() - cpu).abs() / scale.clamp(min=1e-30)).max())
    cpu64 = ddsp.noise_analysis(x.double(), hop, F, average=average, iterations=iterations)
    dev64 = ddsp.noise_analysis(x.double().cuda(), hop, F, average=average, iterations=iterations)
    err64 = float(((dev64.cpu() - cpu64).abs() / cpu64.max(dim=-1, keepdim=True).values.clamp(min=1e-300)).max())
    print(f"F = 300, device torch path against the CPU path: fp32 {err:.3e} of max_b H (2 TOL_H {2 * TOL_H:g}), fp64 {err64:.3e}")
    assert dev64.dtype == torch.float64
    assert err <= 2 * TOL_H
    assert err64 <= 1e-12


def test_invalid_arguments_come_back_without_a_launch():
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    buf = (ctypes.c_float * 64)()                                 # a valid, 16-byte aligned HOST address: a launch would fault on it
    p = (ctypes.addressof(buf) + 15) & ~15
    call = lambda x, H, ws, B, T, F, hop, average, iterations: L.ddsp_noise_analysis(x, H, None, ws, B, T, F, hop, average,    # noqa: E731
                                                                                        iterations, None)
    assert call(None, p, p, 1, 4, 65, 128, 1, 16) == EINVAL and call(p, None, p, 1, 4, 65, 128, 1, 16) == EINVAL
    assert call(p, p, None, 1, 4, 65, 128, 1, 16) == EINVAL
    for B, T, F, hop, average, iterations in [(-1, 4, 65, 128, 1, 16), (1, 0, 65, 128, 1, 16), (1, 4, 1, 128, 1, 16), (1, 4, 65, 0, 1, 16),
                                              (1, 4, 65, 128, 0, 16), (1, 4, 65, 128, 2, 16), (1, 4, 65, 128, 1, -1)]:
        assert call(p, p, p, B, T, F, hop, average, iterations) == EINVAL, (B, T, F, hop, average, iterations)
    for B, T, F, hop in [(1, 4, 65, 127), (1, 4, 258, 1024), (1, 4, 65, 1025), (1 << 20, 1 << 20, 65, 128)]:
        assert call(p, p, p, B, T, F, hop, 1, 16) == ERANGE, (B, T, F, hop)
        assert L.ddsp_noise_analysis_workspace_bytes(B, T, F, hop) == 0
    assert call(None, None, None, 0, 4, 65, 128, 1, 16) == 0      # an empty batch
    assert L.ddsp_noise_analysis_workspace_bytes(2, 12, 65, 128) >= 4 * (65 * 128 + 64 * 65 + 2 * 12 * 64)
    assert L.ddsp_noise_analysis_workspace_bytes(1, 4, 257, 512) > 0 and L.ddsp_noise_analysis_workspace_bytes(0, 4, 65, 128) == 0


def test_end_to_end_through_the_filtered_noise():
    """FilteredNoise with the in-kernel draw at hop 128, 65 bands, 4096 frames of one constant smooth H; the analysis averaged
    over 4095 frames gives it back.  The cap is host test 4's: the oracle's noise at this frame count is within 0.0135 and 0.0100
    (tests/test_noise_analysis_host.py::test_statistical_recovery)."""
    hop, F, T = 128, 65, 4096
    Hs = ref.smooth_H(F)
    ctrl = {"H": torch.from_numpy(np.tile(Hs.astype(np.float32), (1, T, 1))).cuda()}
    y = ddsp.FilteredNoise(type("Conf", (), dict(hop_length=hop)), rng="device", seed=3).cuda()(ctrl)
    H = ddsp.noise_analysis(y, hop, F, average=4095, iterations=16).double().cpu().numpy()[0]
    centre = H[T // 2 - 8:T // 2 + 8]
    errs = np.linalg.norm(centre - Hs[None], axis=-1) / np.linalg.norm(Hs)
    print(f"FilteredNoise -> noise_analysis: |H - H*| / |H*| over the 16 centre frames: {errs.min():.4f} .. {errs.max():.4f}")
    assert (errs <= 0.05).all()


def test_autoencoder_analyse_with_noise():
    """A tone-plus-noise row and a white-noise row through AutoEncoder(tracker='yin').analyse(noise=True) and back through the
    decoder's synthesis.  The noise branch's rms over the residual's: what the fp64 definition gives on the same residual,
    sqrt(sum_t R(H_t)[0] / sum resid^2), within 0.05: five standard deviations of the rms of one draw of 40 frames x 512 samples
    counted as a quarter as many independent ones (1/2 sqrt(2 / 5120) = 0.0099)."""
    rng = np.random.default_rng(43)
    L = 2048 + 512 * 40
    x = [yin_reference.tone(220.0, L, 44100, rng, top=8000.0) + 0.1 * rng.standard_normal(L), 0.3 * rng.standard_normal(L)]
    x = torch.from_numpy(np.stack(x).astype(np.float32)).cuda()
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    hop, nf = AEConf.hop_length, AEConf.n_noise_filters
    T = L // hop
    average = 5

    z = ae.analyse(x, noise=True, average=average)
    assert sorted(z) == ["H", "a", "c", "f0"]
    assert z["H"].shape == (2, T, nf) and torch.isfinite(z["H"]).all() and (z["H"] >= 0).all()
    torch.manual_seed(5)
    with torch.no_grad():
        y = ae.decoder.synthesize(z)
        noise = ae.decoder.noise(z)
    assert y.shape == (2, T * hop) and torch.isfinite(y).all()

    plain = ae.analyse(x)                                         # without noise: what it returned before, bit for bit
    with torch.no_grad():
        enc = ae.encoder(F_.pad(x, (ae.padding // 2, ae.padding - ae.padding // 2)))
    clip = x[:, :T * hop]
    args = (clip, enc["f0"], hop, AEConf.sample_rate, AEConf.n_harmonics, ae.padding + hop)
    before = ddsp.harmonic_analysis(*args, voiced=enc.get("voiced"))
    assert sorted(plain) == ["a", "c", "f0"] and all(torch.equal(plain[k], before[k]) for k in before)
    assert all(torch.equal(plain[k], z[k]) for k in plain)        # and the harmonic half of the noise dict is the same analysis

    resid = ddsp.harmonic_residual(*args, voiced=enc.get("voiced"))[1].double().cpu().numpy()
    H64, _ = ref.noise_analysis(resid, hop, nf, average, 16)
    assert (np.abs(z["H"].cpu().numpy() - H64) <= TOL_H * H64.max(axis=-1, keepdims=True)).all()
    want = np.sqrt(ref.model_R(H64, hop)[..., 0].sum(axis=-1) / (resid ** 2).sum(axis=-1))
    got = np.sqrt((noise.double().cpu().numpy() ** 2).sum(axis=-1) / (resid ** 2).sum(axis=-1))
    print(f"decoder.noise rms / residual rms: {got}; expected from the fp64 definition: {want}")
    assert (np.abs(got / want - 1.0) <= 0.05).all()
