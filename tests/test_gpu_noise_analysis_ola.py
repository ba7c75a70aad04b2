"""The noise analysis for the overlap-add noise on the device (csrc/ddsp_noise_analysis.hip: ddsp_noise_analysis_ola) against the
fp64 definition of tests/noise_analysis_ola_reference.py, through the real FilteredNoise(overlap_add=True), and through
AutoEncoder.analyse(noise='overlap_add').  TOL_H_OLA and TOL_P_OLA are derived in tests/test_noise_analysis_ola_host.py; every
test prints its observed figures before it asserts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import ddsp_pytorch_amd as ddsp
import noise_analysis_ola_reference as ref
import yin_reference
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

TOL_H, TOL_P = ref.TOL_H_OLA, ref.TOL_P_OLA


def device(x, hop, F, average, iterations):
    """rows [B, N] (numpy fp32) -> (H, p) from one call on the device."""
    H, p = ddsp.noise_analysis(torch.from_numpy(np.array(x, order="C")).cuda(), hop, F, average=average, iterations=iterations,
                               return_power=True, overlap_add=True)
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
    print(f"{shape}: max |H - fp64| / max_b H = {eH:.3e} (TOL_H_OLA {TOL_H:g}), |p - fp64| / max_b p = {eP:.3e} (TOL_P_OLA {TOL_P:g})")
    assert np.isfinite(H).all() and (H >= 0).all() and (p >= 0).all()
    zeroed = ref.zeroed_frames(x, hop)
    if T >= 3:
        assert zeroed.any()                                       # the inputs hold a frame of zeros
    if average == 1:
        assert (H[zeroed] == 0).all() and (p[zeroed] == 0).all()
    silent = Hr.max(axis=-1) == 0
    assert (H[silent] == 0).all() and (p[silent] == 0).all()
    assert (np.abs(H - Hr) <= TOL_H * Hr.max(axis=-1, keepdims=True)).all()
    assert (np.abs(p - pr) <= TOL_P * pr.max(axis=-1, keepdims=True)).all()
    if iterations == 0:
        assert same_bits(H, np.sqrt(p * np.float32(3.0 / hop)))   # H^0


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
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
    # another row in front moves every frame of a row into another slot of the kernel's four-frame tiles: a copy of the row where
    # T is no multiple of 4; otherwise rows without their first frame (T - 1 frames; a frame looks ahead only, so the frames whose
    # averaging window does not hold the dropped one are the same sums)
    b, s = B - 1, (average - 1) // 2
    if T % 4:
        moved = device(np.concatenate([x[:1], x[b:b + 1]]), hop, F, average, iterations)
        assert all(same_bits(a[1], c[b]) for a, c in zip(moved, first))
    else:
        moved = device(np.concatenate([x[:1, hop:], x[b:b + 1, hop:]]), hop, F, average, iterations)
        assert all(same_bits(a[1, s:], c[b, 1 + s:]) for a, c in zip(moved, first))


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_nan_sample_reaches_the_frames_of_step_6_and_nothing_else(shape):
    B, T, hop, F, average, iterations = shape
    x, _, (H0, p0) = case(shape)
    n = (T // 2) * hop + min(3, hop - 1)
    bad = x.copy()
    bad[0, n] = np.nan
    H, p = device(bad, hop, F, average, iterations)
    near = ref.reach(n, T, hop, F, average)
    own = np.arange(T)[(np.arange(T) * hop <= n) & (n < np.arange(T) * hop + hop + F - 2)]
    assert near.sum() == min(T, own[-1] + average // 2 + 1) - max(0, own[0] - average // 2) and near[T // 2]
    assert np.isnan(H[0, near]).all() and np.isnan(p[0, near]).all()
    assert same_bits(H[0, ~near], H0[0, ~near]) and same_bits(p[0, ~near], p0[0, ~near])
    assert same_bits(H[1:], H0[1:]) and same_bits(p[1:], p0[1:])


def test_power_is_optional_and_the_module_is_the_function():
    shape = B, T, hop, F, average, iterations = ref.GPU_SHAPES[1]
    x, _, (H, _) = case(shape)
    xt = torch.from_numpy(x).cuda()
    assert same_bits(ddsp.noise_analysis(xt, hop, F, average=average, iterations=iterations, overlap_add=True).cpu().numpy(), H)
    assert same_bits(ddsp.noise_analysis(xt, hop, F, average=average, overlap_add=True).cpu().numpy(), H)      # 8 is the default
    Conf = type("Conf", (), dict(n_noise_filters=F, hop_length=hop, noise_overlap_add=True))
    assert same_bits(ddsp.NoiseAnalyzer(Conf).cuda()(xt, average=average).cpu().numpy(), H)
    assert ddsp.noise_analysis(torch.zeros((0, 4 * hop), device="cuda"), hop, F, overlap_add=True).shape == (0, 4, F)
    with pytest.raises(RuntimeError):
        ddsp.noise_analysis(xt.clone().requires_grad_(), hop, F, overlap_add=True)
    with pytest.raises(ValueError):
        ddsp.noise_analysis(xt[:, :-1], hop, F, overlap_add=True)


def test_outside_the_kernel_range_runs_the_torch_path_on_the_device():
    """F = 300 > 257: the same stock-op path as CPU tensors take, on the device.  Both are fp32 evaluations of the definition in
    some order, each within TOL_H_OLA of it, so within 2 TOL_H_OLA of each other; in fp64 they agree to rounding."""
    shape = B, T, hop, F, average, iterations = (1, 3, 600, 300, 1, 2)
    x = torch.from_numpy(ref.gpu_rows(shape))
    assert not ddsp.analysis._noise_ola_in_kernel_range(x.cuda(), hop, F) and ddsp.analysis._noise_ola_in_kernel_range(x.cuda(), 2, 257)
    kw = dict(average=average, iterations=iterations, overlap_add=True)
    cpu = ddsp.noise_analysis(x, hop, F, **kw)
    dev = ddsp.noise_analysis(x.cuda(), hop, F, **kw)
    assert dev.is_cuda and dev.dtype == torch.float32
    scale = cpu.max(dim=-1, keepdim=True).values
    assert (dev.cpu()[scale[..., 0] == 0] == 0).all() and (scale > 0).any()       # the frame of zeros
    err = float(((dev.cpu() - cpu).abs() / scale.clamp(min=1e-30)).max())
    cpu64 = ddsp.noise_analysis(x.double(), hop, F, **kw)
    dev64 = ddsp.noise_analysis(x.double().cuda(), hop, F, **kw)
    err64 = float(((dev64.cpu() - cpu64).abs() / cpu64.max(dim=-1, keepdim=True).values.clamp(min=1e-300)).max())
    print(f"F = 300, device torch path against the CPU path: fp32 {err:.3e} of max_b H (2 TOL_H_OLA {2 * TOL_H:g}), fp64 {err64:.3e}")
    assert dev64.dtype == torch.float64
    assert err <= 2 * TOL_H
    assert err64 <= 1e-12


@pytest.mark.parametrize("hop", [128, 32])
def test_end_to_end_through_the_filtered_noise(hop):
    """FilteredNoise(overlap_add=True) with the in-kernel draw, 65 bands, 4096 frames of one constant smooth H, at hop 128 and at
    hop 32 (below 2 (F - 1) = 128, where the truncated model has no answer); the analysis averaged over 4095 frames gives it
    back.  The cap is the host test's: the fp64 synthesiser's noise at this frame count is within 0.0090 and 0.0220
    (tests/test_noise_analysis_ola_host.py::test_the_model_is_the_synthesisers_noise)."""
    F, T = 65, 4096
    Hs = ref.smooth_H(F)
    ctrl = {"H": torch.from_numpy(np.tile(Hs.astype(np.float32), (1, T, 1))).cuda()}
    y = ddsp.FilteredNoise(type("Conf", (), dict(hop_length=hop)), rng="device", seed=3, overlap_add=True).cuda()(ctrl)
    H = ddsp.noise_analysis(y, hop, F, average=4095, overlap_add=True).double().cpu().numpy()[0]
    centre = H[T // 2 - 8:T // 2 + 8]
    errs = np.linalg.norm(centre - Hs[None], axis=-1) / np.linalg.norm(Hs)
    print(f"hop {hop}: FilteredNoise(overlap_add) -> noise_analysis: |H - H*| / |H*| over the 16 centre frames: {errs.min():.4f} .. {errs.max():.4f}")
    assert (errs <= 0.05).all()


def test_autoencoder_analyse_with_the_overlap_add_noise():
    """Section 15's tone-plus-noise row and white-noise row through AutoEncoder(tracker='yin', noise_overlap_add=True)
    .analyse(noise='overlap_add') and back through the decoder's synthesis.  The noise branch's rms over the residual's: what the
    fp64 definition gives on the same residual, sqrt(sum_t R_ola(H_t)[0] / sum resid^2), within 0.05: five standard deviations
    of the rms of one draw of 40 frames x 512 samples counted as a quarter as many independent ones (1/2 sqrt(2 / 5120) =
    0.0099)."""
    rng = np.random.default_rng(43)
    L = 2048 + 512 * 40
    x = [yin_reference.tone(220.0, L, 44100, rng, top=8000.0) + 0.1 * rng.standard_normal(L), 0.3 * rng.standard_normal(L)]
    x = torch.from_numpy(np.stack(x).astype(np.float32)).cuda()
    ae = ddsp.AutoEncoder(AEConf, tracker='yin', noise_overlap_add=True).cuda().eval()
    hop, nf = AEConf.hop_length, AEConf.n_noise_filters
    T = L // hop
    average = 5

    z = ae.analyse(x, noise='overlap_add', average=average)
    assert sorted(z) == ["H", "a", "c", "f0"]
    assert z["H"].shape == (2, T, nf) and torch.isfinite(z["H"]).all() and (z["H"] >= 0).all()
    torch.manual_seed(5)
    with torch.no_grad():
        y = ae.decoder.synthesize(z)
        noise = ae.decoder.noise(z)
    assert y.shape == (2, T * hop) and torch.isfinite(y).all()

    plain = ae.analyse(x)
    assert all(torch.equal(plain[k], z[k]) for k in plain)        # the harmonic half of the noise dict is the plain analysis
    with torch.no_grad():
        enc = ae.encoder(F_.pad(x, (ae.padding // 2, ae.padding - ae.padding // 2)))
    args = (x[:, :T * hop], enc["f0"], hop, AEConf.sample_rate, AEConf.n_harmonics, ae.padding + hop)
    resid = ddsp.harmonic_residual(*args, voiced=enc.get("voiced"))[1].double().cpu().numpy()
    H64, _ = ref.noise_analysis(resid, hop, nf, average, 8)
    eH = (np.abs(z["H"].cpu().numpy() - H64) / H64.max(axis=-1, keepdims=True)).max()
    want = np.sqrt(ref.model_R(H64, hop)[..., 0].sum(axis=-1) / (resid ** 2).sum(axis=-1))
    got = np.sqrt((noise.double().cpu().numpy() ** 2).sum(axis=-1) / (resid ** 2).sum(axis=-1))
    print(f"|H - fp64| / max_b H = {eH:.3e}; decoder.noise rms / residual rms: {got}; expected from the fp64 definition: {want}")
    assert (np.abs(z["H"].cpu().numpy() - H64) <= TOL_H * H64.max(axis=-1, keepdims=True)).all()
    assert (np.abs(got / want - 1.0) <= 0.05).all()

    with pytest.raises(ValueError, match="truncated.*overlap_add"):          # each spelling is refused on the other decoder
        ae.analyse(x, noise=True)
    with pytest.raises(ValueError, match="truncated.*overlap_add"):
        ae.analyse(x, noise='truncated')
    with pytest.raises(ValueError, match="overlap-add"):
        ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval().analyse(x, noise='overlap_add')
    with pytest.raises(ValueError):
        ae.analyse(x, noise='ola')
