"""The definition of the noise analysis for the overlap-add noise (tests/noise_analysis_ola_reference.py)
in fp64 on the host: the model is what the overlap-add synthesiser's noise has, the fixed point inverts the model, and the
package's torch-op path is the definition.  test_device_bound derives TOL_H_OLA.  Every test prints its figures before it
asserts."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import noise_analysis_ola_reference as ref
import noise_analysis_reference as nar

FRAMES = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def synthesiser_statistics(F, hop, seed):
    """(H*, the mean over the row of the r measured on 4096 frames of fp64 overlap-add noise of H*, R_ola(H*)): computed once."""
    Hs = ref.smooth_H(F)
    x = ref.ola_noise(np.tile(Hs, (FRAMES, 1)), hop, seed)
    return Hs, ref.measure(x, hop, F).mean(axis=0), ref.model_R(Hs, hop)


@pytest.mark.parametrize("F,hop,seed", [(65, 128, 1), (65, 128, 2), (65, 32, 1), (65, 32, 2), (33, 100, 1), (33, 100, 2)])
def test_the_model_is_the_synthesisers_noise(F, hop, seed):
    """hop 32 with 65 bands lies below M = 128, where the truncated model is not identifiable."""
    Hs, r, R = synthesiser_statistics(F, hop, seed)
    eR = ref.rel(r, R)
    eH = ref.rel(ref.fixed_point(r, hop, F, 8)[0], Hs)
    print(f"F {F}, hop {hop}, seed {seed}: |mean r - R_ola(H*)| / |R_ola(H*)| = {eR:.4f}; |H - H*| / |H*| after 8 iterations = {eH:.4f}")
    assert eR <= 0.05
    assert eH <= 0.05


@pytest.mark.parametrize("F,hop", [(65, 128), (65, 32), (33, 100), (195, 512)])
def test_the_fixed_point_inverts_the_model(F, hop):
    Hs = ref.smooth_H(F)
    R = ref.model_R(Hs, hop)
    e0 = ref.rel(ref.fixed_point(R, hop, F, 0)[0], Hs)
    e8 = ref.rel(ref.fixed_point(R, hop, F, 8)[0], Hs)
    print(f"F {F}, hop {hop}: exact statistics, |H - H*| / |H*| of H0 {e0:.2e}, after 8 iterations {e8:.2e}")
    assert e8 <= 2e-3
    if (F, hop) in [(65, 128), (33, 100)]:
        assert e0 > 1e-2                                          # what the fixed point is for: the closed-form start alone is not enough


def test_the_model_has_no_truncation_weights_and_hop_is_a_scale():
    Hs = ref.smooth_H(33)
    h = ref.olar.responses(Hs)
    full = np.correlate(h, h, mode="full")[len(h) - 1:][:32]      # sum_e h[e] h[e + l], l >= 0
    assert np.abs(ref.rho(Hs) - full).max() <= 1e-15 * full.max()
    assert np.array_equal(ref.model_R(Hs, 64) * 2, ref.model_R(Hs, 128))
    assert np.array_equal(ref.model_R(np.stack([Hs, 2 * Hs]), 100)[1], 4 * ref.model_R(Hs, 100))


def test_the_last_frames_normalisation_and_zero_counts():
    """T = 1 with hop < L: lag l has hop - l products, scaled to hop of them; the lags from hop on have none and are 0."""
    F, hop = 17, 5
    x = np.random.default_rng(3).standard_normal(hop)
    r = ref.measure(x, hop, F)[0]
    for lag in range(F - 1):
        want = hop / (hop - lag) * (x[:hop - lag] * x[lag:]).sum() if lag < hop else 0.0
        assert abs(r[lag] - want) <= 1e-15 * np.abs(x).max() ** 2 * hop, lag
    assert (r[hop:] == 0).all() and (ref.counts(1, hop, F - 1)[0] == np.maximum(hop - np.arange(F - 1), 0)).all()
    # inside a long row every count is hop and a lag reaches several frames ahead
    T = 9
    x = np.random.default_rng(4).standard_normal(T * hop)
    r = ref.measure(x, hop, F)
    assert (ref.counts(T, hop, F - 1)[:T - 4] == hop).all()
    assert abs(r[2, 13] - (x[2 * hop:3 * hop] * x[2 * hop + 13:3 * hop + 13]).sum()) <= 1e-14
    # the expectation is the model's whatever the count: white noise of variance 1 has r[0] = hop in the mean, at the end too
    w = np.random.default_rng(5).standard_normal((4000, 3 * hop))
    m = ref.measure(w, hop, 4).mean(axis=0)
    assert np.abs(m[:, 0] - hop).max() <= 0.05 * hop and np.abs(m[:, 1:]).max() <= 0.05 * hop * 2


def test_edges():
    F, hop, T = 17, 12, 9                                         # hop < L = 16: a lag reaches two frames ahead
    x = ref.ola_noise(ref.smooth_H(F, T, seed=5), hop, seed=9)
    x[3 * hop:4 * hop] = 0.0
    xt = torch.from_numpy(x)[None]

    for n, h, average, iterations in [(T * hop, hop, 2, 4), (T * hop, hop, 0, 4), (T * hop, hop, 1, -1), (T * hop - 1, hop, 1, 4)]:
        with pytest.raises(ValueError):
            ref.noise_analysis(x[:n], h, F, average, iterations)
        with pytest.raises(ValueError):
            ddsp.noise_analysis(xt[:, :n], h, F, average=average, iterations=iterations, overlap_add=True)
    with pytest.raises(ValueError):
        ddsp.noise_analysis(xt, hop, 1, overlap_add=True)
    with pytest.raises(ValueError):
        ddsp.noise_analysis(xt, hop, F)                           # hop < 2 (F - 1): still refused by the truncated model
    with pytest.raises(RuntimeError):
        ddsp.noise_analysis(xt.clone().requires_grad_(), hop, F, overlap_add=True)

    H, p = ref.noise_analysis(x, hop, F, 1, 8)
    assert (H[3] == 0).all() and (p[3] == 0).all() and (H >= 0).all() and np.isfinite(H).all()     # a frame of zeros gives zeros
    assert (np.delete(H, 3, axis=0).max(axis=-1) > 0).all()

    H0, p0 = ref.noise_analysis(x, hop, F, 3, 0)                  # iterations = 0 returns H^0
    assert np.array_equal(H0, np.sqrt(3.0 * p0 / hop))
    assert np.array_equal(ref.noise_analysis(x, hop, F, 3)[0], ref.noise_analysis(x, hop, F, 3, 8)[0])     # the default is 8

    whole = ref.fixed_point(ref.measure(x, hop, F).mean(axis=0), hop, F, 4)[0]                      # average beyond T is clipped
    for average in (2 * T - 1, 2 * T + 1, 1001):
        assert np.abs(ref.noise_analysis(x, hop, F, average, 4)[0] - whole[None]).max() <= 1e-13 * whole.max(), average

    for average in (1, 3, 5):                                     # a NaN reaches the frames of step 6 and no other
        clean = ref.noise_analysis(x, hop, F, average, 4)[0]
        for n in (5 * hop + 7, 5 * hop, T * hop - 1, 0):
            bad = x.copy()
            bad[n] = np.nan
            got = ref.noise_analysis(bad, hop, F, average, 4)[0]
            near = ref.reach(n, T, hop, F, average)
            own = [t for t in range(T) if t * hop <= n < t * hop + hop + F - 2]
            assert near.sum() == len(range(max(0, own[0] - average // 2), min(T, own[-1] + average // 2 + 1)))
            assert np.isnan(got[near]).all() and np.array_equal(got[~near], clean[~near]), (average, n)
            pkg = ddsp.noise_analysis(torch.from_numpy(bad)[None], hop, F, average=average, iterations=4, overlap_add=True)[0].numpy()
            assert np.isnan(pkg[near]).all() and np.abs(pkg[~near] - clean[~near]).max() <= 1e-12, (average, n)
    assert ref.reach(5 * hop + 7, T, hop, F).tolist() == [t in (4, 5) for t in range(T)]       # 67 < 4 hop + hop + L - 1 = 75
    assert ref.reach(5 * hop, T, hop, F).tolist() == [t in (3, 4, 5) for t in range(T)]        # 60 < 3 hop + hop + L - 1 = 63


@pytest.mark.parametrize("shape", [(2, 7, 40, 17, 3, 6), (1, 4, 16, 33, 1, 3), (1, 1, 5, 9, 1, 2), (1, 3, 100, 33, 9, 0)])
def test_the_cpu_torch_path_is_the_definition(shape):
    B, T, hop, F, average, iterations = shape
    x = ref.gpu_rows(shape).astype(np.float64)
    H, p = ref.noise_analysis(x, hop, F, average, iterations)
    Ht, pt = ddsp.noise_analysis(torch.from_numpy(x), hop, F, average=average, iterations=iterations, return_power=True,
                                 overlap_add=True)
    assert Ht.dtype == torch.float64 and Ht.shape == (B, T, F) and pt.shape == (B, T, F)
    eH, eP = np.abs(Ht.numpy() - H).max() / H.max(), np.abs(pt.numpy() - p).max() / p.max()
    print(f"{shape}: CPU torch-op path against numpy, fp64: H {eH:.2e}, p {eP:.2e}")
    assert eH <= 1e-13 and eP <= 1e-13
    Conf = type("Conf", (), dict(n_noise_filters=F, hop_length=hop))
    module = ddsp.NoiseAnalyzer(Conf, overlap_add=True)
    assert not list(module.parameters()) and module.overlap_add
    assert torch.equal(module(torch.from_numpy(x), average=average, iterations=iterations), Ht)
    H32 = ddsp.noise_analysis(torch.from_numpy(x).float(), hop, F, average=average, iterations=iterations, overlap_add=True)
    assert H32.dtype == torch.float32 and np.abs(H32.numpy() - H).max() <= 1e-4 * H.max()
    assert ddsp.noise_analysis(torch.zeros((0, 3 * hop)), hop, F, overlap_add=True).shape == (0, 3, F)


def test_the_flag_and_the_default_iterations():
    F, hop = 9, 16
    x = torch.from_numpy(ref.gpu_rows((1, 6, hop, F, 1, 8)))
    Conf = type("Conf", (), dict(n_noise_filters=F, hop_length=hop))
    OlaConf = type("OlaConf", (Conf,), dict(noise_overlap_add=True))
    assert not ddsp.NoiseAnalyzer(Conf).overlap_add and ddsp.NoiseAnalyzer(OlaConf).overlap_add      # None reads the configuration
    assert not ddsp.NoiseAnalyzer(OlaConf, overlap_add=False).overlap_add and ddsp.NoiseAnalyzer(Conf, overlap_add=True).overlap_add
    ola = ddsp.noise_analysis(x, hop, F, overlap_add=True)
    assert torch.equal(ola, ddsp.noise_analysis(x, hop, F, iterations=8, overlap_add=True))
    assert not torch.equal(ola, ddsp.noise_analysis(x, hop, F, iterations=16, overlap_add=True))
    assert torch.equal(ddsp.NoiseAnalyzer(OlaConf)(x), ola)
    trunc = ddsp.noise_analysis(x, hop, F)                        # the truncated model keeps its default of 16
    assert torch.equal(trunc, ddsp.noise_analysis(x, hop, F, iterations=16)) and torch.equal(ddsp.NoiseAnalyzer(Conf)(x), trunc)
    assert not torch.equal(trunc, ola)


def test_the_abi_declares_and_exports_the_entry_points():
    names = ("ddsp_noise_analysis_ola_workspace_bytes", "ddsp_noise_analysis_ola")
    with open(os.path.join(ROOT, "include", "ddsp_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+DDSP_HIP_ABI_VERSION\s+5\b", header) and ddsp._lib.ABI_VERSION == 5
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5
    for name in names:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name)
    assert ddsp._lib.SIGNATURES[names[0]] == ddsp._lib.SIGNATURES["ddsp_noise_analysis_workspace_bytes"]       # the truncated pair's lists
    assert ddsp._lib.SIGNATURES[names[1]] == ddsp._lib.SIGNATURES["ddsp_noise_analysis"]


def test_the_c_entry_validates_before_the_device():
    """No GPU here: every one of these returns before a launch (the pointer is a host address nothing reads)."""
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    call = lambda x, H, ws, B, T, F, hop, average, iterations: L.ddsp_noise_analysis_ola(x, H, None, ws, B, T, F, hop, average,    # noqa: E731
                                                                                            iterations, None)
    assert call(None, p, p, 1, 4, 65, 128, 1, 8) == EINVAL and call(p, None, p, 1, 4, 65, 128, 1, 8) == EINVAL
    assert call(p, p, None, 1, 4, 65, 128, 1, 8) == EINVAL and call(p, p, p + 4, 1, 4, 65, 128, 1, 8) == EINVAL
    for B, T, F, hop, average, iterations in [(-1, 4, 65, 128, 1, 8), (1, 0, 65, 128, 1, 8), (1, 4, 1, 128, 1, 8), (1, 4, 65, 0, 1, 8),
                                              (1, 4, 65, 128, 0, 8), (1, 4, 65, 128, 2, 8), (1, 4, 65, 128, 1, -1)]:
        assert call(p, p, p, B, T, F, hop, average, iterations) == EINVAL, (B, T, F, hop, average, iterations)
    for B, T, F, hop in [(1, 4, 258, 1024), (1, 4, 65, 1025), (1 << 20, 1 << 20, 65, 128), (1, (2 ** 31 - 8192) // 1024, 65, 1024),
                         (1, 2 ** 31 - 8192, 65, 1), (2 ** 31, 1, 65, 1)]:
        assert call(p, p, p, B, T, F, hop, 1, 8) == ERANGE, (B, T, F, hop)
        assert L.ddsp_noise_analysis_ola_workspace_bytes(B, T, F, hop) == 0
    assert call(None, None, None, 0, 4, 65, 128, 1, 8) == 0       # an empty batch
    assert L.ddsp_noise_analysis_ola_workspace_bytes(2, 12, 65, 128) >= 4 * (2 * 65 * 64 + 2 * 12 * 64)
    assert L.ddsp_noise_analysis_ola_workspace_bytes(1, 4, 65, 32) > 0          # below 2 (F - 1): analysable here
    assert L.ddsp_noise_analysis_ola_workspace_bytes(1, 3, 257, 1024) > 0 and L.ddsp_noise_analysis_ola_workspace_bytes(1, 40, 2, 1) > 0
    assert L.ddsp_noise_analysis_ola_workspace_bytes(0, 4, 65, 128) == 0
    assert L.ddsp_noise_analysis_ola_workspace_bytes(1, (2 ** 31 - 8192) // 1024 - 1, 65, 1024) > 0


def test_device_bound():
    """TOL_H_OLA, by section 15's rule: the definition evaluated in the kernels' arithmetic (fp32 tables, every sum an fp32 FMA
    chain in the kernels' order) on the device tests' own inputs, its largest deviation from fp64 relative to each frame's
    max_b H (TOL_P_OLA: of p relative to max_b p), times two because any other summation order is as valid, rounded up to one
    digit."""
    worst = worst_p = 0.0
    for shape in ref.GPU_SHAPES:
        B, T, hop, F, average, iterations = shape
        x = ref.gpu_rows(shape)
        H, p = ref.noise_analysis(x.astype(np.float64), hop, F, average, iterations)
        He, pe = ref.analyse_ola_fp32(x, hop, F, average, iterations)
        eH = (np.abs(He - H) / np.maximum(H.max(axis=-1, keepdims=True), 1e-300)).max()
        eP = (np.abs(pe - p) / np.maximum(p.max(axis=-1, keepdims=True), 1e-300)).max()
        print(f"{shape}: fp32 emulation against fp64: H {eH:.3e} of max_b H, p {eP:.3e} of max_b p")
        assert (He[H.max(axis=-1) == 0] == 0).all()              # a frame of zeros is 0 in fp32 as well
        worst, worst_p = max(worst, eH), max(worst_p, eP)
    print(f"largest: H {worst:.3e}, p {worst_p:.3e}; TOL_H_OLA = {ref.TOL_H_OLA:g}, TOL_P_OLA = {ref.TOL_P_OLA:g}")
    assert worst <= ref.TOL_H_OLA / 2 and worst_p <= ref.TOL_P_OLA / 2
    assert ref.TOL_H_OLA <= 3 * worst and ref.TOL_P_OLA <= 3 * worst_p      # the bounds stay the derived ones
    assert nar.TOL_H == 3e-6                                      # (the truncated model's bound is its own)
