"""The definition of the noise analysis (tests/noise_analysis_reference.py) against the oracle's filtered
noise, in fp64 on the host: the impulse-response map is the reference's, the truncated model is what its frames have, the fixed
point inverts the model, and the package's torch-op path is the definition.  test_device_bound derives TOL_H.  Every test prints
its figures before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import noise_analysis_reference as ref
from oracle import torch_restatement as oracle

FRAMES = 4096


@functools.lru_cache(maxsize=None)
def oracle_statistics(F, hop, seed):
    """(H*, the mean over 4096 oracle frames of the measured r, R(H*)): computed once, shared, not modified."""
    Hs = ref.smooth_H(F)
    x, _ = ref.oracle_noise(np.tile(Hs, (FRAMES, 1)), hop, seed)
    return Hs, ref.measure(x, hop, F).mean(axis=0), ref.model_R(Hs, hop)


@pytest.mark.parametrize("F,hop", [(33, 100), (65, 128), (195, 512), (257, 512)])
def test_amat_is_the_references_filter(F, hop):
    want = oracle.impulse_response(torch.eye(F, dtype=torch.float64), hop).numpy().T        # column b: the response of unit vector b
    got = ref.amat(F, hop)
    err = np.abs(got - want).max() / np.abs(want).max()
    d, _ = ref.support(F, hop)
    rows = np.zeros_like(got)
    rows[d] = ref.amat_rows(F, hop)
    closed = np.abs(rows - want).max() / np.abs(want).max()
    print(f"F {F}, hop {hop}: |Amat - oracle| / max = {err:.2e}; closed form of the M stored rows, zeros elsewhere: {closed:.2e}")
    assert err <= 1e-14
    assert closed <= 1e-14


@pytest.mark.parametrize("F,hop,seed", [(65, 128, 1), (65, 128, 2), (33, 100, 1)])
def test_the_model_is_the_references_noise(F, hop, seed):
    Hs, r, R = oracle_statistics(F, hop, seed)
    err = ref.rel(r, R)
    plain = ref.rel(r, ref.model_R(Hs, hop, truncated=False))
    print(f"F {F}, hop {hop}, seed {seed}: |mean r - R(H)| / |R(H)| = {err:.4f}; without the truncation weights {plain:.4f}")
    assert err <= 0.03
    assert plain > 0.03                                           # the weights (hop - l - d) are what makes the model fit


@pytest.mark.parametrize("F,hop", [(65, 128), (195, 512)])
def test_the_fixed_point_inverts_the_model(F, hop):
    Hs = ref.smooth_H(F)
    R = ref.model_R(Hs, hop)
    e8 = ref.rel(ref.fixed_point(R, hop, F, 8)[0], Hs)
    e30 = ref.rel(ref.fixed_point(R, hop, F, 30)[0], Hs)
    print(f"F {F}, hop {hop}: exact statistics, |H - H*| / |H*| after 8 iterations {e8:.2e}, after 30 {e30:.2e}")
    assert e30 <= 2e-3
    assert e30 < e8


@pytest.mark.parametrize("F,hop,seed", [(65, 128, 1), (65, 128, 2)])
def test_statistical_recovery(F, hop, seed):
    """4096 oracle frames, average >= 2 T - 1 (every frame's window is the whole row, so rbar is the mean over all frames:
    test_edges checks that equivalence on a short row), 16 iterations."""
    Hs, r, R = oracle_statistics(F, hop, seed)
    H, _ = ref.fixed_point(r, hop, F, 16)
    eH = ref.rel(H, Hs)
    eP = ref.rel(ref.P(ref.model_R(H, hop), F), ref.P(R, F))
    print(f"F {F}, hop {hop}, seed {seed}: |H - H*| / |H*| = {eH:.4f}, |P(R(H)) - P(R(H*))| / |P(R(H*))| = {eP:.4f}")
    assert eH <= 0.05
    assert eP <= 0.03


def test_edges():
    F, hop, T = 17, 40, 9
    x, _ = ref.oracle_noise(ref.smooth_H(F, T, seed=5), hop, seed=9)
    x[3 * hop:4 * hop] = 0.0
    xt = torch.from_numpy(x)[None]

    # hop 31 < 2 (F - 1) = 32 (on 9 whole frames of 31), an even average, none, a negative iteration count
    for n, h, average, iterations in [(T * 31, 31, 1, 4), (T * hop, hop, 2, 4), (T * hop, hop, 0, 4), (T * hop, hop, 1, -1)]:
        with pytest.raises(ValueError):
            ref.noise_analysis(x[:n], h, F, average, iterations)
        with pytest.raises(ValueError):
            ddsp.noise_analysis(xt[:, :n], h, F, average=average, iterations=iterations)
    with pytest.raises(ValueError):
        ddsp.noise_analysis(xt[:, :-1], hop, F)                   # no whole number of frames
    with pytest.raises(RuntimeError):
        ddsp.noise_analysis(xt.clone().requires_grad_(), hop, F)

    H, p = ref.noise_analysis(x, hop, F, 1, 8)
    assert (H[3] == 0).all() and (p[3] == 0).all() and (H >= 0).all() and np.isfinite(H).all()     # silence gives zeros
    assert (np.delete(H, 3, axis=0).max(axis=-1) > 0).all()

    H0, p0 = ref.noise_analysis(x, hop, F, 3, 0)                  # iterations = 0 returns H^0
    assert np.array_equal(H0, np.sqrt(3.0 * p0 / hop))

    whole = ref.fixed_point(ref.measure(x, hop, F).mean(axis=0), hop, F, 4)[0]                      # average beyond T is clipped
    for average in (2 * T - 1, 2 * T + 1, 1001):
        assert np.abs(ref.noise_analysis(x, hop, F, average, 4)[0] - whole[None]).max() <= 1e-13 * whole.max(), average

    for average in (1, 3, 5):                                     # a NaN changes exactly the frames within s of its own
        s = (average - 1) // 2
        clean = ref.noise_analysis(x, hop, F, average, 4)[0]
        bad = x.copy()
        bad[5 * hop + 7] = np.nan
        got = ref.noise_analysis(bad, hop, F, average, 4)[0]
        near = np.abs(np.arange(T) - 5) <= s
        assert np.isnan(got[near]).all() and np.array_equal(got[~near], clean[~near]), average
        pkg = ddsp.noise_analysis(torch.from_numpy(bad)[None], hop, F, average=average, iterations=4)[0].numpy()
        assert np.isnan(pkg[near]).all() and np.abs(pkg[~near] - clean[~near]).max() <= 1e-12, average


@pytest.mark.parametrize("shape", [(2, 7, 40, 17, 3, 6), (1, 4, 128, 65, 1, 3), (1, 3, 100, 33, 9, 0)])
def test_the_cpu_torch_path_is_the_definition(shape):
    B, T, hop, F, average, iterations = shape
    x = ref.gpu_rows(shape).astype(np.float64)
    H, p = ref.noise_analysis(x, hop, F, average, iterations)
    Ht, pt = ddsp.noise_analysis(torch.from_numpy(x), hop, F, average=average, iterations=iterations, return_power=True)
    assert Ht.dtype == torch.float64 and Ht.shape == (B, T, F) and pt.shape == (B, T, F)
    eH, eP = np.abs(Ht.numpy() - H).max() / H.max(), np.abs(pt.numpy() - p).max() / p.max()
    print(f"{shape}: CPU torch-op path against numpy, fp64: H {eH:.2e}, p {eP:.2e}")
    assert eH <= 1e-12 and eP <= 1e-12
    module = ddsp.NoiseAnalyzer(type("Conf", (), dict(n_noise_filters=F, hop_length=hop)))
    assert not list(module.parameters())
    assert torch.equal(module(torch.from_numpy(x), average=average, iterations=iterations), Ht)
    H32 = ddsp.noise_analysis(torch.from_numpy(x).float(), hop, F, average=average, iterations=iterations)
    assert H32.dtype == torch.float32 and np.abs(H32.numpy() - H).max() <= 1e-4 * H.max()


def test_the_c_entry_validates_before_the_device():
    """No GPU here: every one of these returns before a launch (the pointer is a host address nothing reads)."""
    L = ddsp._lib.lib()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    assert L.ddsp_noise_analysis(None, p, None, p, 1, 4, 65, 128, 1, 16, None) == -1
    assert L.ddsp_noise_analysis(p, p, None, p, 1, 4, 65, 128, 2, 16, None) == -1                  # an even average
    assert L.ddsp_noise_analysis(p, p, None, p, 1, 4, 65, 127, 1, 16, None) == -2                  # hop < 2 (F - 1)
    assert L.ddsp_noise_analysis(p, p, None, p, 1, 4, 258, 1024, 1, 16, None) == -2
    assert L.ddsp_noise_analysis(None, None, None, None, 0, 4, 65, 128, 1, 16, None) == 0
    assert L.ddsp_noise_analysis_workspace_bytes(1, 4, 65, 127) == 0 and L.ddsp_noise_analysis_workspace_bytes(16, 172, 195, 512) > 0


def test_device_bound():
    """TOL_H, as DESIGN section 14 derives TOL_C: the definition evaluated in the kernels' arithmetic (fp32 tables, every sum an
    fp32 FMA chain in the kernels' order) on the device tests' own inputs, its largest deviation from fp64 relative to each
    frame's max_b H, times two because any other summation order is as valid."""
    worst = worst_p = 0.0
    for shape in ref.GPU_SHAPES:
        B, T, hop, F, average, iterations = shape
        x = ref.gpu_rows(shape)
        H, p = ref.noise_analysis(x.astype(np.float64), hop, F, average, iterations)
        He, pe = ref.analyse_fp32(x, hop, F, average, iterations)
        eH = (np.abs(He - H) / np.maximum(H.max(axis=-1, keepdims=True), 1e-300)).max()
        eP = (np.abs(pe - p) / np.maximum(p.max(axis=-1, keepdims=True), 1e-300)).max()
        print(f"{shape}: fp32 emulation against fp64: H {eH:.3e} of max_b H, p {eP:.3e} of max_b p")
        assert (He[H.max(axis=-1) == 0] == 0).all()              # a silent frame is 0 in fp32 as well
        worst, worst_p = max(worst, eH), max(worst_p, eP)
    print(f"largest: H {worst:.3e}, p {worst_p:.3e}; TOL_H = {ref.TOL_H:g}")
    assert worst <= ref.TOL_H / 2 and worst_p <= ref.TOL_H / 2
    assert ref.TOL_H <= 3 * worst                                 # the bound stays the derived one
