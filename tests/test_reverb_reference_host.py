"""The fp64 reference and the bounds of tests/reverb_reference.py checked on their own: against the fixtures captured from the
reference project, against torch's double-precision autograd of the module's torch formulation, and by measuring the fp32
restatements over exactly the cases tests/test_gpu_reverb_stages.py runs (the figures that size K), with a self-check that one
dropped tap stands more than 100 times above every bound.  All without a device (nothing here launches a kernel)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd.reverb import fft_length

import reverb_reference as R

f32 = np.float32


class Conf:
    def __init__(self, sample_rate):
        self.n_harmonics, self.sample_rate, self.hop_length = 1, sample_rate, 64


def _t(sr):
    return np.arange(sr, dtype=f32) / f32(sr)


def _close(got, ref, tol):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) <= tol * max(1.0, float(np.max(np.abs(ref))))


# ---- the reference against the fixtures from the reference project (tolerances: those of tests/test_reverb.py on the CPU) ----
@pytest.mark.parametrize("clip", [4096, 1024])
def test_reference_equals_g9_clips(clip):
    g = load_golden(f"g9_reverb_clip{clip}")
    sr = int(g["sample_rate"])
    imp, _ = R.impulse(g["noise"], g["decay"], g["wet"], _t(sr), sr)
    assert np.max(np.abs(imp - g["impulse"][0])) <= 1e-6
    used = min(sr, clip)
    y, _ = R.forward(g["x"], R.impulse(g["noise"], g["decay"], g["wet"], _t(sr), used)[0])
    assert _close(y, g["y"], 2e-6)


@pytest.mark.parametrize("name,tol", [("g9_reverb_live", 2e-6), ("g16_reverb_live_16k", 2e-6)])
def test_reference_equals_the_live_fixtures(name, tol):
    g = load_golden(name)
    sr = int(g["sample_rate"])
    imp, _ = R.impulse(g["noise"], g["decay"], g["wet"], _t(sr), sr)
    hist = np.zeros(sr, f32)
    for k in range(3):
        y, _, hist = R.live(g[f"x_{k}"][0], hist, imp)
        assert _close(y, g[f"y_{k}"][0], tol), k
        assert hist.dtype == np.float32
        if f"buffer_{k}" in g:
            assert np.array_equal(R.bits(hist), R.bits(g[f"buffer_{k}"][0]))
    if "buffer_last" in g:
        assert np.array_equal(R.bits(hist), R.bits(g["buffer_last"][0]))


@pytest.mark.parametrize("clip", [3000, 1200])
def test_reference_equals_g16_gradients(clip):
    g = load_golden(f"g16_reverb_grad_clip{clip}")
    sr = int(g["sample_rate"])
    r = R.module_reference(g["x"], g["w"], g["noise"], g["decay"], g["wet"], _t(sr))
    assert _close(r["mod_y"][0], g["y"], 2e-6)
    for stage, name in (("mod_grad_x", "grad_x"), ("mod_grad_noise", "grad_noise"), ("mod_grad_decay", "grad_decay"), ("mod_grad_wet", "grad_wet")):
        assert _close(r[stage][0], g[name], 2e-5), name


# ---- the analytic gradients against torch double autograd ----------------------------------------------------------------------
@pytest.mark.parametrize("decay", [-100.0, -25.0, -20.0, 5.0, 8.0, 20.0, 100.0])
@pytest.mark.parametrize("sr,n", [(64, 40), (64, 64), (64, 100)])
def test_analytic_gradients_equal_torch_double_autograd(sr, n, decay):
    """n_used < length at (64, 40).  1e-10 of the largest value of each array; a scalar relative to itself."""
    x, w, noise, t = R.module_inputs(sr, n, 2, 1000 + int(decay) + n)
    rv = ddsp.Reverb(Conf(sr), initial_wet=0.3, initial_decay=decay)
    with torch.no_grad():
        rv.noise.copy_(torch.from_numpy(noise))
    assert np.array_equal(rv.t.detach().numpy().reshape(-1), t)
    rv = rv.double()
    xt = torch.from_numpy(x).double().requires_grad_()
    y = rv(xt)
    (y * torch.from_numpy(w).double()).sum().backward()
    r = R.module_reference(x, w, noise, f32(decay), f32(0.3), t)
    for stage, got in (("mod_y", y.detach()), ("mod_grad_x", xt.grad), ("mod_grad_noise", rv.noise.grad), ("mod_grad_decay", rv.decay.grad),
                       ("mod_grad_wet", rv.wet.grad)):
        ref = np.asarray(r[stage][0])
        assert np.max(np.abs(got.numpy() - ref)) <= 1e-10 * np.max(np.abs(ref)), (stage, got, ref)
    # the exact zeros of d noise
    used = min(sr, n)
    assert r["mod_grad_noise"][0][0] == 0.0 and np.all(r["mod_grad_noise"][0][used:] == 0.0)
    assert rv.noise.grad[0] == 0.0 and bool((rv.noise.grad[used:] == 0.0).all())


def test_exact_zeros_and_the_exact_slide():
    noise, t = R.reverb_parameters(1000, 1)
    for n_used in (1, 300, 999, 1000):
        r = R.impulse_backward(R.cotangent(n_used, 2), noise, 8.0, 0.3, t, n_used)
        assert r["noise"][0] == 0.0 and np.all(r["noise"][n_used:] == 0.0) and np.all(r["S_noise"][n_used:] == 0.0)
        assert np.all(r["noise"][1:n_used] != 0.0)
        gn, _, _ = R.impulse_backward_f32(R.cotangent(n_used, 2), noise, 8.0, 0.3, t, n_used)
        assert R.bits(gn[:1])[0] == 0 and np.all(R.bits(gn[n_used:]) == 0)
    hist, xs = R.live_inputs(1000, 77, 3)
    _, _, window = R.live(xs[0], hist, np.ones(1000))
    assert window.dtype == np.float32 and np.array_equal(R.bits(window), R.bits(np.concatenate([hist[77:], xs[0]])))
    hist, xs = R.live_inputs(1025, 1025, 3)
    assert np.isnan(hist).all()
    y, A, window = R.live(xs[0], hist, np.ones(1025))
    assert np.array_equal(R.bits(window), R.bits(xs[0])) and np.isfinite(y).all() and np.isfinite(A).all()


def test_the_case_lists_reach_every_hazard():
    assert (1000, 4096 * 256 + 300) in R.IMPULSE_SHAPES and {(1, 1), (2, 1), (255, 254), (256, 768), (257, 258), (1000, 3000)} <= set(R.IMPULSE_SHAPES)
    assert len(R.IMPULSE_EXTREMES) == 36 and (-100.0, 30.0) in R.IMPULSE_EXTREMES
    assert R.SPECTRAL_SHAPES[-1] == (33, 65537) and 33 * 65537 > R.CAP_SPECTRAL_MUL * 256
    assert R.SPECTRAL_BWD_SHAPES[-1] == (1, 4096 * 256 + 5)
    assert (70000, 300) in R.LIVE_SHAPES and max(70000, 300) > R.CAP_LIVE_FINISH * 256 and (1025, 1025) in R.LIVE_SHAPES
    assert set(R.MEASURED) == set(R.STAGES)
    for decay, wet in R.PARAMS.values():                          # every tap counts: the envelope at the last tap
        assert R.envelope(decay, 1.0)[0] >= 0.03 and wet in (-2.0, 0.3)


# ---- the restatements' errors, which size K: over exactly the GPU test's cases -------------------------------------------------
def _recorded(figs):
    for stage, (fig, k) in figs.items():
        assert fig <= R.MEASURED[stage], f"{stage}: measured {fig:.3f} U S above the recorded {R.MEASURED[stage]} (tests/reverb_reference.py)"
        assert fig <= k


def test_measure_impulse_restatement():
    figs, ok = R.Figures(), True
    for length, n_out in R.IMPULSE_SHAPES:
        for decay, wet in R.impulse_cases(length, n_out):
            ok &= R.check_impulse(R.impulse_f32, figs, length, n_out, decay, wet)
    print(figs.line("host impulse"))
    assert ok
    _recorded(figs)


def test_measure_impulse_backward_restatement():
    figs, ok = R.Figures(), True
    for length, n_used in R.IMPULSE_BWD_SHAPES:
        for decay, wet in R.impulse_backward_cases(length, n_used):
            ok &= R.check_impulse_backward(R.impulse_backward_f32, figs, length, n_used, decay, wet)
    print(figs.line("host impulse backward"))
    assert ok
    _recorded(figs)


def test_measure_spectral_restatements():
    figs, ok = R.Figures(), True
    for rows, bins in R.SPECTRAL_SHAPES:
        ok &= R.check_spectral_mul(R.spectral_mul_f32, figs, rows, bins)
    for rows, bins in R.SPECTRAL_BWD_SHAPES:
        ok &= R.check_spectral_mul_backward(R.spectral_mul_backward_f32, figs, rows, bins)
    print(figs.line("host spectral"))
    assert ok
    _recorded(figs)


live_case = functools.lru_cache(maxsize=None)(R.live_case)
module_case = functools.lru_cache(maxsize=None)(R.module_case)


def _live_run(x, hist, noise, decay, wet, t):
    return R.live_f32(x, hist, R.impulse_f32(noise, decay, wet, t, len(noise)))


@pytest.mark.parametrize("L,n", R.LIVE_SHAPES)
def test_measure_live_restatement(L, n):
    figs = R.Figures()
    ok = R.check_live(_live_run, figs, live_case(L, n))
    print(figs.line(f"host live L {L} n {n}"))
    assert ok
    _recorded(figs)


@pytest.mark.parametrize("sr,n,rows", R.MODULE_SHAPES)
def test_measure_module_restatement(sr, n, rows):
    x, w, noise, t, wet, ref = module_case(sr, n, rows)
    figs = R.Figures()
    got = R.module_f32(x, w, noise, f32(8.0), wet, t, fft_length(n + min(sr, n) - 1))
    ok = R.check_module(got, figs, ref, rows)
    print(figs.line(f"host module sr {sr} n {n} rows {rows}"))
    assert ok
    _recorded(figs)


# ---- the bounds have teeth: one dropped tap is more than 100 bounds away ------------------------------------------------------
TEETH = 100.0


@pytest.mark.parametrize("length,n_out", R.IMPULSE_SHAPES)
def test_teeth_impulse(length, n_out):
    """The last tap written (the crop boundary n_out - 1, or the last tap length - 1) dropped.  With one tap there is only tap 0,
    the constant 1: dropping it is caught exactly."""
    last = min(length, n_out) - 1
    for decay, wet in R.PARAMS.values():
        noise, t = R.reverb_parameters(length, 100 + length)
        ref, arg = R.impulse(noise, f32(decay), f32(wet), t, n_out)
        bad = ref.copy()
        bad[last] = 0.0
        assert R.figure(bad, ref, R.tap_weights(ref, arg)) > TEETH * R.K("impulse")


@pytest.mark.parametrize("length,n_used", R.IMPULSE_BWD_SHAPES)
def test_teeth_impulse_backward(length, n_used):
    """The gradient of the last used tap dropped (n_used taken one short); at n_used == 1 there is no tap but the constant."""
    if n_used == 1:
        return
    for decay, wet in R.PARAMS.values():
        noise, t = R.reverb_parameters(length, 200 + length)
        g = R.cotangent(n_used, 300 + length + n_used)
        r, bad = R.impulse_backward(g, noise, f32(decay), f32(wet), t, n_used), R.impulse_backward(g, noise, f32(decay), f32(wet), t, n_used - 1)
        assert R.figure(bad["noise"], r["noise"], r["S_noise"]) > TEETH * R.K("bwd_noise")


@pytest.mark.parametrize("L,n", R.LIVE_SHAPES)
def test_teeth_live(L, n):
    """The last tap dropped, in every callback."""
    c = live_case(L, n)
    imp = c["imp"].copy()
    imp[L - 1] = 0.0
    h = c["hist0"]
    for x, (y, S, window) in zip(c["xs"], c["ref"]):
        bad, _, h = R.live(x, h, imp)
        assert R.figure(bad, y, S) > TEETH * R.K("live", chunks=c["chunks"]), (L, n)


@pytest.mark.parametrize("sr,n,rows", R.MODULE_SHAPES)
def test_teeth_module(sr, n, rows):
    """The last used tap dropped (the crop boundary for n <= sr, the last tap otherwise): y, grad_x and grad_noise."""
    x, w, noise, t, wet, ref = module_case(sr, n, rows)
    used = ref["used"]
    imp = ref["imp"].copy()
    imp[used - 1] = 0.0
    assert R.figure(R.forward(x, imp)[0], *ref["mod_y"]) > TEETH * R.K("mod_y", rows=rows)
    assert R.figure(R.forward_grad_x(w, imp)[0], *ref["mod_grad_x"]) > TEETH * R.K("mod_grad_x", rows=rows)
    if used > 1:
        gn = ref["mod_grad_noise"][0].copy()
        gn[used - 1] = 0.0
        assert R.figure(gn, *ref["mod_grad_noise"]) > TEETH * R.K("mod_grad_noise", rows=rows)
