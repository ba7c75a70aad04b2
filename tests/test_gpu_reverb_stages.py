"""The reverb's six kernels (csrc/ddsp_reverb.hip) one at a time through their C entry points, and the module path around rocFFT
(reverb._ReverbFunction), against the fp64 reference and the per-element bounds of tests/reverb_reference.py: slow decays at which
every tap counts, every branch of the fused spectral backward, the tile edges of the live kernel, the grid-stride loops beyond
their caps, both softplus branches, and the determinism the reductions claim.  Every output sits in front of a guard zone that
must come back untouched.  Every test prints the figures it asserts on beside their K (`pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp

import reverb_reference as R

pytestmark = pytest.mark.gpu

f32 = np.float32


class Guards(list):
    """Wraps a device launcher: its last return value (guards intact) is collected here, the rest passed on."""

    def wrap(self, launch):
        def run(*args, **kw):
            *out, intact = launch(*args, **kw)
            self.append(intact)
            return out[0] if len(out) == 1 else tuple(out)
        return run

    def intact(self):
        return len(self) > 0 and all(self)


# ---- the impulse kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,n_out", R.IMPULSE_SHAPES)
def test_impulse_kernel(length, n_out):
    """Tap 0 exactly 1, the padding exactly +0, every other tap within K U |tap| (1 + |arg|): at the four named parameter sets,
    and at (1000, 1000) every decay x wet of the extremes (both softplus branches, the sigmoid's far ends, taps that underflow)."""
    figs, guards, ok = R.Figures(), Guards(), True
    for decay, wet in R.impulse_cases(length, n_out):
        ok &= R.check_impulse(guards.wrap(R.device_impulse), figs, length, n_out, decay, wet)
    print(figs.line(f"impulse length {length} n_out {n_out}"))
    assert ok and guards.intact()


# ---- the impulse backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,n_used", R.IMPULSE_BWD_SHAPES)
def test_impulse_backward_kernel(length, n_used):
    """d noise elementwise (exactly +0 at tap 0 and from n_used on), d decay and d wet against the sums of their absolute terms;
    the four named sets and both sides of `-decay > 20`; two launches give the same bits."""
    figs, guards, ok = R.Figures(), Guards(), True
    run = guards.wrap(R.device_impulse_backward)
    for decay, wet in R.impulse_backward_cases(length, n_used):
        ok &= R.check_impulse_backward(run, figs, length, n_used, decay, wet)
    print(figs.line(f"impulse backward length {length} n_used {n_used}"))
    noise, t = R.reverb_parameters(length, 200 + length)
    g = R.cotangent(n_used, 300 + length + n_used)
    a, b = run(g, noise, f32(8.0), f32(0.3), t, n_used), run(g, noise, f32(8.0), f32(0.3), t, n_used)
    assert all(np.array_equal(R.bits(u), R.bits(v)) for u, v in zip(a, b))
    assert ok and guards.intact()


# ---- the spectral products ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,bins", R.SPECTRAL_SHAPES)
def test_spectral_mul_kernel(rows, bins):
    figs, guards = R.Figures(), Guards()
    ok = R.check_spectral_mul(guards.wrap(R.device_spectral_mul), figs, rows, bins)
    print(figs.line(f"spectral_mul rows {rows} bins {bins}"))
    assert ok and guards.intact()


@pytest.mark.parametrize("rows,bins", R.SPECTRAL_BWD_SHAPES)
def test_spectral_mul_backward_kernel(rows, bins):
    """Both outputs within their bounds; GK alone (X and S null: a frozen reverb) and S alone (GK null: x needs no gradient) give
    the bits of the both-outputs form; S is the same bits twice."""
    figs, guards = R.Figures(), Guards()
    run = guards.wrap(R.device_spectral_mul_backward)
    ok = R.check_spectral_mul_backward(run, figs, rows, bins)
    print(figs.line(f"spectral_mul_backward rows {rows} bins {bins}"))
    G, X, Kf = R.spectral_inputs(rows, bins, 500 + rows + bins)
    GK, S = run(G, X, Kf)
    gk_only, none_s = run(G, None, Kf, want_s=False)
    none_gk, s_only = run(G, X, Kf, want_gk=False)
    assert none_s is None and none_gk is None
    assert np.array_equal(R.bits(gk_only.view(f32)), R.bits(GK.view(f32)))
    assert np.array_equal(R.bits(s_only.view(f32)), R.bits(S.view(f32)))
    assert np.array_equal(R.bits(run(G, X, Kf)[1].view(f32)), R.bits(S.view(f32)))
    assert ok and guards.intact()


def test_spectral_mul_backward_refuses_s_without_x():
    G, _, Kf = R.spectral_inputs(2, 5, 1)
    g, k, s = R.dev(G), R.dev(Kf), R.Guarded(10)
    lib = ddsp._lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ddsp_spectral_mul_backward(g.data_ptr(), None, k.data_ptr(), None, s.ptr(), 2, 5, stream) == R.EINVAL
    assert lib.ddsp_spectral_mul_backward(g.data_ptr(), None, k.data_ptr(), None, None, 2, 5, stream) == R.EINVAL
    torch.cuda.synchronize()
    assert s.untouched()


# ---- the live kernels ---------------------------------------------------------------------------------------------------------
live_case = functools.lru_cache(maxsize=None)(R.live_case)


@pytest.mark.parametrize("L,n", R.LIVE_SHAPES)
def test_live_kernels(L, n):
    """Three consecutive callbacks, the two history buffers by turns: y within (130 + chunks + K(impulse)) U of its own absolute
    terms (the third block is 1e-6 of the others), the history bitwise the exact slide, the scratch at exactly
    ddsp_reverb_live_scratch_bytes.  n == L reads no history: the buffer handed in is NaN every time."""
    c = live_case(L, n)
    d = R.LiveDevice(c["noise"], c["decay"], c["wet"], c["t"], n)
    d.set_history(c["hist0"])
    figs, ok = R.Figures(), True
    for k, (x, (y, S, window)) in enumerate(zip(c["xs"], c["ref"])):
        if n == L:
            d.set_history(np.full(L, np.nan, f32))
        got, hist, intact = d.call(x)
        ok &= figs.take("live", R.figure(got, y, S), R.K("live", chunks=c["chunks"]))
        assert np.array_equal(R.bits(hist), R.bits(window)), k
        assert intact, k
    print(figs.line(f"live L {L} n {n} chunks {c['chunks']}"))
    assert ok


def test_live_writes_nothing_for_an_empty_block_and_refuses_without_a_launch():
    """n == 0 returns 0 and writes nothing; history_in == history_out is DDSP_EINVAL and n > L is DDSP_ERANGE, both before any
    launch: y, the histories and the scratch keep every sentinel."""
    L = 1000
    noise, t = R.reverb_parameters(L, 1)
    par = [R.dev(noise), R.dev(np.array([8.0], f32)), R.dev(np.array([0.3], f32)), R.dev(t)]
    lib = ddsp._lib.lib()
    x = R.dev(np.ones(L + 1, f32))
    hin, hout, y = R.Guarded(L), R.Guarded(L), R.Guarded(L + 1)
    scratch = R.Guarded(lib.ddsp_reverb_live_scratch_bytes(L, L + 1) // 4)
    assert lib.ddsp_reverb_live_scratch_bytes(L, 0) == 0 and lib.ddsp_reverb_live_scratch_bytes(0, 5) == 0
    stream = torch.cuda.current_stream().cuda_stream

    def call(h_in, h_out, n):
        return lib.ddsp_reverb_live(x.data_ptr(), h_in.ptr(), h_out.ptr(), *[v.data_ptr() for v in par], y.ptr(), scratch.ptr(), L, n, stream)

    assert call(hin, hout, 0) == 0
    assert call(hin, hin, 77) == R.EINVAL
    assert call(hin, hout, L + 1) == R.ERANGE
    torch.cuda.synchronize()
    assert y.untouched() and hin.untouched() and hout.untouched() and scratch.untouched()


# ---- through the module: _ReverbFunction, rocFFT included -----------------------------------------------------------------------
class Conf:
    def __init__(self, sample_rate):
        self.n_harmonics, self.sample_rate, self.hop_length = 1, sample_rate, 64


module_case = functools.lru_cache(maxsize=None)(R.module_case)


def _module_pass(config, x, w, noise, t, wet):
    """One forward (and backward) of a fresh module -> dict stage -> array or None."""
    rv = ddsp.Reverb(Conf(noise.shape[0]), initial_wet=float(wet), initial_decay=8.0)
    with torch.no_grad():
        rv.noise.copy_(torch.from_numpy(noise))
    assert np.array_equal(rv.t.detach().numpy().reshape(-1), t) and float(rv.wet.detach()) == float(wet)
    rv = rv.cuda()
    if config in ("x", "none"):
        for p in (rv.noise, rv.decay, rv.wet):
            p.requires_grad_(False)
    xg = torch.from_numpy(x).cuda().requires_grad_(config in ("both", "x"))
    if config == "none":
        with torch.no_grad():
            y = rv(xg)
        assert not y.requires_grad
    else:
        y = rv(xg)
        (y * torch.from_numpy(w).cuda()).sum().backward()
    torch.cuda.synchronize()

    def host(g):
        return None if g is None else g.detach().cpu().numpy()

    return dict(mod_y=host(y), mod_grad_x=host(xg.grad), mod_grad_noise=host(rv.noise.grad), mod_grad_decay=host(rv.decay.grad),
                mod_grad_wet=host(rv.wet.grad))


@pytest.mark.parametrize("config", R.GRAD_CONFIGS)
@pytest.mark.parametrize("sr,n,rows", R.MODULE_SHAPES)
def test_through_the_module(sr, n, rows, config):
    """y and every gradient that was asked for against the direct fp64 sums, per element; the others None; d noise exactly 0
    beyond min(n, sr); a second pass gives the same bits.  The kernels the pass launched are then launched at the module's own
    shapes in front of guard zones."""
    x, w, noise, t, wet, ref = module_case(sr, n, rows)
    got = _module_pass(config, x, w, noise, t, wet)
    want_x, want_p = config in ("both", "x"), config in ("both", "params")
    assert (got["mod_grad_x"] is not None) == want_x
    for stage in ("mod_grad_noise", "mod_grad_decay", "mod_grad_wet"):
        assert (got[stage] is not None) == want_p, stage
    figs = R.Figures()
    ok = R.check_module(got, figs, ref, rows)
    print(figs.line(f"module sr {sr} n {n} rows {rows} {config}"))
    assert got["mod_y"].shape == (rows, n) and ok
    used = ref["used"]
    if want_p:
        gn = got["mod_grad_noise"]
        assert gn.shape == (sr,) and R.bits(gn[:1])[0] == 0 and np.all(R.bits(gn[used:]) == 0)
    again = _module_pass(config, x, w, noise, t, wet)
    for stage, a in got.items():
        assert (a is None) == (again[stage] is None) and (a is None or np.array_equal(R.bits(a), R.bits(again[stage]))), stage
    # the same launches in front of guards: the impulse cropped to `used`, the products at the transform's bins, the backward
    guards = Guards()
    bins = ddsp.reverb.fft_length(n + used - 1) // 2 + 1
    G, X, Kf = R.spectral_inputs(rows, bins, sr + n)
    imp = guards.wrap(R.device_impulse)(noise, f32(8.0), wet, t, used)
    assert R.figure(imp, ref["imp"], R.tap_weights(ref["imp"], R.envelope(8.0, t)[1])) <= R.K("impulse")
    guards.wrap(R.device_spectral_mul)(X, Kf)
    guards.wrap(R.device_spectral_mul_backward)(G, X if want_p else None, Kf, want_gk=want_x or not want_p, want_s=want_p)
    guards.wrap(R.device_impulse_backward)(R.cotangent(used, 5), noise, f32(8.0), wet, t, used)
    assert guards.intact()
