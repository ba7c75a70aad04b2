"""The f0 refinement without a GPU: conditions on the method, put to the fp64 definition of
tests/harmonic_refine_reference.py; the package's CPU path against that definition; the frames that must not move; the clamp;
refine=0; the entry points' binding and argument checks; and the bound the device tests use.

The device bound, per frame.  The kernel differs from the definition by (1) its fp32 arithmetic and (2) the hardware sine and cosine,
allowed EPS_SIN in the worst direction: eps_C = sqrt(2) EPS_SIN sum_j |w x|, eps_D = sqrt(2) EPS_SIN sum_j |w' x|, carried through
  |d num| <= sum_k k (|D_k| eps_C + |C_k| eps_D + eps_C eps_D),   |d den| <= sum_k k^2 (2 |C_k| eps_C + eps_C^2),
  |d g|   <= (sr / 2 pi) (|d num| + |num / den| |d den|) / (den - |d den|)  + 2^-23 f0 (the mean's fp32 weights, the fp32 store)
(reference.bound).  (1) is measured by evaluating the step in exactly the kernel's arithmetic with exact sines
(reference.step_fp32) on the device tests' own inputs, as a share of (2) frame by frame; test_device_bound prints the shares,
asserts that they stay below FP32_SHARE and that the bound is vacuous nowhere (den > 2 |d den| on every measured frame).  The device
tests allow 2 (1 + FP32_SHARE) times (2): the factor 2 is for EPS_SIN, which is assumed and not documented."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import harmonic_analysis_reference as ref
import harmonic_refine_reference as rr

EINVAL, ERANGE = -1, -2


def package(audio, f0, hop, sr, H, W, voiced=None, **kw):
    """The package's CPU path on fp64 tensors: rows [B, N], f0 [B, T] -> the refined track [B, T] as numpy."""
    v = None if voiced is None else torch.from_numpy(np.asarray(voiced))[..., None]
    g = ddsp.refine_f0(torch.from_numpy(np.asarray(audio, np.float64)), torch.from_numpy(np.asarray(f0, np.float64))[..., None],
                       hop, sr, H, W, voiced=v, **kw)
    assert g.dtype == torch.float64 and g.shape == np.shape(f0) + (1,)
    return g[..., 0].numpy()


@functools.lru_cache(maxsize=None)
def vibrato(noise):
    y, f0, _, conf = ref.vibrato_case(noise=noise, seconds=1.0)
    return y, f0.astype(np.float64), conf


def method_case(name):
    """-> (audio, the true track, the start, (hop, sr, H, W), caps after two steps: max cents, rms cents, residual)."""
    if name == "steady 220 Hz, 8 cents off":
        y, true, start = rr.steady_case(220.0, 16000, 64, 512, 20, 40, 8.0)
        return y, true, start, (64, 16000, 20, 512), (0.05, None, 5e-4)
    if name == "steady 110 Hz, 9.5 cents off":
        y, true, start = rr.steady_case(110.0, 16000, 128, 1024, 60, 24, 9.5)
        return y, true, start, (128, 16000, 60, 1024), (0.05, None, 5e-4)
    if name == "vibrato from the grid":
        y, f0, conf = vibrato(0.0)
        return y, f0, rr.to_grid(f0), conf, (2.0, 1.2, 0.013)
    if name == "vibrato from the true track":
        y, f0, conf = vibrato(0.0)
        return y, f0, f0, conf, (2.0, None, 0.013)
    if name == "noisy vibrato from the grid":
        y, f0, conf = vibrato(0.05)
        return y, f0, rr.to_grid(f0), conf, (6.0, 2.0, None)
    assert name == "glide from the grid"
    y, true, start = rr.glide_case()
    return y, true, start, (512, 44100, 60, 2048), (1.5, None, 0.02)


@pytest.mark.parametrize("name", ["steady 220 Hz, 8 cents off", "steady 110 Hz, 9.5 cents off", "vibrato from the grid",
                                  "vibrato from the true track", "noisy vibrato from the grid", "glide from the grid"])
def test_method(name):
    y, true, start, (hop, sr, H, W), (cap_max, cap_rms, cap_resid) = method_case(name)
    frames = rr.interior_frames(len(true), hop, W)
    tracks = rr.refine(y, start, hop, sr, H, W, iterations=2)
    for i, g in enumerate(tracks):
        c = rr.cents(g, true)[frames]
        print(f"{name}, after {i} steps: max {np.abs(c).max():.4f} cents, rms {np.sqrt(np.mean(c ** 2)):.4f}, "
              f"residual {100 * rr.residual(y, g, hop, sr, H, W):.4f} % of the signal's rms")
    c = rr.cents(tracks[2], true)[frames]
    assert np.abs(c).max() <= cap_max
    assert cap_rms is None or np.sqrt(np.mean(c ** 2)) <= cap_rms
    assert cap_resid is None or rr.residual(y, tracks[2], hop, sr, H, W) <= cap_resid
    if "from the grid" in name or "off" in name:                 # the start was worse than the cap: the cap shows a repair
        assert np.abs(rr.cents(start, true)[frames]).max() > 4 * cap_max or "noisy" in name


def test_white_noise_stays_finite_and_within_max_cents():
    rng = np.random.default_rng(0)
    x, f0 = 0.1 * rng.standard_normal(40 * 64), np.full(40, 200.0)
    for max_cents in (50.0, 5.0):
        g = rr.refine(x, f0, 64, 16000, 20, 512, iterations=3, max_cents=max_cents)[-1]
        moved = np.abs(rr.cents(g, f0)).max()
        print(f"white noise, max_cents {max_cents}: moved {moved:.2f} cents in 3 steps")
        assert np.isfinite(g).all() and moved <= max_cents * (1 + 1e-12)
        assert np.abs(package(x[None], f0[None], 64, 16000, 20, 512, iterations=3, max_cents=max_cents) - g).max() <= 1e-9


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_cpu_path_matches_the_definition_in_fp64(shape):
    """Sums of at most 2048 fp64 terms in another order: 1e-9 Hz is 1e4 times what that can do to a track of a few hundred Hz."""
    B, T, hop, W, H, sr = shape
    audio, f0, voiced = ref.gliding_rows(*shape)
    worst = 0.0
    for its in (1, 2):
        g = package(audio, f0, hop, sr, H, W, voiced, iterations=its)
        for b in range(B):
            want = rr.refine(audio[b], f0[b], hop, sr, H, W, voiced[b], iterations=its)[-1]
            dead = ~rr.alive_frames(f0[b].astype(np.float64), voiced[b])
            assert np.array_equal(g[b, dead].view(np.uint64), f0[b, dead].astype(np.float64).view(np.uint64)), (b, its)     # bit for bit
            worst = max(worst, np.abs(g[b, ~dead] - want[~dead]).max())
            if rr.interior_frames(T, hop, W) and its == 1:
                assert not np.array_equal(g[b, ~dead], f0[b, ~dead].astype(np.float64))
    print(f"{shape}: CPU fp64 path against the definition, max difference {worst:.3e} Hz")
    assert worst <= 1e-9


def test_without_an_interior_frame_the_track_comes_back():
    audio, f0, _ = ref.gliding_rows(1, 1, 64, 256, 20, 16000)                    # T = 1
    assert np.array_equal(package(audio, f0, 64, 16000, 20, 256), f0.astype(np.float64))
    assert np.array_equal(rr.refine(audio[0], f0[0], 64, 16000, 20, 256)[-1], f0[0].astype(np.float64))
    audio, f0, voiced = ref.gliding_rows(2, 6, 32, 256, 20, 16000)               # W = 256 > N = 192
    assert np.array_equal(package(audio, f0, 32, 16000, 20, 256, voiced), f0.astype(np.float64), equal_nan=True)
    assert np.array_equal(rr.refine(audio[0], f0[0], 32, 16000, 20, 256, voiced[0])[-1], f0[0].astype(np.float64), equal_nan=True)


def test_the_clamp_holds():
    y, true, start = rr.steady_case(220.0, 16000, 64, 512, 20, 40, 8.0)
    for g in (rr.refine(y, start, 64, 16000, 20, 512, iterations=2, max_cents=3.0)[-1],
              package(y[None], start[None], 64, 16000, 20, 512, iterations=2, max_cents=3.0)[0]):
        moved = rr.cents(g, start)
        print(f"max_cents 3 on a track 8 cents above the tone: moved {moved.min():.6f} .. {moved.max():.6f} cents")
        assert np.abs(moved + 3.0).max() <= 1e-9                 # every frame is carried to the lower edge, the ends by the ratio


def test_refine_0_is_the_call_without_the_argument():
    shape = B, T, hop, W, H, sr = ref.GPU_SHAPES[0]
    audio, f0, voiced = ref.gliding_rows(*shape)
    args = (torch.from_numpy(audio), torch.from_numpy(f0)[..., None], hop, sr, H, W)
    v = torch.from_numpy(voiced)[..., None]
    plain, zero, two = (ddsp.harmonic_residual(*args, voiced=v, **kw) for kw in ({}, dict(refine=0), dict(refine=2)))
    for key in ("f0", "a", "c"):
        assert torch.equal(plain[2][key], zero[2][key]), key
    assert torch.equal(plain[0], zero[0]) and torch.equal(plain[1], zero[1])
    assert torch.equal(ddsp.harmonic_analysis(*args, voiced=v)["a"], ddsp.harmonic_analysis(*args, voiced=v, refine=0)["a"])
    want = ddsp.refine_f0(*args, voiced=v, iterations=2)
    assert torch.equal(two[2]["f0"], torch.where(torch.isfinite(want) & (want > 0), want, torch.zeros(())))   # the track demodulated
    assert not torch.equal(two[2]["a"], plain[2]["a"])
    conf = type("Conf", (), dict(n_harmonics=H, sample_rate=sr, hop_length=hop, n_fft=W))
    assert torch.equal(ddsp.HarmonicAnalyzer(conf, refine=2)(args[0], args[1], v)["a"], two[2]["a"])
    assert torch.equal(ddsp.HarmonicAnalyzer(conf)(args[0], args[1], v)["a"], plain[2]["a"])
    assert np.array_equal(ddsp.refine_f0(*args, iterations=0).numpy().view(np.uint32), args[1].numpy().view(np.uint32))


def test_symbols_are_bound():
    order = list(ddsp._lib.EXPORTS)
    at = order.index("ddsp_harm_resynth")
    assert order[at + 1:at + 3] == ["ddsp_harm_refine_workspace_bytes", "ddsp_harm_refine"]          # the header's order
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert L.ddsp_harm_refine_workspace_bytes.restype is ctypes.c_size_t and L.ddsp_harm_refine.restype is ctypes.c_int
    assert list(L.ddsp_harm_refine_workspace_bytes.argtypes) == [ctypes.c_long, ctypes.c_long, ctypes.c_int]
    assert list(L.ddsp_harm_refine.argtypes) == ([ctypes.c_void_p] * 8 + [ctypes.c_long] * 2 + [ctypes.c_int] * 4
                                                 + [ctypes.c_float, ctypes.c_uint, ctypes.c_void_p])
    base = L.ddsp_harm_workspace_bytes(2, 16, 64)
    assert L.ddsp_harm_refine_workspace_bytes(2, 16, 64) >= base + 4 * 4096 + 4 * 2 * 16
    assert L.ddsp_harm_refine_workspace_bytes(0, 16, 64) == 0 and L.ddsp_harm_refine_workspace_bytes(1 << 40, 1 << 40, 64) == 0
    assert ddsp.refine_f0 is ddsp.analysis.refine_f0 and "refine_f0" in ddsp.__all__


def test_argument_checks_return_before_any_launch():
    """Every call here is refused (or is the empty batch) by the host checks: the pointers are never dereferenced."""
    L = ddsp._lib.lib()
    p, q, N = 4096, 8192, None                                   # non-null, aligned addresses that are never read
    call = lambda ptrs, B=2, T=16, hop=64, W=256, H=20, sr=16000, mc=50.0, fl=0: L.ddsp_harm_refine(      # noqa: E731
        *ptrs, B, T, hop, W, H, sr, mc, fl, N)
    good = (p, p, p, N, q, N, N, p)                              # voiced, num_out and den_out may be null
    assert call((N,) * 8, B=0) == 0
    for i in (0, 1, 2, 4, 7):
        assert call(tuple(N if k == i else v for k, v in enumerate(good))) == EINVAL, i
    assert call((p, p, p, N, p, N, N, p)) == EINVAL              # f0_out is f0_in
    assert call(good, W=255) == EINVAL and call(good, W=0) == EINVAL and call(good, B=-1) == EINVAL and call(good, T=0) == EINVAL
    assert call(good, hop=0) == EINVAL and call(good, H=0) == EINVAL and call(good, sr=0) == EINVAL and call(good, fl=1) == EINVAL
    assert call(good, mc=0.0) == EINVAL and call(good, mc=-1.0) == EINVAL and call(good, mc=float("nan")) == EINVAL
    assert call(good, mc=float("inf")) == EINVAL and call((p, p, p, N, q, N, N, p + 4)) == EINVAL
    assert call(good, W=4098) == ERANGE and call(good, H=257) == ERANGE and call(good, B=1 << 40, T=1 << 40) == ERANGE


def test_wrapper_refuses_bad_inputs():
    audio, f0 = torch.zeros(2, 16 * 64), torch.full((2, 16, 1), 200.0)
    args = (64, 16000, 20, 256)
    for fn in (ddsp.harmonic_analysis, ddsp.harmonic_residual):
        with pytest.raises(ValueError):
            fn(audio, f0, *args, refine=-1)
        with pytest.raises(ValueError):
            fn(audio, f0, *args, refine=1, max_cents=0.0)
    with pytest.raises(ValueError):
        ddsp.refine_f0(audio, f0, *args, iterations=-1)
    with pytest.raises(ValueError):
        ddsp.refine_f0(audio, f0, *args, max_cents=-2.0)
    with pytest.raises(ValueError):
        ddsp.refine_f0(audio[:, :-1], f0, *args)
    with pytest.raises(ValueError):
        ddsp.HarmonicAnalyzer(type("Conf", (), dict(n_harmonics=20, sample_rate=16000, hop_length=64, n_fft=256)), refine=-1)
    with pytest.raises(RuntimeError):
        ddsp.refine_f0(audio.clone().requires_grad_(), f0, *args)
    with pytest.raises(RuntimeError):
        ddsp.refine_f0(audio, f0.clone().requires_grad_(), *args)
    silent = ddsp.refine_f0(audio, f0, *args)                    # den = 0: the track comes back, in fp32
    assert silent.dtype == torch.float32 and torch.equal(silent, f0)
    assert ddsp.refine_f0(audio[:0], f0[:0], *args).shape == (0, 16, 1)


def test_device_bound():
    """The fp32 arithmetic of the kernel as a share of the sine / cosine part, frame by frame, for the first step from the given
    fp32 track and for the second step from the first iterate rounded to fp32 (what the device tests compare)."""
    worst = np.zeros(3)
    for shape in ref.GPU_SHAPES:
        B, T, hop, W, H, sr = shape
        audio, f0, voiced = ref.gliding_rows(*shape)
        for b in range(B):
            first = rr.step(audio[b], f0[b], f0[b], hop, sr, H, W, voiced[b])[0].astype(np.float32)
            for start in (f0[b], first):
                want = rr.step(audio[b], start, f0[b], hop, sr, H, W, voiced[b])
                got = rr.step_fp32(audio[b], start, f0[b], hop, sr, H, W, voiced[b])
                dnum, dden, dg, vacuous = rr.bound(audio[b], start, hop, sr, H, W, voiced[b])
                assert not vacuous, (shape, b)
                measured = dg > 0
                alive = rr.alive_frames(f0[b].astype(np.float64), voiced[b])
                assert np.array_equal(measured, alive & np.isin(np.arange(T), rr.interior_frames(T, hop, W))), (shape, b)
                assert np.array_equal(got[0][~alive].view(np.uint32), f0[b][~alive].view(np.uint32))
                if not measured.any():
                    assert np.array_equal(got[0].view(np.uint32), f0[b].view(np.uint32))
                    continue
                share = [np.abs(got[i] - want[i])[measured] / d[measured] for i, d in ((0, dg), (1, dnum), (2, dden))]
                print(f"{shape} row {b}: sine part of g <= {dg.max():.3e} Hz ({np.abs(rr.cents(start + dg, start))[measured].max():.3f} cents); "
                      f"fp32 share of g {share[0].max():.4f}, num {share[1].max():.4f}, den {share[2].max():.4f}; "
                      f"den / |d den| >= {(want[2][measured] / dden[measured]).min():.1f}")
                worst = np.maximum(worst, [s.max() for s in share])
    print(f"fp32 arithmetic as a share of the sine / cosine part: g {worst[0]:.4f}, num {worst[1]:.4f}, den {worst[2]:.4f}; "
          f"FP32_SHARE = {rr.FP32_SHARE:g}")
    assert worst.max() <= rr.FP32_SHARE
