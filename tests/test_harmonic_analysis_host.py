"""The harmonic analysis without a GPU: the definition's own behaviour (tests/harmonic_analysis_reference.py,
fp64), the package's CPU path against it, the masks, the entry points' binding and argument checks, and the bound the device
tests use.

TOL_C, the bound on |C_device - C_fp64| (absolute; the inputs have peak 1).  The kernel differs from the definition by
  (1) its fp32 arithmetic: the window rounded to fp32, fl32(w x), one FMA per term into an fp32 accumulator, a 32-bit phase word
      multiplied by k and converted to fp32 (2^-25 turns of rounding), and
  (2) the hardware sine and cosine, taken here to be within EPS_SIN = 2e-6 (absolute) of the true values on [-0.5, 0.5] turns.
(1) is measured by evaluating the definition in exactly that arithmetic with exact sines (reference.analyse_fp32) on the device
tests' own inputs; (2) is bounded per frame by sqrt(2) EPS_SIN (2 / norm) sum_j |w x|, every term's error taken in the worst
direction.  test_device_bound prints both and asserts that twice the fp32 part (another order of the same sums is as valid) plus
the sine part (2.39e-6) stays below TOL_C = 5e-6, and TOL_C below the project's audio contract of 1e-5 max|audio|.  The factor 2
between the derived figure and TOL_C is for EPS_SIN, the one figure taken and not derived: it admits a hardware error of 4.4e-6."""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import harmonic_analysis_reference as ref

EINVAL, ERANGE = -1, -2


def package(audio, f0, hop, sr, H, W, voiced=None):
    """The package's CPU path on fp64 tensors: rows [B, N], f0 [B, T] -> (C, a, c, harm) as numpy."""
    v = None if voiced is None else torch.from_numpy(np.asarray(voiced))[..., None]
    harm, resid, z = ddsp.harmonic_residual(torch.from_numpy(np.asarray(audio, np.float64)), torch.from_numpy(np.asarray(f0, np.float64))[..., None],
                                            hop, sr, H, W, voiced=v, return_complex=True)
    assert z["C"].dtype == torch.complex128 and z["a"].dtype == torch.float64 and harm.dtype == torch.float64
    assert np.array_equal(resid.numpy(), np.asarray(audio, np.float64) - harm.numpy(), equal_nan=True)
    return z["C"].numpy(), z["a"].numpy()[..., 0], z["c"].numpy(), harm.numpy()


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_cpu_path_matches_the_definition_in_fp64(shape):
    B, T, hop, W, H, sr = shape
    audio, f0, voiced = ref.gliding_rows(*shape)
    C, a, c, harm = package(audio, f0, hop, sr, H, W, voiced)
    worst = 0.0
    for b in range(B):
        Cr, ar, cr = ref.analyse(audio[b], f0[b], hop, sr, H, W, voiced[b])
        hr = ref.resynth(Cr, f0[b], hop, sr)
        worst = max(worst, np.abs(C[b] - Cr).max(), np.abs(a[b] - ar).max(), np.abs(c[b] - cr).max(), np.abs(harm[b] - hr).max())
    print(f"{shape}: CPU fp64 path against the definition, max difference {worst:.3e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("case", ref.STATIONARY)
def test_stationary_controls_are_recovered(case):
    hop, W, T, H, m = case
    f0, a, c = ref.stationary_controls(*case)
    y = ref.bank(f0, a, c, hop, 16000)
    C, _, _ = ref.analyse(y, f0, hop, 16000, H, W)
    frames, samples = ref.interior(T, hop, W)
    cn = c.astype(np.float64) / c.astype(np.float64).sum(axis=-1, keepdims=True)   # (the fp32 c sums to 1 within 1e-7 only)
    err = np.abs(np.abs(C[frames]) - (a[:, None] * cn)[frames]).max()
    resid = y - ref.resynth(C, f0, hop, 16000)
    ratio = np.sqrt(np.mean(resid[samples] ** 2) / np.mean(y[samples] ** 2))
    print(f"{case}: | |C| - a c | <= {err:.3e} on {len(frames)} interior frames, residual rms / signal rms = {ratio:.3e}")
    assert len(frames) >= 2
    assert err <= 1e-12
    assert ratio <= 1e-12


def test_vibrato_leaves_a_small_residual():
    y, f0, _, (hop, sr, H, W) = ref.vibrato_case()
    C, _, _ = ref.analyse(y, f0, hop, sr, H, W)
    _, samples = ref.interior(len(f0), hop, W)
    resid = y - ref.resynth(C, f0, hop, sr)
    ratio = np.sqrt(np.mean(resid[samples] ** 2) / np.mean(y[samples] ** 2))
    print(f"vibrato: interior residual rms / signal rms = {ratio:.4f}")
    assert ratio <= 0.02


def test_residual_is_the_noise_that_was_added():
    y, f0, e, (hop, sr, H, W) = ref.vibrato_case(noise=0.05)
    C, _, _ = ref.analyse(y, f0, hop, sr, H, W)
    _, samples = ref.interior(len(f0), hop, W)
    resid = (y - ref.resynth(C, f0, hop, sr))[samples]
    corr = np.corrcoef(resid, e[samples])[0, 1]
    print(f"noise 0.05: correlation of residual and noise {corr:.4f}, rms ratio {np.sqrt(np.mean(resid ** 2) / np.mean(e[samples] ** 2)):.4f}")
    assert corr >= 0.9


def test_masks():
    hop, W, H, sr, T = 64, 256, 20, 16000, 12
    rng = np.random.default_rng(5)
    f0 = np.full((1, T), 500.0, dtype=np.float32)               # 16 harmonics at or below 8000 Hz (16 x 500 is not above it)
    f0[0, 2], f0[0, 3], f0[0, 4] = 0.0, -500.0, np.nan
    voiced = np.ones((1, T), dtype=bool)
    voiced[0, 6] = False
    audio = rng.standard_normal((1, T * hop))
    audio[0, 8 * hop - 96:8 * hop + 160] = 0.0                  # frame 8's whole window
    for where, (C, a, c) in (("reference", [v[None] for v in ref.analyse(audio[0], f0[0], hop, sr, H, W, voiced[0])]),
                             ("cpu", package(audio, f0, hop, sr, H, W, voiced)[:3])):
        amp = np.abs(C[0])
        assert (amp[0, :16] > 0).all() and not amp[:, 16:].any(), where       # the strict >: harmonic 16 stays
        for t in (2, 3, 4, 6, 8):
            assert not amp[t].any() and a[0, t] == 0 and np.array_equal(c[0, t], np.full(H, 1.0 / H)), (where, t)
        for t in (0, 1, 5, 7, 9, 10, 11):
            assert a[0, t] > 0 and abs(c[0, t].sum() - 1) < 1e-12 and np.isfinite(C[0, t]).all(), (where, t)
    # without the voiced mask frame 6 is analysed; the others do not move
    C2 = package(audio, f0, hop, sr, H, W)[0]
    assert np.abs(C2[0, 6]).max() > 0 and np.array_equal(np.delete(C2, 6, axis=1), np.delete(C, 6, axis=1))
    z = ddsp.harmonic_analysis(torch.from_numpy(audio), torch.from_numpy(f0.astype(np.float64))[..., None], hop, sr, H, W)
    assert sorted(z) == ["a", "c", "f0"] and z["f0"].shape == (1, T, 1) and z["c"].shape == (1, T, H)
    assert z["f0"][0, 2:5, 0].tolist() == [0.0, 0.0, 0.0] and float(z["f0"][0, 0, 0]) == 500.0     # the track that was demodulated


def test_a_single_frame():
    audio, f0, _ = ref.gliding_rows(1, 1, 64, 256, 20, 16000)
    C, a, c, harm = package(audio, f0, 64, 16000, 20, 256)
    Cr, ar, cr = ref.analyse(audio[0], f0[0], 64, 16000, 20, 256)
    assert C.shape == (1, 1, 20) and harm.shape == (1, 64) and ar[0] > 0
    assert np.abs(C[0] - Cr).max() <= 1e-10 and np.abs(harm[0] - ref.resynth(Cr, f0[0], 64, 16000)).max() <= 1e-10


def test_nan_sample_reaches_only_the_frames_that_hold_it():
    B, T, hop, W, H, sr = shape = ref.GPU_SHAPES[0]
    audio, f0, voiced = ref.gliding_rows(*shape)
    f0, bad = np.abs(np.nan_to_num(f0, nan=300.0)) + 1.0, audio.copy()
    at = 5 * hop + 3
    bad[0, at] = np.nan
    C, _, _, harm = package(bad, f0, hop, sr, H, W)
    C0, _, _, harm0 = package(audio, f0, hop, sr, H, W)
    holds = np.array([ref.frame_start(t, hop, W) <= at < ref.frame_start(t, hop, W) + W for t in range(T)])
    assert holds.sum() == W // hop and np.isnan(C[0, holds, 0]).all()
    assert np.array_equal(C[0, ~holds], C0[0, ~holds]) and np.array_equal(C[1], C0[1]) and np.array_equal(harm[1], harm0[1])
    touched = np.isnan(harm[0])
    first, last = np.flatnonzero(holds)[[0, -1]]
    assert not touched[:(first - 1) * hop + hop // 2].any() and not touched[(last + 1) * hop + hop // 2 + 1:].any() and touched.any()


def test_symbols_are_bound_and_the_abi_is_still_5():
    order = list(ddsp._lib.EXPORTS)
    names = ["ddsp_harm_workspace_bytes", "ddsp_harm_analysis", "ddsp_harm_resynth"]
    at = order.index("ddsp_yin_salience")
    assert order[at + 1:at + 4] == names                         # the table keeps the header's order
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert L.ddsp_harm_workspace_bytes.restype is ctypes.c_size_t and L.ddsp_harm_analysis.restype is ctypes.c_int
    assert list(L.ddsp_harm_analysis.argtypes) == [ctypes.c_void_p] * 7 + [ctypes.c_long] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    assert list(L.ddsp_harm_resynth.argtypes) == ([ctypes.c_void_p] * 6 + [ctypes.c_long] * 2 + [ctypes.c_int] * 3
                                                  + [ctypes.c_uint, ctypes.c_void_p])
    assert L.ddsp_harm_workspace_bytes(2, 16, 64) >= 4 * 2 * 16 * 64
    assert L.ddsp_harm_workspace_bytes(0, 16, 64) == 0 and L.ddsp_harm_workspace_bytes(1 << 40, 1 << 40, 64) == 0
    assert ddsp.harmonic_analysis is ddsp.analysis.harmonic_analysis and issubclass(ddsp.HarmonicAnalyzer, torch.nn.Module)


def test_argument_checks_return_before_any_launch():
    """Every call here is refused (or is the empty batch) by the host checks: the pointers are never dereferenced."""
    L = ddsp._lib.lib()
    p, N = 4096, None                                            # a non-null, aligned address that is never read
    ana = lambda ptrs, B=2, T=16, hop=64, W=256, H=20, sr=16000: L.ddsp_harm_analysis(*ptrs, B, T, hop, W, H, sr, N)   # noqa: E731
    syn = lambda ptrs, B=2, T=16, hop=64, H=20, sr=16000, fl=0: L.ddsp_harm_resynth(*ptrs, B, T, hop, H, sr, fl, N)    # noqa: E731
    good = (p, p, N, p, p, p, p)                                 # voiced may be null
    assert ana((N,) * 7, B=0) == 0 and syn((N,) * 6, B=0) == 0
    for i in (0, 1, 3, 4, 5, 6):
        assert ana(tuple(N if k == i else v for k, v in enumerate(good))) == EINVAL, i
    assert ana(good, W=255) == EINVAL and ana(good, W=4097) == EINVAL and ana(good, W=0) == EINVAL
    assert ana(good, B=-1) == EINVAL and ana(good, T=0) == EINVAL and ana(good, hop=0) == EINVAL and ana(good, H=0) == EINVAL
    assert ana(good, W=4098) == ERANGE and ana(good, H=257) == ERANGE and ana(good, B=1 << 40, T=1 << 40) == ERANGE
    good = (p, p, N, p, N, p)                                    # audio and resid may be null together
    for i in (0, 1, 3, 5):
        assert syn(tuple(N if k == i else v for k, v in enumerate(good))) == EINVAL, i
    assert syn((p, p, N, p, p, p)) == EINVAL                     # a residual needs the audio
    assert syn(good, fl=2) == EINVAL and syn(good, hop=-3) == EINVAL and syn((p + 4, p, N, p, N, p)) == EINVAL
    assert syn(good, H=257) == ERANGE and syn(good, B=1 << 40, T=1 << 40) == ERANGE


def test_wrapper_refuses_bad_inputs():
    audio, f0 = torch.zeros(2, 16 * 64), torch.full((2, 16, 1), 200.0)
    args = (64, 16000, 20, 256)
    with pytest.raises(ValueError):
        ddsp.harmonic_analysis(audio[:, :-1], f0, *args)
    with pytest.raises(ValueError):
        ddsp.harmonic_analysis(audio, f0[..., 0], *args)
    with pytest.raises(ValueError):
        ddsp.harmonic_analysis(audio, f0, 64, 16000, 20, 255)
    with pytest.raises(ValueError):
        ddsp.harmonic_analysis(audio, f0, *args, voiced=torch.ones(2, 15, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="voiced is on"):         # a mask on another device than the audio: never a kernel's pointer
        ddsp.harmonic_analysis(audio, f0, *args, voiced=torch.ones(2, 16, 1, dtype=torch.bool, device="meta"))
    half = ddsp.harmonic_analysis(audio.half() + 0.25, f0, *args, return_complex=True)            # 16-bit audio is analysed in fp32
    assert half["a"].dtype == torch.float32 and half["C"].dtype == torch.complex64 and float(half["a"].min()) >= 0
    with pytest.raises(ValueError):
        ddsp.harmonic_resynthesis(torch.zeros(2, 16, 20, dtype=torch.complex32), f0, 64, 16000)
    with pytest.raises(ValueError):
        ddsp.harmonic_residual(audio[:1], f0, *args)
    with pytest.raises(ValueError):
        ddsp.harmonic_resynthesis(torch.zeros(2, 16, 20), f0, 64, 16000)
    with pytest.raises(RuntimeError):
        ddsp.harmonic_analysis(audio.clone().requires_grad_(), f0, *args)
    with pytest.raises(RuntimeError):
        ddsp.harmonic_analysis(audio, f0.clone().requires_grad_(), *args)
    with pytest.raises(RuntimeError):
        ddsp.harmonic_resynthesis(torch.zeros(2, 16, 20, dtype=torch.complex64, requires_grad=True), f0, 64, 16000)
    z = ddsp.HarmonicAnalyzer(type("Conf", (), dict(n_harmonics=20, sample_rate=16000, hop_length=64, n_fft=256)))(audio, f0)
    assert not list(ddsp.HarmonicAnalyzer(type("Conf", (), dict(n_harmonics=20, sample_rate=16000, hop_length=64, n_fft=256))).parameters())
    assert z["a"].dtype == torch.float32 and not z["a"].any() and torch.equal(z["c"], torch.full((2, 16, 20), 1 / 20))
    empty = ddsp.harmonic_residual(audio[:0], f0[:0], *args, return_complex=True)
    assert empty[0].shape == empty[1].shape == (0, 1024) and empty[2]["C"].shape == (0, 16, 20) and empty[2]["a"].shape == (0, 16, 1)


def test_cpu_path_keeps_fp32():
    """fp32 in, fp32 out.  torch chooses the order of the W = 256 fp32 terms, so the bound is the worst case of any order,
    W 2^-24 (2 / norm) sum |w x| <= 256 x 6e-8 x 2 = 3.1e-5 at peak 1, plus 2 x 2.4e-7 for the fp32 angle: 1e-4 covers both."""
    B, T, hop, W, H, sr = shape = ref.GPU_SHAPES[0]
    audio, f0, voiced = ref.gliding_rows(*shape)
    z = ddsp.harmonic_analysis(torch.from_numpy(audio), torch.from_numpy(f0)[..., None], hop, sr, H, W,
                               voiced=torch.from_numpy(voiced)[..., None], return_complex=True)
    assert z["C"].dtype == torch.complex64 and z["a"].dtype == torch.float32
    err = max(np.abs(z["C"][b].numpy() - ref.analyse(audio[b], f0[b], hop, sr, H, W, voiced[b])[0]).max() for b in range(B))
    print(f"CPU fp32 path against the definition: {err:.3e}")
    assert err <= 1e-4


def test_device_bound():
    fp32_part, sine_part, peak = 0.0, 0.0, np.inf
    for shape in ref.GPU_SHAPES:
        B, T, hop, W, H, sr = shape
        audio, f0, voiced = ref.gliding_rows(*shape)
        peak = min(peak, float(np.abs(audio).max(axis=-1).min()))
        for b in range(B):
            want = ref.analyse(audio[b], f0[b], hop, sr, H, W, voiced[b])[0]
            got, gain = ref.analyse_fp32(audio[b], f0[b], hop, sr, H, W, voiced[b])
            e, s = np.abs(got - want).max(), np.sqrt(2.0) * ref.EPS_SIN * gain.max()
            print(f"{shape} row {b}: fp32 arithmetic {e:.3e}, sine / cosine within {ref.EPS_SIN:g}: {s:.3e}")
            fp32_part, sine_part = max(fp32_part, e), max(sine_part, s)
    derived = 2 * fp32_part + sine_part
    print(f"derived bound: 2 x {fp32_part:.3e} + {sine_part:.3e} = {derived:.3e}; TOL_C = {ref.TOL_C:g}; smallest peak {peak:g}")
    assert derived <= ref.TOL_C <= 1e-5 * peak
