"""The harmonic analysis on the device (csrc/ddsp_harm.hip) against the fp64 definition of tests/harmonic_analysis_reference.py,
through the real oscillator bank, and through AutoEncoder.analyse.  TOL_C is derived in tests/test_harmonic_analysis_host.py;
every test prints its observed maximum before it asserts."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import harmonic_analysis_reference as ref
import yin_reference
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

TOL_C = ref.TOL_C
GRID_CAP = 8192                                                  # csrc/ddsp_harm.hip: kMaxBlocks


def device(audio, f0, hop, sr, H, W, voiced=None):
    """rows [B, N], f0 [B, T] (numpy) -> (C complex64, a, c, harm, resid) from ONE harmonic_residual call on the device."""
    v = None if voiced is None else torch.from_numpy(np.ascontiguousarray(voiced)).cuda()[..., None]
    harm, resid, z = ddsp.harmonic_residual(torch.from_numpy(np.ascontiguousarray(audio)).cuda(),
                                            torch.from_numpy(np.ascontiguousarray(f0)).cuda()[..., None], hop, sr, H, W, voiced=v,
                                            return_complex=True)
    assert z["C"].dtype == torch.complex64 and z["a"].shape == f0.shape + (1,) and harm.shape == audio.shape
    return z["C"].cpu().numpy(), z["a"][..., 0].cpu().numpy(), z["c"].cpu().numpy(), harm.cpu().numpy(), resid.cpu().numpy()


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape, the definition's answer and the device's: computed once, shared, not modified."""
    B, T, hop, W, H, sr = shape
    audio, f0, voiced = ref.gliding_rows(*shape)
    want = [ref.analyse(audio[b], f0[b], hop, sr, H, W, voiced[b]) for b in range(B)]
    got = device(audio, f0, hop, sr, H, W, voiced)
    return audio, f0, voiced, want, got


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_kernel_matches_the_definition(shape):
    B, T, hop, W, H, sr = shape
    audio, f0, voiced, want, (C, a, c, _, _) = case(shape)
    keep = ref.keep_mask(f0.reshape(-1), sr, H, voiced.reshape(-1)).reshape(B, T, H)
    if T >= 4:                                                   # the inputs reach the masks: a top harmonic that comes and goes,
        assert keep[..., -1].any() and not keep[..., -1].all() and not keep.any(axis=-1).all()      # and frames without any
    eC = ea = ec = 0.0
    for b in range(B):
        Cr, ar, cr = want[b]
        eC = max(eC, np.abs(C[b] - Cr).max())
        ea = max(ea, np.abs(a[b] - ar).max())
        loud = ar > 100 * TOL_C
        ec = max(ec, (np.abs(c[b] - cr)[loud] * ar[loud, None]).max()) if loud.any() else ec
        assert np.array_equal(C[b] == 0, Cr == 0) and (c[b][ar == 0] == np.float32(1.0 / H)).all(), b     # the masks, exactly
    print(f"{shape}: max |C - fp64| = {eC:.3e} (TOL_C {TOL_C:g}), |a - fp64| = {ea:.3e}, a |c - fp64| = {ec:.3e}")
    assert np.isfinite(C).all() and np.isfinite(c).all()
    assert eC <= TOL_C
    assert ea <= H * TOL_C
    assert ec <= (H + 1) * TOL_C


def test_hardware_sine_is_within_the_figure_the_bound_assumes():
    """TOL_C rests on EPS_SIN, which no document gives: this puts it to the device.  One unit sample per frame under the window's
    peak (hop 128 > W 64: frames share nothing) makes C[t, k] = (2 / norm) exp(-2 pi i k theta): the hardware cosine and sine of
    64 x 256 angles, scaled by 1 / 16.  What else is in the difference is below EPS_SIN / 4: the phase word (k 2^-33 turns <=
    1.9e-7 rad), its fp32 conversion (2^-25 turns = 1.9e-7 rad) and the fp32 scale (6e-8)."""
    T, hop, W, H, sr = 64, 128, 64, 256, 16000
    rng = np.random.default_rng(77)
    f0 = rng.uniform(20.0, 31.0, (1, T)).astype(np.float32)      # 256 f0 <= 8000: every harmonic is kept
    audio = np.zeros((1, T * hop), dtype=np.float32)
    audio[0, [ref.frame_start(t, hop, W) + W // 2 for t in range(T)]] = 1.0
    C = device(audio, f0, hop, sr, H, W)[0]
    Cr = ref.analyse(audio[0], f0[0], hop, sr, H, W)[0]
    assert np.abs(np.abs(Cr) - 2.0 / (W / 2)).max() < 1e-12
    err = np.abs(C[0] - Cr).max() * (W / 2) / 2.0
    print(f"hardware cosine / sine over {T * H} angles: max error {err:.3e} (EPS_SIN {ref.EPS_SIN:g})")
    assert err <= ref.EPS_SIN


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_resynthesis_of_the_device_amplitudes(shape):
    B, T, hop, W, H, sr = shape
    audio, f0, _, _, (C, _, _, harm, resid) = case(shape)
    alone = ddsp.harmonic_resynthesis(torch.from_numpy(C).cuda(), torch.from_numpy(f0).cuda()[..., None], hop, sr).cpu().numpy()
    assert same_bits(alone, harm)                                # its own phase pass, and the one the analysis left
    assert same_bits(resid, audio - harm)
    worst = 0.0
    for b in range(B):
        err = np.abs(harm[b] - ref.resynth(C[b].astype(np.complex128), f0[b], hop, sr)).max()
        worst = max(worst, err / max(1.0, np.abs(C[b]).sum(axis=-1).max()))
    print(f"{shape}: max |harm - fp64 resynthesis of the same C| / max(1, max_t sum_k |C|) = {worst:.3e}")
    assert worst <= 1e-5


def test_more_frames_than_the_grid():
    """hop 2, W 64, H 3 over cap + 4 frames: the first blocks walk a second frame (and a second segment).  Row 1 launched alone
    has its frames in other blocks and other turns of the stride than inside the batch: the same bits either way."""
    B, T, hop, W, H, sr = shape = (2, GRID_CAP + 4, 2, 64, 3, 16000)
    audio, f0, voiced = ref.gliding_rows(*shape)
    C, a, c, harm, _ = device(audio, f0, hop, sr, H, W, voiced)
    frames = [0, 1, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, GRID_CAP + 3]
    Cr, ar, _ = ref.analyse(audio[0], f0[0], hop, sr, H, W, voiced[0], frames=frames)
    err = np.abs(C[0, frames] - Cr[frames]).max()
    print(f"frames either side of the cap: max |C - fp64| = {err:.3e}")
    assert err <= TOL_C and np.abs(a[0, frames] - ar[frames]).max() <= H * TOL_C
    herr = np.abs(harm[0] - ref.resynth(C[0].astype(np.complex128), f0[0], hop, sr)).max() / max(1.0, np.abs(C[0]).sum(axis=-1).max())
    print(f"segments either side of the cap: resynthesis off by {herr:.3e}")
    assert herr <= 1e-5
    C1, a1, c1, harm1, _ = device(audio[1:], f0[1:], hop, sr, H, W, voiced[1:])
    assert same_bits(C1[0], C[1]) and same_bits(a1[0], a[1]) and same_bits(c1[0], c[1]) and same_bits(harm1[0], harm[1])


@pytest.mark.parametrize("hop,W,T,H,m", ref.STATIONARY)
def test_round_trip_through_the_oscillator_bank(hop, W, T, H, m):
    """Stationary controls -> OscillatorBank -> analysis.  The bank is within 1e-5 of its definition (the project's audio
    contract); step 4's factor 2 makes that 2e-5 on C, which the window average does not amplify."""
    f0, a, c = ref.stationary_controls(hop, W, T, H, m)
    conf = type("Conf", (), dict(n_harmonics=H, sample_rate=16000, hop_length=hop, n_fft=W))
    ctl = {"f0": torch.from_numpy(f0).cuda()[None, :, None], "a": torch.from_numpy(a).cuda()[None, :, None],
           "c": torch.from_numpy(c).cuda()[None]}
    y = ddsp.OscillatorBank(conf).cuda()(ctl)
    harm, resid, z = ddsp.harmonic_residual(y, ctl["f0"], hop, 16000, H, W, return_complex=True)
    module = ddsp.HarmonicAnalyzer(conf).cuda()(y, ctl["f0"])
    assert sorted(module) == ["a", "c", "f0"] and torch.equal(module["a"], z["a"]) and torch.equal(module["c"], z["c"])
    frames, samples = ref.interior(T, hop, W)
    cn = c.astype(np.float64) / c.astype(np.float64).sum(axis=-1, keepdims=True)
    err = np.abs(np.abs(z["C"][0].cpu().numpy().astype(np.complex128)) - a[:, None] * cn)[frames].max()
    rmax = float(resid[0, samples].abs().max())
    bound = 1e-5 + H * (2e-5 + TOL_C) + 1e-5
    print(f"{(hop, W, T, H, m)}: | |C| - a c | <= {err:.3e} (bound {2e-5 + TOL_C:.1e}), interior residual max {rmax:.3e} (bound {bound:.2e})")
    assert err <= 2e-5 + TOL_C
    assert rmax <= bound
    back = z["a"] * z["c"]                                       # the dict is the bank's: a c is what went in
    assert np.abs(back[0].cpu().numpy() - a[:, None] * cn)[frames].max() <= 2e-5 + TOL_C + 1e-6


def test_deterministic_and_rows_independent():
    shape = B, T, hop, W, H, sr = ref.GPU_SHAPES[1]
    audio, f0, voiced, _, first = case(shape)
    again = device(audio, f0, hop, sr, H, W, voiced)
    assert all(same_bits(x, y) for x, y in zip(first, again))
    for b in range(B):
        alone = device(audio[b:b + 1], f0[b:b + 1], hop, sr, H, W, voiced[b:b + 1])
        assert all(same_bits(x[0], y[b]) for x, y in zip(alone, first)), b
    flipped = device(audio[::-1], f0[::-1], hop, sr, H, W, voiced[::-1])
    assert all(same_bits(x[::-1], y) for x, y in zip(flipped, first))


def test_nan_sample_reaches_only_the_frames_that_hold_it():
    shape = B, T, hop, W, H, sr = ref.GPU_SHAPES[1]
    audio, f0, voiced, _, (C0, a0, c0, harm0, _) = case(shape)
    at = 11 * hop + 5
    bad = audio.copy()
    bad[0, at] = np.nan
    C, a, c, harm, resid = device(bad, f0, hop, sr, H, W, voiced)
    holds = np.array([ref.frame_start(t, hop, W) <= at < ref.frame_start(t, hop, W) + W for t in range(T)])
    assert holds.sum() == W // hop
    assert same_bits(C[1:], C0[1:]) and same_bits(harm[1:], harm0[1:]) and same_bits(a[1:], a0[1:])
    assert same_bits(C[0, ~holds], C0[0, ~holds]) and same_bits(a[0, ~holds], a0[0, ~holds]) and same_bits(c[0, ~holds], c0[0, ~holds])
    live = holds & (a0[0] > 0)                                   # a masked frame stays 0 whatever its samples
    assert live.any() and np.isnan(a[0, live]).all() and np.isnan(C[0, live, 0]).all()
    first, last = np.flatnonzero(holds)[[0, -1]]
    outside = np.ones(T * hop, dtype=bool)
    outside[(first - 1) * hop + hop // 2:(last + 1) * hop + hop // 2 + 1] = False
    assert same_bits(harm[0, outside], harm0[0, outside]) and np.isnan(harm[0]).any() and np.isnan(resid[0, at])


def test_autoencoder_analyse_without_weights():
    """The two 44.1 kHz tone rows (and the noise row) of tests/test_gpu_yin.py through AutoEncoder(tracker='yin').analyse."""
    rng = np.random.default_rng(41)
    L = 2048 + 512 * 40
    x = [yin_reference.tone(f, L, 44100, rng, top=8000.0) for f in (196.0, 523.25)] + [0.3 * rng.standard_normal(L)]
    x = torch.from_numpy(np.stack(x).astype(np.float32)).cuda()
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    z = ae.analyse(x, return_complex=True)
    T = L // AEConf.hop_length
    assert sorted(z) == ["C", "a", "c", "f0"]
    assert z["f0"].shape == z["a"].shape == (3, T, 1) and z["c"].shape == (3, T, AEConf.n_harmonics)
    clip = x[:, :T * AEConf.hop_length]
    y = ae.decoder.harmonics({k: z[k] for k in ("f0", "a", "c")})
    assert y.shape == clip.shape and torch.isfinite(y).all()
    rms = lambda v: v.double().pow(2).mean(-1).sqrt().cpu().numpy()                                # noqa: E731
    # The residual that can be small is the one that keeps the analysed phases: the bank starts every harmonic at phase 0 and
    # the tones do not, so clip - bank(a, c) has the power of both (rms ratio ~ sqrt(2): 1.39 and 1.36 measured on the
    # tone rows), whatever the analysis returns.  The sanity condition is therefore put to the resynthesis of C, and the bank's
    # output, which has the same |C|, is compared with it in power: the two differ by the interpolation of a C whose phase
    # turns by up to 0.66 rad per frame (harmonic 8 of a pitch decoded 10 cents off), cos(0.33) = 0.95 at worst mid-frame,
    # so within 10 %.
    harm = ddsp.harmonic_resynthesis(z["C"], z["f0"], AEConf.hop_length, AEConf.sample_rate)
    ratio = rms(clip - harm) / rms(clip)
    power = rms(y) / rms(harm)
    print(f"(clip - resynthesis of analyse(clip)) rms / clip rms: {ratio}; (clip - decoder.harmonics) rms / clip rms: "
          f"{rms(clip - y) / rms(clip)}; bank rms / resynthesis rms: {power}")
    assert (ratio[:2] < 1.0).all()
    assert (np.abs(power[:2] - 1.0) < 0.1).all()
    assert sorted(ae.analyse(x)) == ["a", "c", "f0"]


def test_empty_batch():
    audio, f0 = torch.zeros((0, 16 * 64), device="cuda"), torch.zeros((0, 16, 1), device="cuda")
    harm, resid, z = ddsp.harmonic_residual(audio, f0, 64, 16000, 20, 256, return_complex=True)
    assert harm.shape == resid.shape == (0, 1024) and harm.is_cuda
    assert z["C"].shape == (0, 16, 20) and z["a"].shape == z["f0"].shape == (0, 16, 1) and z["c"].shape == (0, 16, 20)
    assert ddsp.harmonic_resynthesis(z["C"], f0, 64, 16000).shape == (0, 1024)
    with pytest.raises(ValueError, match="voiced is on"):         # a host mask with device audio is refused before any launch
        ddsp.harmonic_analysis(torch.zeros((1, 1024), device="cuda"), torch.ones((1, 16, 1), device="cuda"), 64, 16000, 20, 256,
                               voiced=torch.ones((1, 16, 1), dtype=torch.bool))
    with pytest.raises(RuntimeError):
        ddsp.harmonic_analysis(torch.zeros((1, 1024), device="cuda", requires_grad=True), torch.ones((1, 16, 1), device="cuda"), 64, 16000, 20, 256)


def test_outside_the_kernel_range_runs_the_torch_path_on_the_device():
    """W = 4098: the same stock-op path as CPU tensors take, on the device; each is within rounding of the definition."""
    B, T, hop, W, H, sr = shape = (1, 6, 1024, 4098, 12, 16000)
    audio, f0, voiced = ref.gliding_rows(*shape)
    args = (hop, sr, H, W)
    cpu = ddsp.harmonic_residual(torch.from_numpy(audio), torch.from_numpy(f0)[..., None], *args, return_complex=True)
    dev = ddsp.harmonic_residual(torch.from_numpy(audio).cuda(), torch.from_numpy(f0).cuda()[..., None], *args, return_complex=True)
    assert dev[0].is_cuda and dev[2]["C"].is_cuda and dev[2]["C"].dtype == torch.complex64
    err = float((dev[2]["C"].cpu() - cpu[2]["C"]).abs().max())
    herr = float((dev[0].cpu() - cpu[0]).abs().max())
    print(f"W = 4098, device torch path against the CPU path: C {err:.3e}, harm {herr:.3e}")
    assert err <= TOL_C
    assert float((dev[2]["a"].cpu() - cpu[2]["a"]).abs().max()) <= H * TOL_C
    assert herr <= 1e-5 * max(1.0, float(cpu[2]["a"].max()))
