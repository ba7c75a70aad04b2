"""The f0 refinement on the device (csrc/ddsp_harm.hip: ddsp_harm_refine) against the fp64 definition of
tests/harmonic_refine_reference.py, step by step, then end to end through harmonic_residual and AutoEncoder.analyse.  The bound is
per frame, 2 (1 + FP32_SHARE) times what EPS_SIN can do to that frame (derived in tests/test_harmonic_refine_host.py); every test
prints its observed maximum before it asserts."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import harmonic_analysis_reference as ref
import harmonic_refine_reference as rr
import yin_reference
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

ALLOW = 2.0 * (1.0 + rr.FP32_SHARE)
GRID_CAP = 8192                                                  # csrc/ddsp_harm.hip: kMaxBlocks
GUARD = 64                                                       # floats behind every output, which must stay as they were
SENTINEL = -12345.0


def device_step(audio, f0, anchor, hop, sr, H, W, voiced=None, max_cents=50.0):
    """One ddsp_harm_refine call on rows [B, N], f0 and anchor [B, T] (numpy fp32) -> (g, num, den) [B, T]; the guard zones behind
    the three outputs are checked here, on every call."""
    B, T = f0.shape
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (audio, f0, anchor)]
    v = None if voiced is None else torch.from_numpy(np.ascontiguousarray(voiced)).to(torch.uint8).cuda()
    outs = [torch.full((B * T + GUARD,), SENTINEL, device="cuda") for _ in range(3)]
    L = ddsp._lib.lib()
    ws = torch.empty(L.ddsp_harm_refine_workspace_bytes(B, T, hop), device="cuda", dtype=torch.uint8)
    rc = L.ddsp_harm_refine(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), None if v is None else v.data_ptr(),
                            outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), B, T, hop, W, H, sr, max_cents, 0,
                            torch.cuda.current_stream().cuda_stream)
    ddsp._lib.check(rc, "ddsp_harm_refine")
    outs = [o.cpu().numpy() for o in outs]
    assert all((o[B * T:] == np.float32(SENTINEL)).all() for o in outs)
    return tuple(o[:B * T].reshape(B, T) for o in outs)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def compare(shape, audio, start, anchor, voiced, got, frames=None):
    """The device's (g, num, den) of one step from `start` against the definition, frame by frame under each frame's own bound.
    -> the largest ratios error / bound of g on measured frames, of g on the frames at the clip's ends, of num and of den."""
    B, T, hop, W, H, sr = shape
    worst = np.zeros(4)
    inter = rr.interior_frames(T, hop, W)
    for b in range(B):
        want = rr.step(audio[b], start[b], anchor[b], hop, sr, H, W, voiced[b], frames=frames)
        dnum, dden, dg, vacuous = rr.bound(audio[b], start[b], hop, sr, H, W, voiced[b], frames=frames)
        assert not vacuous, b                                    # a vacuous bound is a failed test
        alive = rr.alive_frames(start[b].astype(np.float64), voiced[b])
        measured = alive & np.isin(np.arange(T), inter if frames is None else [t for t in inter if t in frames])
        assert np.array_equal(measured, dg > 0), b               # no alive interior frame is left out
        assert same_bits(got[0][b][~alive], start[b][~alive]), b                 # frames that are not alive: bit for bit
        if not inter:
            assert same_bits(got[0][b], start[b]), b
            continue
        assert not got[1][b][~measured].any() and not got[2][b][~measured].any() or frames is not None, b
        err = [np.abs(got[i][b].astype(np.float64) - want[i]) for i in range(3)]
        if measured.any():
            worst[0] = max(worst[0], (err[0][measured] / dg[measured]).max())
            worst[2] = max(worst[2], (err[1][measured] / dnum[measured]).max())
            worst[3] = max(worst[3], (err[2][measured] / dden[measured]).max())
        if frames is None:                                       # the ends carry the ratio of the nearest interior frame
            for edge, sel in ((inter[0], np.arange(T) < inter[0]), (inter[-1], np.arange(T) > inter[-1])):
                sel = sel & alive
                if sel.any():
                    carried = start[b][sel].astype(np.float64) / start[b][edge] * dg[edge] if alive[edge] else 0.0
                    worst[1] = max(worst[1], (err[0][sel] / (carried + 2.0 ** -23 * start[b][sel])).max())
    return worst


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape, the first iterate of the definition rounded to fp32, and the device's first step: computed once."""
    B, T, hop, W, H, sr = shape
    audio, f0, voiced = ref.gliding_rows(*shape)
    first = np.stack([rr.step(audio[b], f0[b], f0[b], hop, sr, H, W, voiced[b])[0] for b in range(B)]).astype(np.float32)
    return audio, f0, voiced, first, device_step(audio, f0, f0, hop, sr, H, W, voiced)


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_one_step_matches_the_definition(shape):
    audio, f0, voiced, _, got = case(shape)
    worst = compare(shape, audio, f0, f0, voiced, got)
    print(f"{shape}: one step from the given track, error / derived bound: g {worst[0]:.3f} (ends {worst[1]:.3f}), num {worst[2]:.3f}, "
          f"den {worst[3]:.3f}; allowed {ALLOW:g}")
    assert np.isfinite(got[0][rr.alive_frames(f0.astype(np.float64), voiced)]).all()
    assert worst.max() <= ALLOW


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_second_step_from_the_definitions_first_iterate(shape):
    """Teacher-forced: the device's step is judged alone, from the same fp32 track as the definition's."""
    B, T, hop, W, H, sr = shape
    audio, f0, voiced, first, _ = case(shape)
    got = device_step(audio, first, f0, hop, sr, H, W, voiced)
    worst = compare(shape, audio, first, f0, voiced, got)
    print(f"{shape}: the second step, error / derived bound: g {worst[0]:.3f} (ends {worst[1]:.3f}), num {worst[2]:.3f}, "
          f"den {worst[3]:.3f}; allowed {ALLOW:g}")
    assert worst.max() <= ALLOW


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_the_clamp_is_reached_and_held(shape):
    """From a track 8 cents above the given one with max_cents = 3: every frame stays within 3 cents of that start (plus the fp32
    rounding of the edge, 2^-23 relative = 2.1e-4 cents), and where the clip has interior frames some of them sit on the edge."""
    B, T, hop, W, H, sr = shape
    audio, f0, voiced, _, _ = case(shape)
    start = (f0.astype(np.float64) * 2.0 ** (8.0 / 1200.0)).astype(np.float32)
    g = device_step(audio, start, start, hop, sr, H, W, voiced, max_cents=3.0)[0]
    alive = rr.alive_frames(start.astype(np.float64), voiced)
    moved = rr.cents(g[alive], start[alive])
    print(f"{shape}: max_cents 3 from 8 cents above: moved {moved.min():.5f} .. {moved.max():.5f} cents")
    assert same_bits(g[~alive], start[~alive])
    assert np.abs(moved).max() <= 3.0 + 2.1e-4
    if rr.interior_frames(T, hop, W):
        assert moved.min() <= -3.0 + 2.1e-4
        want = np.stack([rr.step(audio[b], start[b], start[b], hop, sr, H, W, voiced[b], max_cents=3.0)[0] for b in range(B)])
        at_edge = alive & (np.abs(rr.cents(np.where(alive, want, 1.0), np.where(alive, start, 1.0)) + 3.0) < 1e-9)
        assert at_edge.any() and np.abs(rr.cents(g[at_edge], start[at_edge]) + 3.0).max() <= 2.1e-4


def test_deterministic_and_rows_independent():
    shape = B, T, hop, W, H, sr = ref.GPU_SHAPES[1]
    audio, f0, voiced, _, first = case(shape)
    again = device_step(audio, f0, f0, hop, sr, H, W, voiced)
    assert all(same_bits(x, y) for x, y in zip(first, again))
    for b in range(B):
        alone = device_step(audio[b:b + 1], f0[b:b + 1], f0[b:b + 1], hop, sr, H, W, voiced[b:b + 1])
        assert all(same_bits(x[0], y[b]) for x, y in zip(alone, first)), b
    flipped = device_step(audio[::-1], f0[::-1], f0[::-1], hop, sr, H, W, voiced[::-1])
    assert all(same_bits(x[::-1], y) for x, y in zip(flipped, first))


def test_python_entry_runs_the_same_steps():
    shape = B, T, hop, W, H, sr = ref.GPU_SHAPES[1]
    audio, f0, voiced, _, (g1, _, _) = case(shape)
    g2 = device_step(audio, g1, f0, hop, sr, H, W, voiced)[0]
    args = (torch.from_numpy(audio).cuda(), torch.from_numpy(f0).cuda()[..., None], hop, sr, H, W)
    v = torch.from_numpy(voiced).cuda()[..., None]
    for its, want in ((0, f0), (1, g1), (2, g2)):
        got = ddsp.refine_f0(*args, voiced=v, iterations=its)
        assert got.is_cuda and got.shape == (B, T, 1) and same_bits(got[..., 0].cpu().numpy(), want), its
    plain, zero, two = (ddsp.harmonic_residual(*args, voiced=v, return_complex=True, **kw) for kw in ({}, dict(refine=0), dict(refine=2)))
    assert all(torch.equal(plain[2][k], zero[2][k]) for k in ("f0", "a", "c")) and torch.equal(plain[1], zero[1])
    assert same_bits(two[2]["f0"][..., 0].cpu().numpy(), np.where(rr.alive_frames(g2.astype(np.float64)), g2, np.float32(0)))
    along = ddsp.harmonic_residual(args[0], torch.from_numpy(g2).cuda()[..., None], hop, sr, H, W, voiced=v)
    assert torch.equal(two[0], along[0]) and torch.equal(two[2]["a"], along[2]["a"])


def test_nan_sample_reaches_only_the_frames_that_hold_it():
    """The sample is in the middle of the clip, outside the windows of the first and the last interior frame (whose g the frames at
    the clip's ends follow, by the definition).  The frames that hold it keep their f0."""
    shape = B, T, hop, W, H, sr = ref.GPU_SHAPES[1]
    audio, f0, voiced, _, (g0, n0, d0) = case(shape)
    at = 11 * hop + 5
    bad = audio.copy()
    bad[0, at] = np.nan
    g, num, den = device_step(bad, f0, f0, hop, sr, H, W, voiced)
    holds = np.array([ref.frame_start(t, hop, W) <= at < ref.frame_start(t, hop, W) + W for t in range(T)])
    inter = rr.interior_frames(T, hop, W)
    assert holds.sum() == W // hop and not holds[inter[0]] and not holds[inter[-1]]
    assert same_bits(g[1:], g0[1:]) and same_bits(num[1:], n0[1:]) and same_bits(den[1:], d0[1:])
    assert same_bits(g[0, ~holds], g0[0, ~holds]) and same_bits(num[0, ~holds], n0[0, ~holds])
    assert same_bits(g[0, holds], f0[0, holds])
    live = holds & (d0[0] > 0)
    assert live.any() and np.isnan(den[0, live]).all() and not same_bits(g0[0, live], f0[0, live])


def test_more_frames_than_the_grid():
    """hop 2, W 64, H 3 over cap + 4 frames in each of two rows: the blocks walk a second frame.  Row 0's interior
    frames are all below the cap (a block's first frame), row 1's all above it (a later turn of the stride), and row 1 launched
    alone has its frames in other blocks and other turns than inside the batch: the same bits either way."""
    B, T, hop, W, H, sr = shape = (2, GRID_CAP + 4, 2, 64, 3, 16000)
    audio, f0, voiced = ref.gliding_rows(*shape)
    got = device_step(audio, f0, f0, hop, sr, H, W, voiced)
    inter = rr.interior_frames(T, hop, W)
    frames = [inter[0], inter[0] + 1, T // 2, inter[-1] - 1, inter[-1]]
    assert inter[-1] < GRID_CAP <= T + inter[0]
    worst = compare(shape, audio, f0, f0, voiced, got, frames=frames)
    print(f"frames either side of the cap: error / derived bound: g {worst[0]:.3f}, num {worst[2]:.3f}, den {worst[3]:.3f}")
    assert worst.max() <= ALLOW
    alone = device_step(audio[1:], f0[1:], f0[1:], hop, sr, H, W, voiced[1:])
    assert all(same_bits(x[0], y[1]) for x, y in zip(alone, got))


def residual_share(audio, resid, T, hop, W):
    _, samples = ref.interior(T, hop, W)
    return float(np.sqrt(np.mean(resid.astype(np.float64)[samples] ** 2) / np.mean(audio.astype(np.float64)[samples] ** 2)))


def test_residual_after_two_steps_on_the_device():
    """The host table's caps, put to harmonic_residual(..., refine=2) on the device: the steady 220 Hz tone from 8 cents off and the
    vibrato from its grid rounding."""
    y, true, start = rr.steady_case(220.0, 16000, 64, 512, 20, 40, 8.0)
    vy, vf0, _, (hop, sr, H, W) = ref.vibrato_case(seconds=1.0)
    for name, audio, true, start, caps in (("steady 220 Hz", y, true, start, (0.05, None, 5e-4)),
                                           ("vibrato from the grid", vy, vf0.astype(np.float64), rr.to_grid(vf0), (2.0, 1.2, 0.013))):
        T = len(true)
        a = torch.from_numpy(audio.astype(np.float32)).cuda()[None]
        f = torch.from_numpy(start.astype(np.float32)).cuda()[None, :, None]
        frames = rr.interior_frames(T, hop, W)
        figures = []
        for steps in (0, 2):
            _, resid, z = ddsp.harmonic_residual(a, f, hop, sr, H, W, refine=steps)
            c = rr.cents(z["f0"][0, :, 0].cpu().numpy(), true)[frames]
            figures.append((np.abs(c).max(), np.sqrt(np.mean(c ** 2)), residual_share(audio, resid[0].cpu().numpy(), T, hop, W)))
            print(f"{name}, refine={steps}: max {figures[-1][0]:.4f} cents, rms {figures[-1][1]:.4f}, residual {100 * figures[-1][2]:.4f} %")
        assert figures[1][0] <= caps[0] and (caps[1] is None or figures[1][1] <= caps[1]) and figures[1][2] <= caps[2]
        assert figures[0][2] > 2 * caps[2]                       # the start was outside the cap


def test_autoencoder_analyse_with_refinement():
    """Section 14's two 44.1 kHz tone rows and its noise row through AutoEncoder(tracker='yin').analyse: two steps leave less of
    both tones than the decoded track does, and the noise row stays finite."""
    rng = np.random.default_rng(41)
    L = 2048 + 512 * 40
    x = [yin_reference.tone(f, L, 44100, rng, top=8000.0) for f in (196.0, 523.25)] + [0.3 * rng.standard_normal(L)]
    x = torch.from_numpy(np.stack(x).astype(np.float32)).cuda()
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    T = L // AEConf.hop_length
    clip = x[:, :T * AEConf.hop_length]
    rms = lambda v: v.double().pow(2).mean(-1).sqrt().cpu().numpy()                                # noqa: E731
    ratio = {}
    for steps in (0, 2):
        z = ae.analyse(x, return_complex=True, refine=steps)
        assert sorted(z) == ["C", "a", "c", "f0"] and z["f0"].shape == (3, T, 1)
        assert all(torch.isfinite(z[k]).all() for k in ("f0", "a", "c"))
        harm = ddsp.harmonic_resynthesis(z["C"], z["f0"], AEConf.hop_length, AEConf.sample_rate)
        ratio[steps] = rms(clip - harm) / rms(clip)
        print(f"refine={steps}: (clip - resynthesis of analyse(clip)) rms / clip rms: {ratio[steps]}; "
              f"median f0 of the tone rows: {z['f0'][:2, :, 0].median(dim=1).values.cpu().numpy()}")
    assert (ratio[2][:2] < ratio[0][:2]).all()
    assert np.isfinite(ratio[2]).all()
    assert torch.equal(ae.analyse(x)["a"], ae.analyse(x, refine=0)["a"])
    assert "H" in ae.analyse(x, noise=True, refine=1)


def test_outside_the_kernel_range_runs_the_torch_path_on_the_device():
    """W = 4098: the stock-op path in fp32 on the device against the fp64 definition, on the measured frames.  torch chooses the
    order of the W fp32 terms of C_k and D_k: any order is within W 2^-24 sum_j |w x| (and |w' x|), and the fp32 angle is within
    2 pi 2^-24 rad; `bound` carries an error of sqrt(2) EPS_SIN sum_j |w x| through the step, so the same chain gives this path
    (W 2^-24 + 2 pi 2^-24) / (sqrt(2) EPS_SIN) times that figure, plus the fp32 rounding of the value, which `bound` has."""
    B, T, hop, W, H, sr = shape = (1, 8, 1024, 4098, 12, 16000)
    audio, f0, voiced = ref.gliding_rows(*shape)
    dev = ddsp.refine_f0(torch.from_numpy(audio).cuda(), torch.from_numpy(f0).cuda()[..., None], hop, sr, H, W, iterations=1)
    got = dev[0, :, 0].cpu().numpy()
    want = rr.step(audio[0], f0[0], f0[0], hop, sr, H, W)[0]
    _, _, dg, vacuous = rr.bound(audio[0], f0[0], hop, sr, H, W)
    measured = dg > 0
    factor = (W * 2.0 ** -24 + 2 * np.pi * 2.0 ** -24) / (np.sqrt(2.0) * ref.EPS_SIN)
    ratio = (np.abs(got - want)[measured] / (factor * dg[measured])).max()
    print(f"W = 4098, device torch path against the definition: error / bound {ratio:.3f} (the bound: {factor * dg[measured].max():.2e} Hz)")
    alive = rr.alive_frames(f0[0].astype(np.float64))
    assert dev.is_cuda and measured.sum() >= 2 and not vacuous and same_bits(got[~alive], f0[0][~alive])
    assert ratio <= 1.0
