"""The control transformation on the device (csrc/ddsp_transform.hip) against the fp64 definition of
tests/control_transform_reference.py, through the real oscillator bank, and through AutoEncoder.transform.  TOL_A is derived in
tests/test_control_transform_host.py; every test prints its observed maximum before it asserts."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import control_transform_reference as ref
import harmonic_analysis_reference as href
from ddsp_pytorch_amd import analysis
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

TOL_A = ref.TOL_A
SR = ref.SAMPLE_RATE


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def controls(x):
    return dict(f0=cuda(x["f0"])[..., None], a=cuda(x["a"])[..., None], c=cuda(x["c"]), H=cuda(x["N"]))


def ratios(x, B, T_out):
    """r and q as the package hands them to the kernel (formed on the device), for the definition."""
    dev = torch.device("cuda", torch.cuda.current_device())
    return [analysis._semitone_ratio(cuda(x[k]), B, T_out, dev, "test", k).cpu().numpy() for k in ("transpose", "formant")]


def device(x, H_out):
    out = ddsp.transform_controls(controls(x), SR, transpose=cuda(x["transpose"]), formant=cuda(x["formant"]), positions=cuda(x["pos"]),
                                  n_harmonics=H_out)
    assert all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def compare(got, want, b, H_out):
    """One row of the device's answer against the definition's -> (error of A', of a', of N', each over its scale); the exact
    parts are asserted here."""
    f0, a, c, N = got["f0"][b, :, 0], got["a"][b, :, 0], got["c"][b], got["H"][b]
    assert np.isfinite(f0).all() and np.isfinite(a).all() and np.isfinite(c).all() and np.isfinite(N).all(), b
    assert same_bits(f0, want["f0"]), b
    quiet = want["a"] == 0
    assert not a[quiet].any() and (c[quiet] == np.float32(1) / np.float32(H_out)).all(), b         # the fill, exactly
    assert np.array_equal(c[~quiet] == 0, want["A"][~quiet] == 0) and (a[~quiet] > 0).all(), b     # the zero pattern, exactly
    assert np.array_equal(N == 0, want["N"] == 0), b
    A = a.astype(np.float64)[:, None] * c.astype(np.float64) * ~quiet[:, None]
    scale, nscale = np.maximum(want["scale"], 1e-30), np.maximum(want["nscale"], 1e-30)
    return ((np.abs(A - want["A"]) / scale[:, None]).max(), (np.abs(a - want["a"]) / scale).max(),
            (np.abs(N - want["N"]) / nscale[:, None]).max())


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape, the definition's answer per row and the device's: computed once, shared, not modified."""
    B, T, T_out, H, H_out, F = shape
    x = ref.rows(shape)
    r, q = ratios(x, B, T_out)
    want = [ref.transform(x["f0"][b], x["a"][b], x["c"][b], x["N"][b], x["pos"][b], r[b], q[b], SR, H_out) for b in range(B)]
    return x, want, device(x, H_out)


@pytest.mark.parametrize("shape", ref.GPU_SHAPES)
def test_kernel_matches_the_definition(shape):
    B, T, T_out, H, H_out, F = shape
    x, want, got = case(shape)
    if T >= 4 and T_out >= 5:                                    # the inputs reach every branch
        u = np.concatenate([w["u"][w["live"]].ravel() for w in want])
        assert (u < 1).any() and (u > H).any() and ((u >= 1) & (u < H)).any()
        assert any((w["ok"] & (w["va"] != w["vb"])).any() for w in want)                          # exactly one voiced neighbour
        masked = np.concatenate([w["masked"][w["live"]].ravel() for w in want])
        assert masked.any() and not masked.all()
        assert (x["pos"] > T - 1).any() and (x["pos"] < 0).any() and (x["pos"] == T - 1).any()       # the clamp, both ways
    eA = ea = eN = 0.0
    for b in range(B):
        e = compare(got, want[b], b, H_out)
        eA, ea, eN = max(eA, e[0]), max(ea, e[1]), max(eN, e[2])
    print(f"{shape}: |A' - fp64| = {eA:.3e}, |a' - fp64| = {ea:.3e}, |N' - fp64| = {eN:.3e} of the largest source value (TOL_A {TOL_A:g})")
    assert eA <= TOL_A
    assert ea <= H_out * TOL_A
    assert eN <= TOL_A


def test_identity_and_formants_that_follow_the_pitch():
    shape = B, T, _, H, _, F = (2, 16, 16, 180, 180, 195)
    x = ref.rows(shape)
    same = ddsp.transform_controls(controls(x), SR, stretch=1, transpose=0, formant=0)
    follow = ddsp.transform_controls(controls(x), SR, transpose=-9.0, formant=None)
    r = ref.ratio_of(-9.0)
    worst = 0.0
    for b in range(B):
        A = ref.source_amplitudes(x["f0"][b], x["a"][b], x["c"][b], SR)
        scale = max(A.max(), 1e-30)
        voiced = ref.voiced_of(x["f0"][b])
        got = (same["a"][b] * same["c"][b]).double().cpu().numpy() * (A.sum(-1) != 0)[:, None]
        worst = max(worst, np.abs(got - A).max() / scale)
        assert same_bits(same["f0"][b, voiced, 0].cpu().numpy(), x["f0"][b][voiced])
        assert same_bits(same["H"][b].cpu().numpy(), x["N"][b])
        # q = r: u = k', every harmonic keeps its amplitude (the lower pitch masks none of them)
        got = (follow["a"][b] * follow["c"][b]).double().cpu().numpy() * (A.sum(-1) != 0)[:, None]
        worst = max(worst, np.abs(got - A).max() / scale)
        assert same_bits(follow["f0"][b, voiced, 0].cpu().numpy(), x["f0"][b][voiced] * r)
    print(f"identity and formant=None: max |a' c' - A| = {worst:.3e} of the largest amplitude (TOL_A {TOL_A:g})")
    assert worst <= TOL_A


def test_hostile_per_frame_values_stay_inside_the_buffers():
    """Positions, ratios and pitches that are NaN, infinite, zero, negative or huge, handed to the entry point itself with a guard
    zone behind every output: each frame follows the silent-frame and clamp rules exactly, and nothing else is written."""
    B, T, H, H_out, F, GUARD, MARK = 2, 6, 8, 11, 5, 256, -7.0
    rng = np.random.default_rng(5)
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0, 1e30, -1e30, 1e35, 2.5, 5.0, 4.999, 1e-30], dtype=np.float32)
    T_out = 3 * len(bad)
    f0 = rng.uniform(300.0, 900.0, (B, T)).astype(np.float32)
    f0[:, 1], f0[:, 4], f0[:, 5] = np.nan, np.inf, -np.inf
    a, c, N = (rng.uniform(0.1, 1.0, s).astype(np.float32) for s in ((B, T), (B, T, H), (B, T, F)))
    pos = np.full((B, T_out), 2.5, dtype=np.float32)
    r, q = np.ones((B, T_out), dtype=np.float32), np.ones((B, T_out), dtype=np.float32)
    pos[:, :12], r[:, 12:24], q[:, 24:] = bad, bad, bad
    pos[1], r[1], q[1] = pos[1, ::-1], r[1, ::-1], q[1, ::-1]
    outs = [torch.full((n + GUARD,), MARK, device="cuda") for n in (B * T_out, B * T_out, B * T_out * H_out, B * T_out * F)]
    ins = [cuda(v) for v in (f0, a, c, N, pos, r, q)]
    rc = ddsp._lib.lib().ddsp_transform_controls(*(v.data_ptr() for v in ins), *(v.data_ptr() for v in outs), B, T, T_out, H, H_out, F, SR,
                                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(bool((v[-GUARD:] == MARK).all()) for v in outs)                                    # the guard zones
    shapes = ((B, T_out, 1), (B, T_out, 1), (B, T_out, H_out), (B, T_out, F))
    got = {k: v[:-GUARD].reshape(s).cpu().numpy() for k, v, s in zip(("f0", "a", "c", "H"), outs, shapes)}
    worst = 0.0
    for b in range(B):
        want = ref.transform(f0[b], a[b], c[b], N[b], pos[b], r[b], q[b], SR, H_out)
        usable = np.isfinite(bad) & (bad > 0)
        assert np.array_equal(want["ok"][12:] if b == 0 else want["ok"][:24][::-1], np.concatenate([usable, usable]))
        silent = ~want["live"]
        assert silent.sum() >= 14 and not want["ok"][silent].all() and want["ok"][silent].any()   # bad ratios, and unvoiced pairs
        assert not got["H"][b][~want["ok"]].any()
        worst = max(worst, *compare(got, want, b, H_out)[::2])
    print(f"hostile frames: the usable ones within {worst:.3e} of the definition")
    assert worst <= TOL_A


def test_more_frames_than_the_grid():
    """cap x 4 + 5 output frames: the first wavefronts walk a second frame."""
    shape = B, T, T_out, H, H_out, F = (1, 3, analysis.TRANSFORM_KERNEL_MAX_BLOCKS * analysis.TRANSFORM_KERNEL_WAVES + 5, 2, 2, 2)
    x, want, got = case(shape)
    e = compare(got, want[0], 0, H_out)
    print(f"{shape}: |A' - fp64| = {e[0]:.3e}, |a' - fp64| = {e[1]:.3e}, |N' - fp64| = {e[2]:.3e}")
    assert e[0] <= TOL_A and e[1] <= H_out * TOL_A and e[2] <= TOL_A
    assert want[0]["a"][-5:].any() and got["a"][0, -5:].any()


def test_deterministic_and_rows_independent():
    shape = B, T, T_out, H, H_out, F = ref.GPU_SHAPES[1]
    x, _, first = case(shape)
    again = device(x, H_out)
    assert all(same_bits(first[k], again[k]) for k in first)
    flipped = device({k: v[::-1] for k, v in x.items()}, H_out)
    assert all(same_bits(flipped[k][::-1], first[k]) for k in first)
    alone = device({k: v[1:2] for k, v in x.items()}, H_out)
    assert all(same_bits(alone[k][0], first[k][1]) for k in first)


def test_through_the_oscillator_bank():
    """A steady three-formant tone's controls, stretched by 2 and moved up 5 semitones with the formants kept, played by the real
    bank and analysed along f0': |C| is the definition's A' on the interior frames.  The source pitch is chosen so that the
    window holds whole periods of f0' = 312.5 Hz, as in the analysis' own round trip, whose bound this is: the bank within 1e-5
    of its definition, twice that on C, plus TOL_C, plus TOL_A for the transformation."""
    T, H, hop, W = 64, 40, 64, 256
    r = float(ref.ratio_of(5.0))
    f0, a, c = ref.formant_tone(T, H, f0=312.5 / r)
    conf = type("Conf", (), dict(n_harmonics=H, sample_rate=SR, hop_length=hop, n_fft=W))
    bank = ddsp.OscillatorBank(conf).cuda()
    ctrl = dict(f0=cuda(f0)[None, :, None], a=cuda(a)[None, :, None], c=cuda(c)[None])
    out = ddsp.transform_controls(ctrl, SR, stretch=2, transpose=5.0, formant=0.0)
    assert sorted(out) == ["a", "c", "f0"] and out["c"].shape == (1, 2 * T, H)
    y = bank(out)
    assert y.shape == (1, 2 * T * hop) and torch.isfinite(y).all()
    want = ref.transform(f0, a, c, None, ref.stretch_positions(T, 2), np.full(2 * T, r, np.float32), np.ones(2 * T, np.float32), SR, H)
    assert abs(float(want["f0"][0]) - 312.5) < 1e-4 and same_bits(out["f0"][0, :, 0].cpu().numpy(), want["f0"])
    z = ddsp.harmonic_analysis(y, out["f0"], hop, SR, H, W, return_complex=True)
    frames, _ = href.interior(2 * T, hop, W)
    err = np.abs(np.abs(z["C"][0].cpu().numpy().astype(np.complex128)) - want["A"])[frames].max()
    bound = 2e-5 + href.TOL_C + TOL_A
    audible = (~want["masked"][0]).sum()
    print(f"bank(transform(controls)): | |C| - A' | <= {err:.3e} on {len(frames)} interior frames (bound {bound:.2e}); {audible} audible harmonics")
    assert 20 <= audible < H and err <= bound
    # the formants did not move: the envelope over Hz at the new harmonics is the source's, read between its harmonics
    A = ref.source_amplitudes(f0, a, c, SR)[0]
    hz = np.arange(1, H + 1) * 312.5
    keep = (hz <= H * 312.5 / r) & ~want["masked"][0]
    moved = np.abs(want["A"][0][keep] - np.interp(hz[keep], np.arange(1, H + 1) * 312.5 / r, A)).max()
    assert moved <= 1e-12


def test_autoencoder_transform_without_weights():
    """AutoEncoder(tracker='yin').transform on a three-formant tone the bank synthesised at the autoencoder's configuration."""
    T, H, hop = 44, AEConf.n_harmonics, AEConf.hop_length
    f0, a, c = ref.formant_tone(T, H, f0=220.0)
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x = ae.decoder.harmonics(dict(f0=cuda(f0)[None, :, None], a=cuda(a)[None, :, None], c=cuda(c)[None]))
    frames = ae.analyse(x)["f0"].shape[1]
    T_out = max(1, int(np.floor(frames * 1.5 + 0.5)))
    y = ae.transform(x, stretch=1.5, transpose=3.0)
    assert y.shape == (1, T_out * hop) and torch.isfinite(y).all() and float(y.abs().max()) > 0
    wet = ae.transform(x, stretch=1.5, transpose=3.0, reverb=True)
    assert wet.shape == y.shape and torch.isfinite(wet).all()
    dry = ae.transform(x, stretch=1.5, transpose=3.0, formant=None, noise=False)
    ctrl = ddsp.transform_controls(ae.analyse(x), AEConf.sample_rate, stretch=1.5, transpose=3.0, formant=None)
    assert dry.shape == (1, T_out * hop) and torch.equal(dry, ae.decoder.harmonics(ctrl))           # the harmonics-only path, bit for bit
    pitch = ctrl["f0"][0, 4:-4, 0]
    print(f"analysed and transposed pitch: {float(pitch.min()):.2f} .. {float(pitch.max()):.2f} Hz (220 Hz + 3 semitones = {220 * 2 ** 0.25:.2f})")
    assert float((pitch / (220.0 * 2 ** 0.25) - 1).abs().max()) < 0.02
    frozen = ae.transform(x, positions=torch.full((7,), 10.0, device="cuda"), noise=False)
    assert frozen.shape == (1, 7 * hop)
    with pytest.raises(ValueError, match="overlap"):              # the noise model must be the decoder's, as in analyse
        ae.transform(x, noise='overlap_add')
    with pytest.raises(ValueError):
        ddsp.AutoEncoder(AEConf, tracker='yin', noise_overlap_add=True).cuda().eval().transform(x, noise=True)


def test_empty_batch_and_the_torch_path_on_the_device():
    x = ref.rows((2, 9, 23, 100, 100, 65))
    ctrl = controls(x)
    empty = ddsp.transform_controls({k: v[:0] for k, v in ctrl.items()}, SR, stretch=2.0)
    assert empty["c"].shape == (0, 18, 100) and empty["H"].shape == (0, 18, 65) and empty["c"].is_cuda
    # n_harmonics = 300 is beyond the kernel: the stock-op path, on the device, agrees with the kernel on the harmonics both have
    kw = dict(transpose=cuda(x["transpose"]), formant=cuda(x["formant"]), positions=cuda(x["pos"]))
    wide = ddsp.transform_controls(ctrl, SR, n_harmonics=300, **kw)
    near = ddsp.transform_controls(ctrl, SR, n_harmonics=256, **kw)
    assert wide["c"].shape == (2, 23, 300) and wide["c"].is_cuda and torch.equal(wide["f0"], near["f0"])
    A_wide, A_near = (wide["a"] * wide["c"])[..., :256].double(), (near["a"] * near["c"]).double()
    live = (near["a"] > 0)[..., 0]
    scale = float((ctrl["a"] * ctrl["c"]).max())
    err = float((A_wide - A_near)[live].abs().max()) / scale
    print(f"torch path on the device against the kernel: {err:.3e}")
    assert err <= 1e-5
