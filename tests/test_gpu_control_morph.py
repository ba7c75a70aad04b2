"""The control morph on the device (csrc/ddsp_morph.hip) against the fp64 definition of tests/control_morph_reference.py, against
the transformation's kernel at the weights 0 and 1, through the real oscillator bank, and through AutoEncoder.morph.  TOL_M is
derived in tests/test_control_morph_host.py; every test prints its observed maximum before it asserts.  The definition is
evaluated at the device's own f0' (which is held to one ulp of the definition's, and to its bits wherever it is selected)."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import control_morph_reference as ref
import harmonic_analysis_reference as href
from ddsp_pytorch_amd import analysis
from encoder_common import AEConf

pytestmark = pytest.mark.gpu

TOL_M = ref.TOL_M
SR = ref.SAMPLE_RATE
CASES = [(shape, coordinates) for shape in ref.GPU_SHAPES for coordinates in ref.COORDINATES]
FORMANTS_A = ((600.0, 150.0, 1.0), (1400.0, 200.0, 0.6), (2800.0, 300.0, 0.4))
FORMANTS_B = ((750.0, 150.0, 1.0), (1700.0, 200.0, 0.6), (3300.0, 300.0, 0.4))


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def controls(s, noise=True):
    out = dict(f0=cuda(s["f0"])[..., None], a=cuda(s["a"])[..., None], c=cuda(s["c"]))
    if noise:
        out["H"] = cuda(s["N"])
    return out


def device(x, H_out, coordinates):
    out = ddsp.morph_controls(controls(x["a"]), controls(x["b"]), SR, mix_f0=cuda(x["wf"]), mix_harmonics=cuda(x["wh"]),
                              mix_noise=cuda(x["wn"]), coordinates=coordinates, positions_a=cuda(x["a"]["pos"]),
                              positions_b=cuda(x["b"]["pos"]), n_harmonics=H_out)
    assert all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def ulps(x, y):
    return np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))


def compare(got, want, b, H_out):
    """One row of the device's answer against the definition at the device's f0' -> (error of A', of a', of N', each over its
    scale, and the distance of f0' from the definition's own in ulps); the exact parts are asserted here."""
    f0, a, c, N = got["f0"][b, :, 0], got["a"][b, :, 0], got["c"][b], got["H"][b]
    assert np.isfinite(f0).all() and np.isfinite(a).all() and np.isfinite(c).all() and np.isfinite(N).all(), b
    off = ulps(f0, want["f0_definition"])
    assert not off[want["selected"]].any(), b                                                      # the same bits where f0' is selected
    assert off.max() <= 1, b
    quiet = want["a"] == 0
    assert not a[quiet].any() and (c[quiet] == np.float32(1) / np.float32(H_out)).all(), b         # the fill, exactly
    assert np.array_equal(c[~quiet] == 0, want["A"][~quiet] == 0) and (a[~quiet] > 0).all(), b     # the zero pattern, exactly
    assert np.array_equal(N == 0, want["N"] == 0), b
    silent = ~want["sane"]
    assert not f0[silent].any() and not a[silent].any() and not N[silent].any(), b
    A = a.astype(np.float64)[:, None] * c.astype(np.float64) * ~quiet[:, None]
    scale, nscale = np.maximum(want["scale"], 1e-30), np.maximum(want["nscale"], 1e-30)
    return ((np.abs(A - want["A"]) / scale[:, None]).max(), (np.abs(a - want["a"]) / scale).max(),
            (np.abs(N - want["N"]) / nscale[:, None]).max(), int(off.max()))


@functools.lru_cache(maxsize=None)
def case(shape, coordinates):
    """The inputs of one shape, the device's answer and the definition's per row at the device's f0': computed once, shared, not
    modified."""
    B, H_out = shape[0], shape[6]
    x = ref.rows(shape)
    got = device(x, H_out, coordinates)
    want = [ref.morph(*ref.row_of(x, b), SR, H_out, coordinates, f0=got["f0"][b, :, 0]) for b in range(B)]
    return x, want, got


@pytest.mark.parametrize("shape,coordinates", CASES)
def test_kernel_matches_the_definition(shape, coordinates):
    B, H_out = shape[0], shape[6]
    x, want, got = case(shape, coordinates)
    eA = ea = eN = off = 0
    for b in range(B):
        e = compare(got, want[b], b, H_out)
        eA, ea, eN, off = max(eA, e[0]), max(ea, e[1]), max(eN, e[2]), max(off, e[3])
    print(f"{shape} {coordinates}: |A' - fp64| = {eA:.3e}, |a' - fp64| = {ea:.3e}, |N' - fp64| = {eN:.3e} of the largest source value "
          f"(TOL_M {TOL_M:g}); f0' within {off} ulp")
    assert eA <= TOL_M
    assert ea <= H_out * TOL_M
    assert eN <= TOL_M


def test_the_inputs_reach_every_branch():
    reached, margin = {}, np.inf
    for shape, coordinates in CASES:
        x, want, got = case(shape, coordinates)
        for b, w in enumerate(want):
            margin = min(margin, ref.nyquist_margin(w["f0_definition"], SR, shape[6]))
            for key, value in ref.branches(w, ref.row_of(x, b)).items():
                reached[key] = reached.get(key, 0) + value
    print(f"branches {reached}; fl32(k' f0') at least {margin:.1f} ulp from Nyquist")
    assert all(reached.values()) and margin >= 4


@pytest.mark.parametrize("coordinates", ref.COORDINATES)
def test_mix_0_and_1_are_the_transformation_bit_for_bit(coordinates):
    """a', c' and the bands on every frame, f0' on every frame where the selected sound is present (where it is absent and the
    other present, f0' is the other's pitch, at amplitude 0)."""
    frames = 0
    for shape in (ref.GPU_SHAPES[2], ref.GPU_SHAPES[3], ref.GPU_SHAPES[5]):
        B, H_out = shape[0], shape[6]
        x = ref.rows(shape)
        pos = {k: cuda(x[k]["pos"]) for k in "ab"}
        for mix, key in ((0.0, "a"), (1.0, "b")):
            out = ddsp.morph_controls(controls(x["a"]), controls(x["b"]), SR, mix=mix, coordinates=coordinates, positions_a=pos["a"],
                                      positions_b=pos["b"], n_harmonics=H_out)
            want = ddsp.transform_controls(controls(x[key]), SR, positions=pos[key], n_harmonics=H_out)
            for k in ("a", "c", "H"):
                assert same_bits(out[k].cpu().numpy(), want[k].cpu().numpy()), (shape, mix, k)
            present = np.stack([ref.source_map(x[key]["f0"][b], x[key]["pos"][b])["present"] for b in range(B)])
            assert same_bits(out["f0"].cpu().numpy()[present], want["f0"].cpu().numpy()[present]) and float(want["a"].max()) > 0
            assert not out["a"].cpu().numpy()[~present].any()
            frames += int(present.sum())
    print(f"mix = 0 and mix = 1 in '{coordinates}' coordinates: the transformation's bits on {frames} frames")


def test_hostile_per_frame_values_stay_inside_the_buffers():
    """Weights, positions and pitches that are NaN, infinite or huge, handed to the entry point itself with a guard zone behind
    every output: each frame follows the silent-frame, clamp and presence rules exactly, and nothing else is written."""
    B, T_a, T_b, H_a, H_b, H_out, F, GUARD, MARK = 2, 6, 5, 8, 13, 11, 5, 256, -7.0
    rng = np.random.default_rng(5)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e35, -3.0, 0.0, 2.5, 4.0, 3.999, 1e-30], dtype=np.float32)
    n = len(bad)
    T_out = 5 * n
    sounds = []
    for T, H in ((T_a, H_a), (T_b, H_b)):
        f0 = rng.uniform(300.0, 900.0, (B, T)).astype(np.float32)
        sounds.append(dict(f0=f0, a=rng.uniform(0.1, 1.0, (B, T)).astype(np.float32), c=rng.uniform(0.1, 1.0, (B, T, H)).astype(np.float32),
                           N=rng.uniform(0.1, 1.0, (B, T, F)).astype(np.float32)))
    sounds[0]["f0"][:, 1], sounds[0]["f0"][:, 4], sounds[0]["f0"][:, 5] = np.nan, np.inf, -np.inf
    sounds[1]["f0"][:, 2], sounds[1]["f0"][:, 3] = 1e30, np.nan
    cols = np.full((5, B, T_out), 0.5, dtype=np.float32)         # w_f, w_h, w_n, pos_a, pos_b: each hostile in turn
    cols[3], cols[4] = 2.5, 0.5
    for i in range(5):
        cols[i, :, i * n:(i + 1) * n] = bad
    cols[:, 1] = cols[:, 1, ::-1]
    sounds[0]["pos"], sounds[1]["pos"] = cols[3], cols[4]
    outs = [torch.full((m + GUARD,), MARK, device="cuda") for m in (B * T_out, B * T_out, B * T_out * H_out, B * T_out * F)]
    ins = [cuda(s[k]) for s in sounds for k in ("f0", "a", "c", "N", "pos")] + [cuda(cols[i]) for i in range(3)]
    for coordinates in ref.COORDINATES:
        rc = ddsp._lib.lib().ddsp_morph_controls(*(v.data_ptr() for v in ins), *(v.data_ptr() for v in outs), B, T_a, T_b, T_out, H_a, H_b,
                                                 H_out, F, SR, analysis.MORPH_COORDINATES[coordinates], torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert all(bool((v[-GUARD:] == MARK).all()) for v in outs)                                # the guard zones
        shapes = ((B, T_out, 1), (B, T_out, 1), (B, T_out, H_out), (B, T_out, F))
        got = {k: v[:-GUARD].reshape(s).cpu().numpy() for k, v, s in zip(("f0", "a", "c", "H"), outs, shapes)}
        worst = 0.0
        for b in range(B):
            xa, xb = ({k: v[b] for k, v in s.items()} for s in sounds)
            want = ref.morph(xa, xb, cols[0, b], cols[1, b], cols[2, b], SR, H_out, coordinates, f0=got["f0"][b, :, 0])
            silent = ~want["sane"]
            assert silent.sum() == 9 and (got["c"][b][silent] == np.float32(1) / np.float32(H_out)).all()
            assert (want["a"] > 0).sum() >= 30 and (want["pa"] != want["pb"]).any()
            worst = max(worst, *compare(got, want, b, H_out)[:3:2])
        print(f"hostile frames, '{coordinates}': the usable ones within {worst:.3e} of the definition")
        assert worst <= TOL_M


def test_more_frames_than_the_grid():
    """cap x 4 + 5 output frames: the first wavefronts walk a second frame."""
    shape = ref.GRID_SHAPE
    H_out = shape[6]
    assert shape[3] == analysis.MORPH_KERNEL_MAX_BLOCKS * analysis.MORPH_KERNEL_WAVES + 5
    x, want, got = case(shape, "hz")
    e = compare(got, want[0], 0, H_out)
    print(f"{shape}: |A' - fp64| = {e[0]:.3e}, |a' - fp64| = {e[1]:.3e}, |N' - fp64| = {e[2]:.3e}; f0' within {e[3]} ulp")
    assert e[0] <= TOL_M and e[1] <= H_out * TOL_M and e[2] <= TOL_M
    assert want[0]["a"][-5:].any() and got["a"][0, -5:].any()


def test_deterministic_and_rows_independent():
    shape = ref.GPU_SHAPES[1]
    H_out = shape[6]
    for coordinates in ref.COORDINATES:
        x, _, first = case(shape, coordinates)
        again = device(x, H_out, coordinates)
        assert all(same_bits(first[k], again[k]) for k in first)
        part = lambda cut: {k: ({n: v[cut] for n, v in x[k].items()} if k in "ab" else x[k][cut]) for k in x}    # noqa: E731
        flipped = device(part(slice(None, None, -1)), H_out, coordinates)
        assert all(same_bits(flipped[k][::-1], first[k]) for k in first)
        alone = device(part(slice(1, 2)), H_out, coordinates)
        assert all(same_bits(alone[k][0], first[k][1]) for k in first)


def formant_pair(T_a, T_b, H, f0_out=312.5, semitones=7.0):
    """Two steady three-formant tones `semitones` apart whose geometric mean is f0_out."""
    r = 2.0 ** (semitones / 24.0)
    return [dict(zip(("f0", "a", "c"), ref.formant_tone(T, H, f0, formants)))
            for T, f0, formants in ((T_a, f0_out / r, FORMANTS_A), (T_b, f0_out * r, FORMANTS_B))]


def test_through_the_oscillator_bank():
    """Two steady three-formant tones a fifth apart, morphed halfway in 'hz' coordinates, played by the real bank and analysed
    along f0': |C| is the definition's A' on the interior frames.  The pitches are chosen so that the window holds whole periods
    of f0' = 312.5 Hz, as in the analysis' own round trip, whose bound this is: the bank within 1e-5 of its definition, twice
    that on C, plus TOL_C, plus TOL_M for the morph.  Each formant of the result, of the device's a' c' and of the analysed |C| alike,
    peaks between the two sounds' formants in Hz."""
    T_a, T_b, H, hop, W = 64, 50, 40, 64, 256
    xa, xb = formant_pair(T_a, T_b, H)
    conf = type("Conf", (), dict(n_harmonics=H, sample_rate=SR, hop_length=hop, n_fft=W))
    bank = ddsp.OscillatorBank(conf).cuda()
    ctrl = [dict(f0=cuda(s["f0"])[None, :, None], a=cuda(s["a"])[None, :, None], c=cuda(s["c"])[None]) for s in (xa, xb)]
    out = ddsp.morph_controls(*ctrl, SR, mix=0.5, coordinates="hz")
    assert sorted(out) == ["a", "c", "f0"] and out["c"].shape == (1, T_a, H)
    y = bank(out)
    assert y.shape == (1, T_a * hop) and torch.isfinite(y).all()
    f0 = out["f0"][0, :, 0].cpu().numpy()
    half = np.full(T_a, 0.5, np.float32)
    want = ref.morph(dict(xa, pos=ref.linear_positions(T_a, T_a)), dict(xb, pos=ref.linear_positions(T_b, T_a)), half, half, half, SR, H, "hz", f0=f0)
    assert abs(float(f0[0]) - 312.5) < 1e-4 and ulps(f0, want["f0_definition"]).max() <= 1
    z = ddsp.harmonic_analysis(y, out["f0"], hop, SR, H, W, return_complex=True)
    frames, _ = href.interior(T_a, hop, W)
    err = np.abs(np.abs(z["C"][0].cpu().numpy().astype(np.complex128)) - want["A"])[frames].max()
    bound = 2e-5 + href.TOL_C + TOL_M
    audible = (~want["masked"][0]).sum()
    print(f"bank(morph(controls)): | |C| - A' | <= {err:.3e} on {len(frames)} interior frames (bound {bound:.2e}); {audible} audible harmonics")
    assert 20 <= audible < H and err <= bound
    # the formants of the result, read off what the device returned (a' c') and off what the analysis heard (|C|), on every
    # interior frame: the local maxima over the audible harmonics that stand above a twentieth of the largest (the tones' formant
    # gains are 1, 0.6 and 0.4 over a floor of 1e-3, so a formant is well above that and the floor's ripple well below)
    hz = np.arange(1, audible + 1) * 312.5
    device_A = (out["a"][0] * out["c"][0]).double().cpu().numpy()
    heard = np.abs(z["C"][0].cpu().numpy().astype(np.complex128))
    for name, result in (("a' c'", device_A), ("|C|", heard)):
        for t in frames:
            env = result[t][:audible]
            top = (env[1:-1] > env[:-2]) & (env[1:-1] >= env[2:]) & (env[1:-1] > env.max() / 20)
            peaks = hz[1:-1][top]
            assert len(peaks) == 3, (name, t, peaks)
            for peak, fa, fb in zip(peaks, FORMANTS_A, FORMANTS_B):
                assert fa[0] <= peak <= fb[0], (name, t, peaks)
        print(f"formant peaks of {name} at {peaks} Hz; the sources' at {[f[0] for f in FORMANTS_A]} and {[f[0] for f in FORMANTS_B]}")


def test_autoencoder_morph_without_weights():
    """AutoEncoder(tracker='yin').morph on two tones of different lengths the bank synthesised at the autoencoder's configuration."""
    H, hop = AEConf.n_harmonics, AEConf.hop_length
    xa, xb = formant_pair(44, 60, H, f0_out=270.0)
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x, y = (ae.decoder.harmonics(dict(f0=cuda(s["f0"])[None, :, None], a=cuda(s["a"])[None, :, None], c=cuda(s["c"])[None])) for s in (xa, xb))
    assert x.shape[1] != y.shape[1]
    T_out = ae.analyse(x)["f0"].shape[1]
    out = ae.morph(x, y)
    assert out.shape == (1, T_out * hop) and torch.isfinite(out).all() and float(out.abs().max()) > 0
    wet = ae.morph(x, y, mix=0.3, reverb=True, frames=50)
    assert wet.shape == (1, 50 * hop) and torch.isfinite(wet).all()
    ramp = torch.linspace(0.0, 1.0, T_out, device="cuda")
    dry = ae.morph(x, y, mix=ramp, coordinates='harmonic', noise=False)
    ctrl = ddsp.morph_controls(ae.analyse(x), ae.analyse(y), AEConf.sample_rate, mix=ramp, coordinates='harmonic')
    assert dry.shape == (1, T_out * hop) and torch.equal(dry, ae.decoder.harmonics(ctrl))          # the harmonics-only path, bit for bit
    pitch = ae.analyse(ae.morph(x, y, noise=False))["f0"][0, 4:-4, 0]
    lo, hi = float(xa["f0"][0]), float(xb["f0"][0])
    print(f"YIN on the morph of {lo:.2f} Hz and {hi:.2f} Hz: {float(pitch.min()):.2f} .. {float(pitch.max()):.2f} Hz (halfway in pitch: 270 Hz)")
    assert lo < float(pitch.min()) and float(pitch.max()) < hi and float((pitch / 270.0 - 1).abs().max()) < 0.02
    with pytest.raises(ValueError, match="overlap"):              # the noise model must be the decoder's, as in analyse
        ae.morph(x, y, noise='overlap_add')
    with pytest.raises(ValueError):
        ddsp.AutoEncoder(AEConf, tracker='yin', noise_overlap_add=True).cuda().eval().morph(x, y, noise=True)


def test_empty_batch_and_the_torch_path_on_the_device():
    shape = ref.GPU_SHAPES[2]
    x = ref.rows(shape)
    ctrl_a, ctrl_b = controls(x["a"]), controls(x["b"])
    empty = ddsp.morph_controls({k: v[:0] for k, v in ctrl_a.items()}, {k: v[:0] for k, v in ctrl_b.items()}, SR, frames=18)
    assert empty["c"].shape == (0, 18, 100) and empty["H"].shape == (0, 18, 65) and empty["c"].is_cuda
    # n_harmonics = 300 is beyond the kernel: the stock-op path, on the device, agrees with the kernel on the harmonics both have
    kw = dict(mix_f0=cuda(x["wf"]), mix_harmonics=cuda(x["wh"]), mix_noise=cuda(x["wn"]), positions_a=cuda(x["a"]["pos"]),
              positions_b=cuda(x["b"]["pos"]))
    for coordinates in ref.COORDINATES:
        wide = ddsp.morph_controls(ctrl_a, ctrl_b, SR, n_harmonics=300, coordinates=coordinates, **kw)
        near = ddsp.morph_controls(ctrl_a, ctrl_b, SR, n_harmonics=256, coordinates=coordinates, **kw)
        assert wide["c"].shape == (2, 23, 300) and wide["c"].is_cuda
        off = ulps(wide["f0"].cpu().numpy(), near["f0"].cpu().numpy()).max()
        A_wide, A_near = (wide["a"] * wide["c"])[..., :256].double(), (near["a"] * near["c"]).double()
        live = ((near["a"] > 0) & (wide["f0"] == near["f0"]))[..., 0]            # (one ulp in f0' moves u: compared where it is the same)
        scale = float(max((ctrl_a["a"] * ctrl_a["c"]).max(), (ctrl_b["a"] * ctrl_b["c"]).max()))
        err = float((A_wide - A_near)[live].abs().max()) / scale
        noise = float((wide["H"] - near["H"]).abs().max())
        print(f"torch path on the device against the kernel, '{coordinates}': A' {err:.3e}, N' {noise:.3e}; f0' within {off} ulp on {int(live.sum())} frames")
        assert err <= 1e-5 and noise <= 1e-6 and off <= 1 and int(live.sum()) >= 20
