"""The inharmonic analysis on the device (csrc/ddsp_partials.hip: ddsp_partials_*) against the fp64 definition of
tests/partials_reference.py under its per-element bounds, then through the Python entry points, the real InharmonicBank,
AutoEncoder.analyse_partials and a captured graph.  Every test prints its observed maximum before it asserts."""
import functools

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import harmonic_analysis_reference as ref
import partials_reference as pr
import sinusoids_reference as sref
from encoder_common import AEConf
from sinusoids_reference import EPS

pytestmark = pytest.mark.gpu

GRID_CAP = 8192                                                  # csrc/ddsp_partials.hip: kMaxBlocks
GUARD = 64                                                       # floats behind every output, which must stay as they were
SENTINEL = -12345.0


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def guarded(n):
    return torch.full((n + GUARD,), SENTINEL, device="cuda")


def intact(buffers, sizes):
    return all(bool((b[n:] == SENTINEL).all()) for b, n in zip(buffers, sizes))


def device_analysis(audio, f, voiced, hop, sr, W, reassign=True, resynth=False):
    """Raw ddsp_partials_analysis (and, with `resynth`, ddsp_partials_resynth of its C with the prefix kept) on rows [B, N], f
    [B, T, K] (numpy fp32) -> dict of numpy arrays; the guard zones behind every output are checked here, on every call."""
    B, T, K = f.shape
    L = ddsp._lib.lib()
    a_d, f_d = dev(audio), dev(f)
    v = None if voiced is None else dev(voiced, torch.uint8)
    sizes = [2 * B * T * K, B * T, B * T * K, B * T * K]
    C, a, c, fr = (guarded(n) for n in sizes)
    ws = torch.empty(L.ddsp_partials_workspace_bytes(B, T, K, hop, W), device="cuda", dtype=torch.uint8)
    rc = L.ddsp_partials_analysis(a_d.data_ptr(), f_d.data_ptr(), None if v is None else v.data_ptr(), C.data_ptr(), a.data_ptr(),
                                  c.data_ptr(), fr.data_ptr() if reassign else None, ws.data_ptr(), B, T, K, hop, W, sr,
                                  torch.cuda.current_stream().cuda_stream)
    ddsp._lib.check(rc, "ddsp_partials_analysis")
    out = {}
    if resynth:
        harm, resid = guarded(B * T * hop), guarded(B * T * hop)
        rc = L.ddsp_partials_resynth(C.data_ptr(), f_d.data_ptr(), a_d.data_ptr(), harm.data_ptr(), resid.data_ptr(), ws.data_ptr(), B, T, K,
                                     hop, sr, ddsp.partials.PHASE_READY, torch.cuda.current_stream().cuda_stream)
        ddsp._lib.check(rc, "ddsp_partials_resynth")
        assert intact([harm, resid], [B * T * hop] * 2)
        out.update(harm=harm[:B * T * hop].reshape(B, -1).cpu().numpy(), resid=resid[:B * T * hop].reshape(B, -1).cpu().numpy())
    assert intact([C, a, c], sizes[:3]) and (intact([fr], sizes[3:]) if reassign else bool((fr == SENTINEL).all()))
    Cn = C[:sizes[0]].reshape(B, T, K, 2).cpu().numpy()
    out.update(C=Cn[..., 0].astype(np.float64) + 1j * Cn[..., 1].astype(np.float64), C32=Cn, a=a[:B * T].reshape(B, T).cpu().numpy(),
               c=c[:sizes[2]].reshape(B, T, K).cpu().numpy(), f_re=fr[:sizes[3]].reshape(B, T, K).cpu().numpy() if reassign else None)
    return out


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape, the device's outputs and the definition's, row by row: computed once."""
    B, T, hop, W, K, sr = shape
    audio, f, voiced = pr.string_rows(*shape)
    got = device_analysis(audio, f, voiced, hop, sr, W, resynth=True)
    want = [pr.analyse(audio[b], f[b], hop, sr, W, voiced[b]) for b in range(B)]
    return audio, f, voiced, got, want


def worst_ratio(err, bound):
    r = err / bound
    assert not np.isnan(r).any()
    return float(r.max())


def compare(got, want, f, rows=None):
    """Error / bound of C, a, c and f_re, row by row; the exact parts are asserted here."""
    worst = dict(C=0.0, a=0.0, c=0.0, f_re=0.0)
    held = 0
    for b in (range(len(want)) if rows is None else rows):
        w = want[b]
        live = w["bound_C"] > 0
        assert not got["C"][b][~w["keep"]].any(), b                                          # masked: exactly zero
        assert np.isfinite(got["C"][b]).all() and np.isfinite(got["a"][b]).all(), b
        if live.any():
            worst["C"] = max(worst["C"], worst_ratio(np.abs(got["C"][b] - w["C"])[live], w["bound_C"][live]))
        some = w["bound_a"] > 0
        if some.any():
            worst["a"] = max(worst["a"], worst_ratio(np.abs(got["a"][b] - w["a"])[some], w["bound_a"][some]))
        assert not got["a"][b][~some].any() and np.all(got["c"][b][~some] == np.float32(1.0 / f.shape[-1])), b
        fin = np.isfinite(w["bound_c"]) & (w["bound_c"] > 0)
        assert not got["c"][b][w["bound_c"] == 0].any(), b                                   # a masked partial of a sounding frame
        if fin.any():
            worst["c"] = max(worst["c"], worst_ratio(np.abs(got["c"][b] - w["c"])[fin], w["bound_c"][fin]))
        if got["f_re"] is not None:
            assert same_bits(got["f_re"][b][~w["measured"]], f[b][~w["measured"]]), b       # not defined: the entry's own bits
            assert w["vacuous"] == 0, b                                                      # no entry at the asserted level is left out
            fre = np.isfinite(w["bound_f"])
            held += int(fre.sum())
            if fre.any():
                worst["f_re"] = max(worst["f_re"], worst_ratio(np.abs(got["f_re"][b] - w["f_re"])[fre], w["bound_f"][fre]))
    return worst, held


@pytest.mark.parametrize("shape", pr.GPU_SHAPES)
def test_analysis_matches_the_definition(shape):
    B, T, hop, W, K, sr = shape
    audio, f, voiced, got, want = case(shape)
    worst, held = compare(got, want, f)
    print(f"{shape}: error / derived bound: C {worst['C']:.3f}, a {worst['a']:.3f}, c {worst['c']:.3f}, f_re (and D through it) "
          f"{worst['f_re']:.3f} on {held} entries")
    assert (held > 0) == bool(pr.interior_frames(T, hop, W))
    assert max(worst.values()) <= 1.0
    plain = device_analysis(audio, f, voiced, hop, sr, W, reassign=False)                    # the kernel without the second window
    assert all(same_bits(plain[k], got[k]) for k in ("C32", "a", "c"))


@pytest.mark.parametrize("shape", pr.GPU_SHAPES)
def test_resynthesis_of_the_devices_own_amplitudes(shape):
    B, T, hop, W, K, sr = shape
    audio, f, voiced, got, _ = case(shape)
    worst = 0.0
    for b in range(B):
        harm, bound = pr.resynth(got["C"][b], f[b], hop, sr)
        some = bound > 0
        assert not got["harm"][b][~some].any(), b
        if some.any():
            worst = max(worst, (np.abs(got["harm"][b] - harm)[some] / bound[some]).max())
        assert same_bits(got["resid"][b], audio[b] - got["harm"][b]), b
    print(f"{shape}: resynthesis of the device's C against fp64: error / bound {worst:.3f}")
    assert worst <= 1.0
    C = dev(got["C32"])
    alone = ddsp.partial_resynthesis(torch.view_as_complex(C), dev(f), hop, sr)              # its own prefix pass
    assert same_bits(alone.cpu().numpy(), got["harm"])


def test_more_frames_than_the_grid():
    """hop 2, W 64, K 3 over cap + 4 frames in each of two rows: the blocks walk a second frame and a second segment.  Frames
    either side of the cap are judged, and row 1 launched alone has its frames in other blocks and other turns than inside the
    batch: the same bits either way."""
    B, T, hop, W, K, sr = shape = (2, GRID_CAP + 4, 2, 64, 3, 16000)
    audio, f, voiced = pr.string_rows(*shape)
    got = device_analysis(audio, f, voiced, hop, sr, W, resynth=True)
    inter = pr.interior_frames(T, hop, W)
    frames = [0, inter[0], inter[0] + 1, T // 2, GRID_CAP - 1 - T % GRID_CAP, inter[-1] - 1, inter[-1], T - 1]
    want = [pr.analyse(audio[b], f[b], hop, sr, W, voiced[b], frames=frames) for b in range(B)]
    sub = {k: (None if v is None else v[:, frames] if v.ndim >= 2 and v.shape[1] == T else v) for k, v in got.items()}
    for w in want:
        for k in ("C", "keep", "bound_C", "a", "bound_a", "c", "bound_c", "f_re", "measured", "bound_f"):      # (`vacuous` is a count)
            w[k] = w[k][frames]
    worst, held = compare(sub, want, f[:, frames])
    print(f"frames either side of the cap: error / derived bound: {worst} on {held} entries")
    assert held > 0 and max(worst.values()) <= 1.0
    alone = device_analysis(audio[1:], f[1:], voiced[1:], hop, sr, W, resynth=True)
    assert all(same_bits(alone[k][0], got[k][1]) for k in ("C32", "a", "c", "f_re", "harm", "resid"))
    harm, bound = pr.resynth(got["C"][1], f[1], hop, sr)
    assert (np.abs(got["harm"][1] - harm) <= bound).all()


def test_deterministic_and_rows_independent():
    shape = B, T, hop, W, K, sr = pr.GPU_SHAPES[1]
    audio, f, voiced, first, _ = case(shape)
    keys = ("C32", "a", "c", "f_re", "harm", "resid")
    again = device_analysis(audio, f, voiced, hop, sr, W, resynth=True)
    assert all(same_bits(first[k], again[k]) for k in keys)
    for b in range(B):
        alone = device_analysis(audio[b:b + 1], f[b:b + 1], voiced[b:b + 1], hop, sr, W, resynth=True)
        assert all(same_bits(alone[k][0], first[k][b]) for k in keys), b
    flipped = device_analysis(audio[::-1], f[::-1], voiced[::-1], hop, sr, W, resynth=True)
    assert all(same_bits(np.ascontiguousarray(flipped[k][::-1]), first[k]) for k in keys)


def test_nan_sample_reaches_only_the_frames_that_hold_it():
    shape = B, T, hop, W, K, sr = pr.GPU_SHAPES[1]
    audio, f, voiced, first, _ = case(shape)
    at = 11 * hop + 5
    bad = audio.copy()
    bad[0, at] = np.nan
    got = device_analysis(bad, f, voiced, hop, sr, W)
    holds = np.array([ref.frame_start(t, hop, W) <= at < ref.frame_start(t, hop, W) + W for t in range(T)])
    assert holds.sum() == W // hop
    for k in ("C32", "a", "c", "f_re"):
        assert same_bits(got[k][1:], first[k][1:]) and same_bits(got[k][0, ~holds], first[k][0, ~holds]), k
    assert same_bits(got["f_re"][0, holds], f[0, holds])                                     # not measurable: the entry's own bits
    live = holds & (first["a"][0] > 0)
    assert live.any() and np.isnan(got["a"][0, live]).all()


def test_python_entries_run_the_same_kernels():
    shape = B, T, hop, W, K, sr = pr.GPU_SHAPES[1]
    audio, f, voiced, first, _ = case(shape)
    args = (dev(audio), dev(f), hop, sr, W)
    v = dev(voiced)[..., None]
    harm, resid, d = ddsp.partial_residual(*args, voiced=v, return_complex=True, reassign=True)
    assert sorted(d) == ["C", "a", "c", "f", "f_re"] and harm.is_cuda and d["C"].dtype == torch.complex64
    assert same_bits(torch.view_as_real(d["C"]).cpu().numpy(), first["C32"]) and same_bits(d["a"][..., 0].cpu().numpy(), first["a"])
    assert same_bits(d["c"].cpu().numpy(), first["c"]) and same_bits(d["f_re"].cpu().numpy(), first["f_re"])
    assert same_bits(harm.cpu().numpy(), first["harm"]) and same_bits(resid.cpu().numpy(), first["resid"])
    assert np.array_equal(d["f"].cpu().numpy(), np.where(pr.usable(f), f, np.float32(0)))
    plain = ddsp.partial_analysis(*args, voiced=v)
    assert sorted(plain) == ["a", "c", "f"] and torch.equal(plain["a"], d["a"])
    # refine_partials: each step is this launch and the frame-rate arithmetic of the definition
    one = ddsp.refine_partials(*args, voiced=v, iterations=1).cpu().numpy()
    want = ddsp.partials._carry_and_clamp(torch.from_numpy(f), torch.from_numpy(first["f_re"]), torch.from_numpy(f),
                                          torch.from_numpy(voiced)[..., None], hop, W, 50.0).numpy()
    alive = pr.usable(f) & voiced[..., None]
    assert same_bits(one[~alive], f[~alive])                                                 # dead entries come back as they are
    assert np.abs(pr.cents(one[alive], want[alive])).max() <= 1e-3                           # (fp32 arithmetic on either side)
    assert np.abs(pr.cents(one[alive], f[alive])).max() <= 50.0 + 2.1e-4


def test_outside_the_kernel_range_runs_the_torch_path_on_the_device():
    """W = 4098 and K = 257: the stock-op path in fp32 on the device against the same path on the CPU.  Both are within
    (W + 8) 2^-24 (the order of the fp32 sum and the products), 2 pi 2^-24 (the fp32 angle) and 4 2^-24 (cos / sin) of the exact sum
    per unit of (2 / norm) sum |w x|, times sqrt(2) for the modulus; they may differ by twice that."""
    B, T, hop, W, K, sr = shape = (1, 6, 1024, 4098, 257, 16000)
    audio, f, voiced = pr.string_rows(*shape)
    assert not ddsp._lib.lib().ddsp_partials_supported(K, hop, W)
    on_dev = ddsp.partial_analysis(dev(audio), dev(f), hop, sr, W, return_complex=True)
    on_cpu = ddsp.partial_analysis(torch.from_numpy(audio), torch.from_numpy(f), hop, sr, W, return_complex=True)
    w, _ = pr.windows(W)
    gain = np.zeros(T)
    for t in range(T):
        n = ref.frame_start(t, hop, W) + np.arange(W)
        inside = (n >= 0) & (n < T * hop)
        gain[t] = 2.0 * np.abs(w[inside] * audio[0][n[inside]]).sum() / w[inside].sum()
    tol = 2 * np.sqrt(2.0) * gain * ((W + 12) * EPS + 2 * np.pi * EPS)
    err = (on_dev["C"].cpu() - on_cpu["C"]).abs().numpy()[0].max(axis=-1)
    print(f"W 4098, K 257, device torch path against the CPU path: error / tolerance {(err / tol).max():.3f}")
    assert on_dev["C"].is_cuda and (err <= tol).all() and torch.equal(on_dev["C"].cpu() == 0, on_cpu["C"] == 0)


class BankConf:
    n_harmonics, sample_rate, hop_length, n_fft = 12, 16000, 64, 512


@pytest.mark.parametrize("model", ["stiff", "free"])
def test_round_trip_through_the_bank(model):
    """bank(controls) -> inharmonic_analysis -> bank(dict), all on the device.  The bank's contract holds its output within 1e-5 of
    the fp64 forward of the same dict; C is linear in the audio with a gain of at most 2 (step 4), so the device's analysis of the
    bank's output is within 2e-5 plus the C bound of the fp64 analysis of the fp64 forward, on interior frames."""
    conf, T = BankConf, 24
    K, hop, sr, W = conf.n_harmonics, conf.hop_length, conf.sample_rate, conf.n_fft
    bank = ddsp.InharmonicBank(conf, inharmonicity=2e-4).cuda()
    rng = np.random.default_rng(17)
    tt = np.arange(T) / T
    ctrl = dict(f0=dev((196.0 * 2.0 ** (tt / 12.0))[None, :, None], torch.float32), a=dev(0.4 + 0.2 * tt[None, :, None], torch.float32),
                c=dev(rng.uniform(0.3, 1.0, (1, T, K)) / np.arange(1, K + 1), torch.float32))
    with torch.no_grad():
        y = bank(ctrl)
        d = ddsp.inharmonic_analysis(y, ctrl["f0"] * 1.003, hop, sr, K, W, iterations=3, model=model)
        y2 = bank(d)
    f_d = (d["f0"] * d["ratios"]).float()
    assert torch.equal(f_d, bank.frequencies(d)) and abs(float(d["inharmonicity"][0]) / 2e-4 - 1.0) < 0.05
    fwd = sref.forward(f_d.cpu().numpy(), d["c"].cpu().numpy(), d["a"].cpu().numpy(), hop, sr)
    contract = np.abs(y2.cpu().numpy() - fwd["y"]).max()
    got = ddsp.partial_analysis(y2, f_d, hop, sr, W, return_complex=True)["C"][0].cpu().numpy().astype(np.complex128)
    want = pr.analyse(fwd["y"][0], f_d[0].cpu().numpy(), hop, sr, W)
    inter = pr.interior_frames(T, hop, W)
    ratio = (np.abs(got - want["C"])[inter] / (2e-5 + want["bound_C"][inter])).max()
    print(f"model={model}: bank(dict) within {contract:.2e} of fp64 (contract 1e-5); its analysis: error / (2e-5 + bound) {ratio:.3f}; "
          f"B {float(d['inharmonicity'][0]):.3e}")
    assert contract <= 1e-5 and ratio <= 1.0


def test_autoencoder_analyse_partials():
    """A stiff-string row and a white-noise row at 44.1 kHz through AutoEncoder(tracker='yin', synth='inharmonic'): the dict plays,
    and the phase-keeping resynthesis leaves a small share of the tone's rms and nearly all of the noise's -- each held to twice
    what the fp64 CPU path leaves (or removes) on the same clips along the same tracks."""
    rng = np.random.default_rng(41)
    hop, sr, K, W = AEConf.hop_length, AEConf.sample_rate, AEConf.n_harmonics, AEConf.n_fft
    T = 44
    L = T * hop
    f = np.tile(196.0 * pr.stretched(K, 1.5e-4), (T, 1))
    tone = sref.forward(f[None], np.tile(1.0 / np.arange(1, K + 1), (1, T, 1)), np.full((1, T, 1), 0.5), hop, sr, cast=False)["y"][0]
    x = dev(np.stack([tone, 0.3 * rng.standard_normal(L)]), torch.float32)
    ae = ddsp.AutoEncoder(AEConf, tracker='yin', synth='inharmonic').cuda().eval()
    z = ae.analyse_partials(x, noise=True, return_complex=True)
    assert sorted(z) == ["C", "H", "a", "c", "f0", "inharmonicity", "ratios"] and z["ratios"].shape == (2, T, K)
    assert all(torch.isfinite(z[k]).all() for k in ("f0", "ratios", "a", "c", "H", "inharmonicity"))
    with torch.no_grad():
        played = ae.decoder.synthesize(z)
    assert played.shape == (2, L) and torch.isfinite(played).all()
    f_d = (z["f0"] * z["ratios"]).float()
    _, resid, _ = ddsp.partial_residual(x, f_d, hop, sr, W)
    _, resid64, _ = ddsp.partial_residual(x.cpu().double(), f_d.cpu().double(), hop, sr, W)
    rms = lambda v: v.double().pow(2).mean(-1).sqrt().cpu().numpy()                                # noqa: E731
    share, share64 = rms(resid) / rms(x), rms(resid64) / rms(x)
    print(f"residual rms / clip rms (tone, noise): device {share}, fp64 CPU path {share64}; median f0 of the tone row "
          f"{float(z['f0'][0].median()):.2f} Hz, B {z['inharmonicity'].cpu().numpy()}")
    assert share[0] <= 2 * share64[0] and share[1] >= 1.0 - 2 * (1.0 - share64[1])
    assert share64[0] < 0.5 < share64[1]                                                    # a tone is explained, noise is not
    bank = ae.decoder.harmonics
    bank.init_from(z)
    assert torch.isfinite(bank.detune_cents).all() and abs(float(bank.inharmonicity.detach()) - float(z["inharmonicity"].mean())) < 1e-9


def test_the_loops_capture_into_a_graph():
    shape = B, T, hop, W, K, sr = pr.GPU_SHAPES[0]
    audio, f, voiced, _, _ = case(shape)
    a_d, f_d, v = dev(audio), dev(f), dev(voiced)[..., None]
    f0 = torch.where(torch.isfinite(f_d[..., :1]), f_d[..., :1], torch.zeros((), device="cuda"))

    def work():
        d = ddsp.inharmonic_analysis(a_d, f0, hop, sr, K, W, voiced=v, iterations=2, return_complex=True)
        return ddsp.refine_partials(a_d, f_d, hop, sr, W, voiced=v, iterations=2), d["f0"], d["ratios"], d["a"], d["c"], d["inharmonicity"]

    with torch.no_grad():
        eager = [t.clone() for t in work()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            work()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = work()
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for got, want in zip(out, eager):
                assert same_bits(got.float().cpu().numpy(), want.float().cpu().numpy())


def test_more_rows_and_partials_than_the_prefix_grid():
    """B K above 8192 blocks of 256 threads: the prefix strides.  The last row (the pairs of the second turn) inside the batch and
    launched alone give the same bits, and it is judged against the definition."""
    B, T, hop, W, K, sr = GRID_CAP + 2, 3, 4, 8, 256, 16000
    rng = np.random.default_rng(7)
    audio = rng.uniform(-1.0, 1.0, (B, T * hop)).astype(np.float32)
    f = rng.uniform(20.0, 7900.0, (B, T, K)).astype(np.float32)
    assert B * K > GRID_CAP * 256
    got = device_analysis(audio, f, None, hop, sr, W, resynth=True)
    alone = device_analysis(audio[-1:], f[-1:], None, hop, sr, W, resynth=True)
    assert all(same_bits(alone[k][0], got[k][-1]) for k in ("C32", "a", "c", "f_re", "harm", "resid"))
    want = pr.analyse(audio[-1], f[-1], hop, sr, W)
    ratio = worst_ratio(np.abs(got["C"][-1] - want["C"]), want["bound_C"])
    print(f"the last of {B} rows of {K} partials: C error / bound {ratio:.3f}")
    assert ratio <= 1.0
