"""The inharmonic sinusoid bank's kernels (csrc/ddsp_sinusoids.hip) against tests/sinusoids_reference.py, element by element within
the counted bounds, under the planner's own lengths and under those forced through ddsp_sinusoids_set_form.  The inputs are
tests/sinusoids_cases.py's, whose bounds tests/test_sinusoids_host.py holds against the tightness cap."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import sinusoids_cases as cases
import sinusoids_reference as ref

pytestmark = pytest.mark.gpu

SR = cases.SR
GUARD, SENTINEL = 64, -12345.0
# ddsp_sinusoids_set_form words: the planner's lengths; chunks of 2 segments walked 1 at a time; chunks of 3 walked 2 at a time
# with 64-record tiles in the backward
FORMS = {"planned": 0, "chunk2_iter1": (2 << 8) | (1 << 16), "chunk3_iter2_tile64": (3 << 8) | (2 << 16) | (1 << 24)}


@pytest.fixture(autouse=True)
def _default_hooks():
    yield
    L = ddsp._lib.lib()
    assert L.ddsp_sinusoids_set_form(0) == 0 and L.ddsp_sinusoids_set_grid(0) == 0


def set_form(form):
    assert ddsp._lib.lib().ddsp_sinusoids_set_form(FORMS[form]) == 0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def guarded(n, dtype=torch.float32):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def raw_forward(case, phase=None):
    """ddsp_sinusoids_forward into a buffer with guard zones -> y [B, T hop] (numpy)"""
    B, T, K, hop = case["shape"]
    f, c, a = dev(case["f"]), dev(case["c"]), dev(case["a"])
    buf, y = guarded(B * T * hop)
    rc = ddsp._lib.lib().ddsp_sinusoids_forward(f.data_ptr(), c.data_ptr(), a.data_ptr(), y.data_ptr(), None,
                                                None if phase is None else phase.data_ptr(), B, T, K, hop, SR, int(case["normalize"]), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return y.cpu().numpy().reshape(B, T * hop)


def raw_backward(case, gy, want_grad_f=True, phase=None):
    """-> (grad_f or the untouched guarded buffer's content, grad_c, grad_a) as numpy"""
    B, T, K, hop = case["shape"]
    lib = ddsp._lib.lib()
    f, c, a, g = dev(case["f"]), dev(case["c"]), dev(case["a"]), dev(gy.astype(np.float32))
    (bf, gf), (bc, gc), (ba, ga) = guarded(B * T * K), guarded(B * T * K), guarded(B * T)
    scratch = torch.empty(lib.ddsp_sinusoids_backward_scratch_bytes(B, T, K, hop, int(want_grad_f)), device="cuda", dtype=torch.uint8)
    rc = lib.ddsp_sinusoids_backward(g.data_ptr(), f.data_ptr(), c.data_ptr(), a.data_ptr(), scratch.data_ptr(),
                                     gf.data_ptr() if want_grad_f else None, gc.data_ptr(), ga.data_ptr(),
                                     None if phase is None else phase.data_ptr(), B, T, K, hop, SR, int(case["normalize"]), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(bf) and guards_intact(bc) and guards_intact(ba)
    return gf.cpu().numpy().reshape(B, T, K), gc.cpu().numpy().reshape(B, T, K), ga.cpu().numpy().reshape(B, T, 1)


def check_forward(case, y, P0=None, part="bound"):
    want = ref.forward(case["f"], case["c"], case["a"], case["shape"][3], SR, P0, case["normalize"])
    err = np.abs(y.astype(np.float64) - want["y"])
    worst = float((err / np.maximum(want[part], 1e-300)).max()) if (want[part] > 0).any() else float(err.max() > 0)
    print(f"forward {case['shape']} {case['track']} normalize={case['normalize']}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.isfinite(y).all() and (err <= want[part]).all(), worst
    return want


def check_backward(case, gy, got, P0=None, names=("f", "c", "a")):
    want = ref.backward(gy, case["f"], case["c"], case["a"], case["shape"][3], SR, P0, case["normalize"])
    for name, g in zip(("f", "c", "a"), got):
        if name not in names:
            continue
        err = np.abs(g.astype(np.float64) - want["grad_" + name])
        bound = want["bound_" + name]
        worst = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else float(err.max() > 0)
        print(f"grad_{name} {case['shape']} {case['track']} normalize={case['normalize']}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
        assert np.isfinite(g).all() and (err <= bound).all(), (name, worst)
    return want


FORWARD_CASES = cases.forward_cases()


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_forward_against_fp64(shape):
    for case in FORWARD_CASES:
        if case["shape"] != shape:
            continue
        y = raw_forward(case)
        check_forward(case, y)
        if case["track"] == "silent":                            # finite (checked) and silent where both bracketing frames are
            B, T, K, hop = shape
            i0, i1, _, _ = ref.upsample_plan(T, hop)
            dead = [t for t in range(T) if t == T // 2 or (T >= 3 and t == T - 1)]
            both = np.isin(i0, dead) & np.isin(i1, dead)
            assert (y[:, both] == 0.0).all()


def test_exact_values_of_a_quarter_rate_partial():
    """f = sample_rate / 4: the phase is (n + 1) / 4 turns exactly, the sine 1, 0, -1, 0; only the bound's fp32 part is allowed."""
    for hop, T in ((8, 5), (7, 4), (128, 3)):
        case = dict(shape=(1, T, 1, hop), track="quarter", normalize=True, f=np.full((1, T, 1), SR / 4, np.float32),
                    c=np.full((1, T, 1), 0.7, np.float32), a=np.full((1, T, 1), 0.75, np.float32))
        y = raw_forward(case)
        check_forward(case, y, part="bound_fp32")
        if hop != 7:                                             # (dyadic upsampling weights: up(a) is 0.75 to the bit)
            assert np.array_equal(y[0], 0.75 * np.tile(np.array([1.0, 0.0, -1.0, 0.0], np.float32), T * hop // 4 + 1)[:T * hop])


def test_an_invalid_entry_silences_itself_and_nothing_else():
    case = cases.make_case((2, 9, 33, 64), "random", 900)
    f, c = case["f"].copy(), case["c"].copy()
    bad_frames = {1: np.nan, 3: np.inf, 4: -np.inf, 6: -100.0, 8: np.nan}
    clean_f, clean_c = f.copy(), c.copy()
    for t, v in bad_frames.items():
        f[:, t, 5] = v
        clean_f[:, t, 5] = 0.0
        clean_c[:, t, 5] = 0.0
    for normalize in (True, False):
        y_bad = raw_forward(dict(case, f=f, normalize=normalize))
        y_clean = raw_forward(dict(case, f=clean_f, c=clean_c, normalize=normalize))
        assert np.isfinite(y_bad).all() and np.array_equal(y_bad, y_clean)
        check_forward(dict(case, f=f, normalize=normalize), y_bad)


def test_large_phase_stays_inside_the_bound():
    case = cases.large_phase_case()
    want = check_forward(case, raw_forward(case))
    assert want["P"].max() > 3.0e4


@pytest.mark.parametrize("form", FORMS)
def test_forms_and_grid_stride(form):
    """More units than workgroups (two), and every length the planner decides forced: forward and backward within their bounds, and
    the forward's bits those of the planned launch."""
    assert ddsp._lib.lib().ddsp_sinusoids_set_grid(2) == 0
    for shape, track in (((2, 9, 33, 64), "octaves"), ((2, 3, 5, 7), "octaves"), ((3, 7, 4, 2), "random"), ((1, 3, 2, 1024), "octaves")):
        case = cases.make_case(shape, track, 910)
        B, T, K, hop = shape
        gy = np.random.default_rng(911).standard_normal((B, T * hop))
        set_form("planned")
        planned = raw_forward(case)
        set_form(form)
        y = raw_forward(case)
        assert np.array_equal(y, planned)
        check_forward(case, y)
        check_backward(case, gy, raw_backward(case, gy))


def test_two_calls_give_the_same_bits():
    case = cases.make_case((2, 9, 33, 64), "octaves", 920)
    gy = np.random.default_rng(921).standard_normal((2, 9 * 64))
    y, g = raw_forward(case), raw_backward(case, gy)
    for _ in range(2):
        assert np.array_equal(y, raw_forward(case))
        again = raw_backward(case, gy)
        assert all(np.array_equal(u, v) for u, v in zip(g, again))           # grad_f too: the backward has no atomics


class LiveConf:
    n_harmonics, sample_rate, hop_length = 5, SR, 16


def live_blocks(n, B=3, T=4):
    """blocks whose tracks reach the module as x['ratios'] beside f0 = 1 Hz: f exactly as built"""
    return [cases.make_case((B, T, 5, 16), "octaves", 930 + i) for i in range(n)]


def test_live_carries_a_phase_per_row_and_partial():
    bank = ddsp.InharmonicBank(LiveConf).cuda()
    blocks = live_blocks(3)
    P0 = None
    for blk in blocks:
        x = {"f0": torch.ones(3, 4, 1, device="cuda"), "ratios": dev(blk["f"]), "c": dev(blk["c"]), "a": dev(blk["a"])}
        with torch.no_grad():
            y = bank.live(x).cpu().numpy()
        want = check_forward(blk, y, P0)
        P0 = want["end"]
        state = bank.phase.cpu().numpy()
        d = np.abs(state - P0)
        assert state.shape == (3, 5) and (np.minimum(d, 1.0 - d) <= want["E_end"]).all(), (state, P0)
    assert len(set(np.round(state.reshape(-1), 6))) == 15                    # (every row and partial carries its own phase)
    bank.reset_phase()
    assert float(bank.phase.abs().max()) == 0.0


def test_live_under_graph_replay_equals_eager_blocks():
    bank = ddsp.InharmonicBank(LiveConf).cuda()
    blk = live_blocks(1, B=2)[0]
    x = {"f0": torch.ones(2, 4, 1, device="cuda"), "ratios": dev(blk["f"]), "c": dev(blk["c"]), "a": dev(blk["a"])}
    with torch.no_grad():
        eager = [bank.live(x).clone() for _ in range(3)]
        bank.reset_phase()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bank.live(x)
        torch.cuda.current_stream().wait_stream(side)
        bank.reset_phase()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = bank.live(x)
        bank.reset_phase()
        for want in eager:
            graph.replay()
            assert torch.equal(out, want)
    assert not torch.equal(eager[0], eager[1])


BACKWARD_CASES = cases.backward_cases()


@pytest.mark.parametrize("shape", cases.SHAPES[:5])
def test_backward_against_fp64(shape):
    for case, gy, bad in BACKWARD_CASES:
        if case["shape"] != shape:
            continue
        got = raw_backward(case, gy)
        want = check_backward(case, gy, got)
        if bad is not None:                                      # no gradient of its own at an invalid entry, one at a masked entry
            assert (got[0][bad] == 0.0).all() and (got[1][bad] == 0.0).all()
            masked = ~bad & (case["f"] > SR // 2)
            assert (got[1][masked] == 0.0).all()
            if shape == (2, 9, 33, 64):                          # (a masked entry still moves the phases behind it)
                assert masked.any() and np.abs(want["grad_f"][masked]).max() > 0.0 and np.abs(got[0][masked]).max() > 0.0
        B, T, K, hop = shape
        one = np.zeros((B, T * hop))                             # one sample: every target can be read off
        one[B - 1, (T * hop) // 2] = 1.5
        check_backward(case, one, raw_backward(case, one))


def test_backward_from_a_start_phase():
    case = cases.make_case((2, 3, 5, 7), "octaves", 940)
    rng = np.random.default_rng(941)
    P0 = rng.uniform(0.0, 1.0, (2, 5))
    gy = rng.standard_normal((2, 21))
    phase = dev(P0)
    check_backward(case, gy, raw_backward(case, gy, phase=phase), P0)
    assert np.array_equal(phase.cpu().numpy(), P0)                           # read only


def test_without_grad_f_the_buffer_is_untouched():
    case = cases.make_case((2, 9, 33, 64), "random", 950)
    gy = np.random.default_rng(951).standard_normal((2, 9 * 64))
    gf, gc, ga = raw_backward(case, gy, want_grad_f=False)
    assert (gf == SENTINEL).all()
    full = raw_backward(case, gy)
    assert np.array_equal(gc, full[1]) and np.array_equal(ga, full[2])
    check_backward(case, gy, (gf, gc, ga), names=("c", "a"))


def test_autograd_function_matches_the_raw_backward():
    shape = (2, 9, 33, 64)
    case = cases.make_case(shape, "octaves", 960)
    gy = np.random.default_rng(961).standard_normal((2, 9 * 64))
    f, c, a = dev(case["f"]).requires_grad_(), dev(case["c"]).requires_grad_(), dev(case["a"]).requires_grad_()
    y = ddsp.sinusoids._SinusoidsFunction.apply(f, c, a, 64, SR, True)
    y.backward(dev(gy.astype(np.float32)))
    raw = raw_backward(case, gy)
    for got, want in zip((f.grad, c.grad, a.grad), raw):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(y.detach().cpu().numpy(), raw_forward(case))


def test_harmonic_series_plays_what_the_bank_plays():
    """B = 0 and no detune: the oscillator bank's sound.  Allowed: this module's bound, the bank's, and the drift between the two
    phase definitions, 2 pi sum_k |A_k| c 2^-24 P_k[n] with c = 6 roundings of relative size 2^-24 in the bank's phase (DESIGN.md
    section 4): (h + 1) f, its product with fl32(2 pi), the division by the sample rate, w1 x[i1], the fma with w0 x[i0], and the
    running sum rounded to fp32.  The bank's own bound: the v_sin_f32 assumption, the reduced phase in (-4.8, 4.8) rad rounded to fp32
    (2^-22), its product with 1 / (2 pi) (2^-24 * 4.8) and |fl32(2 pi) - 2 pi| = 1.75e-7, and the same fp32 count as here."""
    class Conf:
        n_harmonics, sample_rate, hop_length = 8, SR, 64
    B, T, hop, K = 2, 6, 64, 8
    rng = np.random.default_rng(21)
    f0 = rng.uniform(60.0, 400.0, (B, T, 1)).astype(np.float32)
    c = rng.uniform(0.05, 2.0, (B, T, K)).astype(np.float32)
    a = rng.uniform(0.1, 1.5, (B, T, 1)).astype(np.float32)
    x = {"f0": dev(f0), "c": dev(c), "a": dev(a)}
    inh, bank = ddsp.InharmonicBank(Conf).cuda(), ddsp.OscillatorBank(Conf).cuda()
    with torch.no_grad():
        y_inh, y_bank = inh(x).cpu().numpy().astype(np.float64), bank(x).cpu().numpy().astype(np.float64)
    f = (f0 * np.arange(1, K + 1, dtype=np.float32)).astype(np.float32)      # what the module builds: fl32(f0 k)
    want = ref.forward(f, c, a, hop, SR)
    d = ref._setup(f, c, a, hop, SR, None, True)
    A = np.abs(d["au"])[..., None] * np.abs(d["wv"])
    bank_bound = (A * (ref.EPS_SIN + 2.0 ** -22 + 4.8 * 2.0 ** -24 + 1.75e-7)).sum(-1) + (K + ref.R_FORWARD) * ref.EPS * A.sum(-1)
    drift = 2.0 * np.pi * (A * 6.0 * 2.0 ** -24 * d["P"]).sum(-1)
    err = np.abs(y_inh - y_bank)
    allowed = want["bound"] + bank_bound + drift
    print(f"max |inharmonic - bank| {err.max():.3e}, worst err / allowance {(err / allowed).max():.3f}")
    assert (np.abs(y_inh - want["y"]) <= want["bound"]).all() and (err <= allowed).all()
    assert np.abs(y_bank).max() > 0.05


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
class TinyConf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 65, SR, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 1, 32, 1
    inharmonicity = 2e-4


def tiny_batch(B=2, T=8, seed=90):
    g = torch.Generator().manual_seed(seed)
    return {"f0": (100 + 300 * torch.rand(B, T, 1, generator=g)).cuda(), "normalized_cents": torch.rand(B, T, 1, generator=g).cuda(),
            "loudness": torch.rand(B, T, 1, generator=g).cuda(), "audio": (0.1 * torch.randn(B, T * 64, generator=g)).cuda()}


def tiny_decoder():
    torch.manual_seed(5)
    return ddsp.Decoder(TinyConf, noise_rng="device", seed=3, synth="inharmonic").cuda()


def test_decoder_learns_its_inharmonicity():
    dec, batch = tiny_decoder(), tiny_batch()
    bank = dec.harmonics
    assert isinstance(bank, ddsp.InharmonicBank) and abs(float(bank.inharmonicity.detach()) - 2e-4) < 1e-9
    loss_fn = ddsp.MSSLoss((256, 128, 64)).cuda()
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    before = (bank.inharmonicity.detach().clone(), bank.detune_cents.detach().clone())
    for _ in range(3):
        out = ddsp.train_step(dec, loss_fn, opt, batch)
        assert np.isfinite(float(out[0] if isinstance(out, (tuple, list)) else out))
    loss_fn(dec(batch), batch).backward()
    for name, p in dec.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(bank.inharmonicity.grad.abs()) > 0.0 and float(bank.detune_cents.grad.abs().min()) > 0.0
    assert not torch.equal(before[0], bank.inharmonicity.detach()) and not torch.equal(before[1], bank.detune_cents.detach())
    with torch.no_grad():                                        # the inference shortcut: noise accumulated into the synth's buffer
        assert dec(batch).shape == (2, 8 * 64) and bool(torch.isfinite(dec(batch)).all())


def test_fixed_ratios_pass_no_grad_f_buffer(monkeypatch):
    torch.manual_seed(5)
    dec = ddsp.Decoder(TinyConf, noise_rng="device", seed=3, synth="inharmonic").cuda()
    dec.harmonics = ddsp.InharmonicBank(TinyConf, inharmonicity=2e-4, learn=False).cuda()
    seen = []
    real = ddsp.sinusoids.sinusoids_backward

    def spy(*args, **kw):
        seen.append(kw.get("want_grad_f"))
        out = real(*args, **kw)
        assert out[0] is None
        return out
    monkeypatch.setattr(ddsp.sinusoids, "sinusoids_backward", spy)
    batch = tiny_batch()
    ddsp.MSSLoss((256, 128, 64)).cuda()(dec(batch), batch).backward()
    assert seen == [False] and dec.harmonics.inharmonicity.grad is None


def test_graphed_train_step_replays():
    dec, batch = tiny_decoder(), tiny_batch()
    loss_fn = ddsp.MSSLoss((256, 128, 64)).cuda()
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3, capturable=True)
    step = ddsp.GraphedTrainStep(dec, loss_fn, opt, batch)
    before = dec.harmonics.detune_cents.detach().clone()
    losses = [float(step(batch)[0]) for _ in range(2)]
    assert all(np.isfinite(v) for v in losses)
    assert not torch.equal(before, dec.harmonics.detune_cents.detach())


def test_refusals():
    dec = tiny_decoder()
    with pytest.raises(ValueError, match="inharmonic"):
        ddsp.GraphedLiveDecoder(dec, 4)

    class InConf(TinyConf):
        synth = "inharmonic"
    with pytest.raises(ValueError, match="inharmonic"):
        ddsp.GraphedSynth(InConf, 1, 4, 65, live=True)
    from encoder_common import AEConf
    ae = ddsp.AutoEncoder(AEConf, tracker="yin", synth="inharmonic").cuda()
    x = torch.zeros(1, 4096, device="cuda")
    for call in (lambda: ae.analyse(x), lambda: ae.transform(x), lambda: ae.morph(x, x)):
        with pytest.raises(ValueError, match="inharmonic"):
            call()
