"""The wavetable kernels (csrc/ddsp_wavetable.hip) against tests/wavetable_reference.py, element by element within the counted bounds,
in both kernel forms (the tables in LDS / read from memory) forced through ddsp_wavetable_set_form."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import wavetable_reference as ref

pytestmark = pytest.mark.gpu

SR = 16000
FORMS = {"lds": 1, "global": 2}
SHAPES = [(2, 5, 64, 3, 8), (3, 4, 6, 1, 16), (2, 7, 64, 20, 512), (1, 3, 5, 100, 64)]       # B, T, hop, N, L
TRACKS = ("constant", "ramp", "stall", "nyquist", "grid")
GUARD, SENTINEL = 64, -12345.0


@pytest.fixture(autouse=True)
def _default_hooks():
    yield
    L = ddsp._lib.lib()
    assert L.ddsp_wavetable_set_form(0) == 0 and L.ddsp_wavetable_set_grid(0) == 0


def set_form(form, chunk_frames=0, iter_frames=0):
    assert ddsp._lib.lib().ddsp_wavetable_set_form(FORMS[form] | (chunk_frames << 8) | (iter_frames << 16)) == 0


def f0_track(kind, B, T, L, rng):
    if kind == "constant":
        f0 = np.full((B, T), 220.0)
    elif kind == "ramp":                                    # tens of wraps inside the clip
        f0 = np.linspace(1500.0, 7000.0, B * T).reshape(B, T)
    elif kind == "stall":                                   # frames at exactly 0 Hz: the phase stands still
        f0 = rng.uniform(100.0, 900.0, (B, T))
        f0[:, 1::2] = 0.0
    elif kind == "nyquist":                                 # a frame above sample_rate / 2
        f0 = rng.uniform(100.0, 900.0, (B, T))
        f0[:, T // 2] = 9000.0
    else:                                                   # pos lands on integers: f0 = sample_rate / L * m
        f0 = SR / L * rng.integers(1, 6, (B, T)).astype(np.float64)
    return f0.astype(np.float32)


def make_case(shape, track, seed, tables="random"):
    B, T, hop, N, L = shape
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((N, L)).astype(np.float32)
    if tables == "wrap":                                    # one non-zero entry, at the wrap point
        W[0] = 0.0
        W[0, L - 1] = 1.0
    return dict(shape=shape, f0=f0_track(track, B, T, L, rng), c=rng.uniform(0.05, 2.0, (B, T, N)).astype(np.float32),
                a=rng.uniform(0.1, 1.5, (B, T)).astype(np.float32), W=W)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def raw_forward(case, phase=None):
    """ddsp_wavetable_forward into a buffer with guard zones -> y [B, T hop] (numpy)"""
    B, T, hop, N, L = case["shape"]
    lib = ddsp._lib.lib()
    f0, c, a, W = dev(case["f0"]), dev(case["c"]), dev(case["a"]), dev(case["W"])
    buf, y = guarded(B * T * hop)
    rc = lib.ddsp_wavetable_forward(f0.data_ptr(), c.data_ptr(), a.data_ptr(), W.data_ptr(), y.data_ptr(), None,
                                    None if phase is None else phase.data_ptr(), B, T, N, L, hop, SR, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return y.cpu().numpy().reshape(B, T * hop)


def raw_backward(case, gy):
    B, T, hop, N, L = case["shape"]
    lib = ddsp._lib.lib()
    f0, c, a, W, g = dev(case["f0"]), dev(case["c"]), dev(case["a"]), dev(case["W"]), dev(gy.astype(np.float32))
    (bc, gc), (ba, ga), (bw, gw) = guarded(B * T * N), guarded(B * T), guarded(N * L)
    scratch = torch.empty(lib.ddsp_wavetable_backward_scratch_bytes(B, T, N, L, hop), device="cuda", dtype=torch.uint8)
    rc = lib.ddsp_wavetable_backward(g.data_ptr(), f0.data_ptr(), c.data_ptr(), a.data_ptr(), W.data_ptr(), None, scratch.data_ptr(),
                                     gc.data_ptr(), ga.data_ptr(), gw.data_ptr(), B, T, N, L, hop, SR, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(bc) and guards_intact(ba) and guards_intact(bw)
    return gc.cpu().numpy().reshape(B, T, N), ga.cpu().numpy().reshape(B, T, 1), gw.cpu().numpy().reshape(N, L)


def check_forward(case, y, P0=None):
    want, bound, _ = ref.forward(case["f0"], case["c"], case["a"], case["W"], case["shape"][2], SR, P0)
    err = np.abs(y.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"forward {case['shape']}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.isfinite(y).all() and (err <= bound).all(), worst


def check_backward(case, gy, got):
    want = ref.backward(gy, case["f0"], case["c"], case["a"], case["W"], case["shape"][2], SR)
    for name, g in zip(("c", "a", "W"), got):
        err = np.abs(g.astype(np.float64) - want["grad_" + name])
        bound = want["bound_" + name]
        worst = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
        print(f"grad_{name} {case['shape']}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
        assert np.isfinite(g).all() and (err <= bound).all(), (name, worst)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_fp64(shape, form):
    set_form(form)
    assert ddsp.wavetable_form(*[shape[i] for i in (0, 1, 3, 4, 2)])["forward"] == form
    for i, track in enumerate(TRACKS):
        for tables in ("random", "wrap"):
            case = make_case(shape, track, 100 + i, tables)
            y = raw_forward(case)
            check_forward(case, y)
            if track == "ramp" and tables == "random":       # the same bits every run
                assert all(np.array_equal(y, raw_forward(case)) for _ in range(2))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("chunk_frames,iter_frames", [(2, 1), (3, 2), (0, 1)])
def test_forward_chunk_prefix_and_carried_scan(form, chunk_frames, iter_frames):
    """The paths a long clip takes -- a chunk that starts inside the row, several iterations per chunk -- forced at small shapes."""
    set_form(form, chunk_frames, iter_frames)
    for shape in (SHAPES[2], SHAPES[1]):
        for track in ("ramp", "grid"):
            case = make_case(shape, track, 7)
            check_forward(case, raw_forward(case))


@pytest.mark.parametrize("form", FORMS)
def test_grid_cap_strides_over_units(form):
    set_form(form, 2, 1)
    assert ddsp._lib.lib().ddsp_wavetable_set_grid(2) == 0
    case = make_case((4, 4, 8, 5, 32), "ramp", 11)           # 4 rows x 2 chunks = 8 units on 2 workgroups
    check_forward(case, raw_forward(case))
    gy = np.random.default_rng(12).standard_normal((4, 32))
    check_backward(case, gy, raw_backward(case, gy))


def test_harmonic_init_plays_what_the_bank_plays():
    class Conf:
        n_harmonics, sample_rate, hop_length = 8, SR, 64
    B, T, hop, N, L = 2, 6, 64, 8, 2048
    rng = np.random.default_rng(21)
    f0 = rng.uniform(60.0, 400.0, (B, T, 1)).astype(np.float32)
    c = rng.uniform(0.05, 2.0, (B, T, N)).astype(np.float32)
    a = rng.uniform(0.1, 1.5, (B, T, 1)).astype(np.float32)
    x = {"f0": dev(f0), "c": dev(c), "a": dev(a)}
    wt = ddsp.WavetableBank(Conf, table_size=L).cuda()
    bank = ddsp.OscillatorBank(Conf).cuda()
    for form in FORMS:
        set_form(form)
        with torch.no_grad():
            y_wt, y_bank = wt(x).cpu().numpy().astype(np.float64), bank(x).cpu().numpy().astype(np.float64)
        i0, i1, w0, w1 = ref.upsample_plan(T, hop)
        P = ref.phases(f0[..., 0], hop, SR)
        wn = c.astype(np.float64) / c.astype(np.float64).sum(-1, keepdims=True)
        m = w0[None, :, None] * wn[:, i0] + w1[None, :, None] * wn[:, i1]
        au = w0[None] * a[:, i0, 0].astype(np.float64) + w1[None] * a[:, i1, 0].astype(np.float64)
        h = 2.0 * np.pi * np.arange(1, N + 1)[None, None, :]
        bound = au * (m * ((h / L) ** 2 / 8.0 + h * P[..., None] * 2.0 ** -23)).sum(-1) + 1e-5
        err = np.abs(y_wt - y_bank)
        print(f"{form}: max |wavetable - bank| {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("form", FORMS)
def test_live_carries_a_phase_per_row(form):
    class Conf:
        n_harmonics, sample_rate, hop_length = 5, SR, 16
    set_form(form)
    B, T, hop, N, L = 3, 4, 16, 5, 32
    blocks = [make_case((B, T, hop, N, L), "ramp", 30 + i) for i in range(2)]
    for i, blk in enumerate(blocks):
        blk["f0"] = blk["f0"] * np.array([[0.1], [0.37], [1.0]], np.float32)     # every row at its own pitch
        blk["W"] = blocks[0]["W"]
    wt = ddsp.WavetableBank(Conf, table_size=L, init=torch.from_numpy(blocks[0]["W"])).cuda()
    P0 = None
    for blk in blocks:
        with torch.no_grad():
            y = wt.live({"f0": dev(blk["f0"][..., None]), "c": dev(blk["c"]), "a": dev(blk["a"][..., None])}).cpu().numpy()
        check_forward(blk, y, P0)
        _, _, P0 = ref.forward(blk["f0"], blk["c"], blk["a"], blk["W"], hop, SR, P0)
        state = wt.phase.cpu().numpy()
        d = np.abs(state - P0)
        assert (np.minimum(d, 1.0 - d) <= 1e-12).all(), (state, P0)
    assert len(set(np.round(state, 6))) == B                 # (three different phases: no row carries another's)
    wt.reset_phase()
    assert float(wt.phase.abs().max()) == 0.0


@pytest.mark.parametrize("form", FORMS)
def test_live_under_graph_replay_equals_eager_blocks(form):
    class Conf:
        n_harmonics, sample_rate, hop_length = 5, SR, 16
    set_form(form)
    B, T, hop, N, L = 2, 4, 16, 5, 32
    case = make_case((B, T, hop, N, L), "ramp", 41)
    x = {"f0": dev(case["f0"][..., None]), "c": dev(case["c"]), "a": dev(case["a"][..., None])}
    wt = ddsp.WavetableBank(Conf, table_size=L, init=torch.from_numpy(case["W"])).cuda()
    with torch.no_grad():
        eager = [wt.live(x).clone() for _ in range(2)]
        wt.reset_phase()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            wt.live(x)
        torch.cuda.current_stream().wait_stream(side)
        wt.reset_phase()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = wt.live(x)
        wt.reset_phase()
        for want in eager:
            graph.replay()
            assert torch.equal(out, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_backward_against_fp64(shape, form):
    set_form(form)
    assert ddsp.wavetable_form(*[shape[i] for i in (0, 1, 3, 4, 2)])["backward"] == form
    B, T, hop, N, L = shape
    rng = np.random.default_rng(50)
    for i, track in enumerate(("ramp", "grid", "stall")):
        case = make_case(shape, track, 60 + i, "wrap" if i == 1 else "random")
        case["c"][0, T // 2] = 0.7                           # a frame whose c is all equal: the normalisation's term alone
        gy = rng.standard_normal((B, T * hop))
        got = raw_backward(case, gy)
        check_backward(case, gy, got)
        if i == 0:
            again = raw_backward(case, gy)
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])        # grad_c, grad_a: the same bits
        one = np.zeros((B, T * hop))                         # one sample: every scatter target can be read off
        one[B - 1, (T * hop) // 2 + 1] = 1.5
        check_backward(case, one, raw_backward(case, one))


@pytest.mark.parametrize("form", FORMS)
def test_backward_chunk_prefix_and_carried_scan(form):
    set_form(form, 2, 1)
    for shape in (SHAPES[2], SHAPES[1]):
        case = make_case(shape, "ramp", 71)
        gy = np.random.default_rng(72).standard_normal((shape[0], shape[1] * shape[2]))
        check_backward(case, gy, raw_backward(case, gy))


def test_backward_planned_form_with_shortened_iterations():
    """32 tables of 512 points at hop 128: the planner keeps the backward in the LDS form by walking 3 frames per iteration."""
    shape = (1, 5, 128, 32, 512)
    assert ddsp.wavetable_form(1, 5, 32, 512, 128) == dict(forward="lds", backward="lds")
    case = make_case(shape, "ramp", 75)
    gy = np.random.default_rng(76).standard_normal((1, 5 * 128))
    check_forward(case, raw_forward(case))
    check_backward(case, gy, raw_backward(case, gy))


@pytest.mark.parametrize("form", FORMS)
def test_autograd_function_matches_the_raw_backward(form):
    set_form(form)
    shape = SHAPES[0]
    case = make_case(shape, "ramp", 80)
    f0, c, a = dev(case["f0"][..., None]), dev(case["c"]).requires_grad_(), dev(case["a"][..., None]).requires_grad_()

    class Conf:
        n_harmonics, sample_rate, hop_length = shape[3], SR, shape[2]
    wt = ddsp.WavetableBank(Conf, table_size=shape[4], init=torch.from_numpy(case["W"])).cuda()
    gy = np.random.default_rng(81).standard_normal((shape[0], shape[1] * shape[2]))
    y = wt({"f0": f0, "c": c, "a": a})
    y.backward(dev(gy.astype(np.float32)))
    check_backward(case, gy, (c.grad.cpu().numpy(), a.grad.cpu().numpy(), wt.wavetables.grad.cpu().numpy()))


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
class TinyConf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 65, SR, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 1, 32, 1
    wavetable_size = 64


def tiny_batch(B=2, T=8, seed=90):
    g = torch.Generator().manual_seed(seed)
    return {"f0": (100 + 300 * torch.rand(B, T, 1, generator=g)).cuda(), "normalized_cents": torch.rand(B, T, 1, generator=g).cuda(),
            "loudness": torch.rand(B, T, 1, generator=g).cuda(), "audio": (0.1 * torch.randn(B, T * 64, generator=g)).cuda()}


def tiny_decoder():
    torch.manual_seed(5)
    return ddsp.Decoder(TinyConf, noise_rng="device", seed=3, synth="wavetable").cuda()


@pytest.mark.parametrize("form", FORMS)
def test_decoder_trains_the_tables(form):
    set_form(form)
    dec, batch = tiny_decoder(), tiny_batch()
    assert isinstance(dec.harmonics, ddsp.WavetableBank) and dec.harmonics.wavetables.shape == (8, 64)
    loss_fn = ddsp.MSSLoss((256, 128, 64)).cuda()
    loss = loss_fn(dec(batch), batch)
    loss.backward()
    for name, p in dec.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(dec.harmonics.wavetables.grad.abs().max()) > 0.0
    with torch.no_grad():                                    # the inference shortcut: noise accumulated into the synth's buffer
        assert dec(batch).shape == (2, 8 * 64) and bool(torch.isfinite(dec(batch)).all())
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    before = dec.harmonics.wavetables.detach().clone()
    out = ddsp.train_step(dec, loss_fn, opt, batch)
    assert np.isfinite(float(out[0] if isinstance(out, (tuple, list)) else out))
    assert not torch.equal(before, dec.harmonics.wavetables.detach())


@pytest.mark.parametrize("form", FORMS)
def test_graphed_train_step_replays(form):
    set_form(form)                                           # (captured and replayed under the forced form)
    dec, batch = tiny_decoder(), tiny_batch()
    loss_fn = ddsp.MSSLoss((256, 128, 64)).cuda()
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3, capturable=True)
    step = ddsp.GraphedTrainStep(dec, loss_fn, opt, batch)
    before = dec.harmonics.wavetables.detach().clone()
    losses = [float(step(batch)[0]) for _ in range(2)]
    assert all(np.isfinite(v) for v in losses)
    assert not torch.equal(before, dec.harmonics.wavetables.detach())

