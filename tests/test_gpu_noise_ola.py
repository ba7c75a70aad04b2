"""The overlap-add filtered noise on the device (csrc/ddsp_noise_ola.hip) against the fp64 definition of
tests/noise_ola_reference.py: forward and backward elementwise to TOL_Y Yf / TOL_DH Yb (derived on the host:
tests/test_noise_ola_host.py::test_device_bound) on every shape, the same bits whatever the batch, the run or the alignment, the
reach of a non-finite value, the Python layers that carry the flag, and the statistics that motivate the mode.  The worst ratios
are printed at the end (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
import noise_ola_reference as ref  # noqa: E402
from encoder_common import AEConf  # noqa: E402
from oracle import oracle  # noqa: E402

SHAPES = ref.GPU_SHAPES
SEED, OFFSET = 5, 77
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\noverlap-add noise, worst error / yardstick: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 9, 16000, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1


class OlaConf(Conf):
    noise_overlap_add = True


def hop_conf(hop, **extra):
    return type("HopConf", (), dict(hop_length=hop, **extra))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def forward(H, hop, **kw):
    return ddsp.noise_forward(H if torch.is_tensor(H) else cuda(H), hop, overlap_add=True, **kw)


def backward(g, hop, F, **kw):
    return ddsp.noise_backward(g if torch.is_tensor(g) else cuda(g), hop, F, overlap_add=True, **kw)


@pytest.fixture(scope="module")
def cases():
    """Per shape: inputs and the fp64 results, computed once and left unchanged."""
    out = {}
    for shape in SHAPES:
        B, T, hop, F = shape
        H, u, g = ref.gpu_H(shape), ref.gpu_uniform(shape), ref.gpu_grad(shape)
        up = oracle.philox_uniform(SEED, OFFSET, B, T, hop)
        y, Yf = ref.ola_fp64(H, hop, uniform=u)
        yp, Yfp = ref.ola_fp64(H, hop, uniform=up)
        dH, Yb = ref.ola_grad_fp64(g, F, hop, uniform=u)
        dHp, Ybp = ref.ola_grad_fp64(g, F, hop, uniform=up)
        out[shape] = dict(H=H, u=u, g=g, up=up, y=y, Yf=Yf, yp=yp, Yfp=Yfp, dH=dH, Yb=Yb, dHp=dHp, Ybp=Ybp)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_matches_fp64(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    y = forward(c["H"], hop, uniform=cuda(c["u"]))
    r = ref.ratio(y.cpu().numpy(), c["y"], c["Yf"])
    yp = forward(c["H"], hop, seed=SEED, offset=OFFSET)
    rp = ref.ratio(yp.cpu().numpy(), c["yp"], c["Yfp"])
    print(f"{shape}: |y - fp64| / Yf: injected draw {r:.3e}, in-kernel draw {rp:.3e} (TOL_Y {ref.TOL_Y:g})")
    WORST["forward"] = max(WORST.get("forward", 0.0), r, rp)
    assert y.shape == (B, T * hop) and r <= ref.TOL_Y and rp <= ref.TOL_Y
    assert same_bits(yp, forward(c["H"], hop, uniform=cuda(c["up"])))           # the regenerated draw, injected: the same bits
    assert not same_bits(yp, y)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[8]], ids=str)
def test_device_counter_is_the_offset(shape, cases):
    B, T, hop, F = shape
    H = cuda(cases[shape]["H"])
    counter = torch.tensor([OFFSET], dtype=torch.int64, device="cuda")
    assert same_bits(forward(H, hop, seed=SEED, counter=counter), forward(H, hop, seed=SEED, offset=OFFSET))
    assert same_bits(forward(H, hop, seed=SEED, offset=7, counter=counter), forward(H, hop, seed=SEED, offset=OFFSET + 7))
    g = cuda(cases[shape]["g"])
    assert same_bits(backward(g, hop, F, seed=SEED, counter=counter), backward(g, hop, F, seed=SEED, offset=OFFSET))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_accumulate_is_the_fp32_sum(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    H, u = cuda(c["H"]), cuda(c["u"])
    y0 = torch.randn(B, T * hop, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    out = y0.clone()
    got = forward(H, hop, uniform=u, out=out, accumulate=True)
    assert got.data_ptr() == out.data_ptr()
    assert same_bits(out, y0 + forward(H, hop, uniform=u))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_zero_frame_contributes_exact_zeros(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    u = cuda(c["u"])
    assert (forward(np.zeros_like(c["H"]), hop, uniform=u) == 0).all()
    t0 = T // 2
    only = np.zeros_like(c["H"])
    only[:, t0] = c["H"][:, 0] + 0.01
    y = forward(only, hop, uniform=u).cpu().numpy()
    lo, hi = ref.reach(t0, T, hop, F)
    assert (y[:, :lo] == 0).all() and (y[:, hi:] == 0).all() and (np.abs(y[:, lo:hi]).max(axis=1) > 0).all()
    # and in the shared inputs: where only a zero frame reaches, the output is an exact zero
    y = forward(c["H"], hop, uniform=u).cpu().numpy()
    n = np.arange(T * hop)
    for b, t in ref.zero_frames(c["H"]):
        inner = (n - (F - 2) >= t * hop) & (n + (F - 2) < (t + 1) * hop)          # every source sample within reach lies in frame t
        edge_lo = (t == 0) & (n + (F - 2) < (t + 1) * hop)
        edge_hi = (t == T - 1) & (n - (F - 2) >= t * hop)
        assert (y[b, inner | edge_lo | edge_hi] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bits_do_not_depend_on_batch_run_or_alignment(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    H, u, g = cuda(c["H"]), cuda(c["u"]), cuda(c["g"])
    y, d = forward(H, hop, uniform=u), backward(g, hop, F, uniform=u)
    yp, dp = forward(H, hop, seed=SEED, offset=OFFSET), backward(g, hop, F, seed=SEED, offset=OFFSET)
    assert same_bits(y, forward(H, hop, uniform=u)) and same_bits(d, backward(g, hop, F, uniform=u))             # two calls
    assert same_bits(yp, forward(H, hop, seed=SEED, offset=OFFSET)) and same_bits(dp, backward(g, hop, F, seed=SEED, offset=OFFSET))
    quads = (hop + 3) // 4
    for b in range(B):                                                                                            # each row alone
        assert same_bits(y[b:b + 1], forward(H[b:b + 1], hop, uniform=u[b:b + 1]))
        assert same_bits(d[b:b + 1], backward(g[b:b + 1], hop, F, uniform=u[b:b + 1]))
        off = OFFSET + b * T * quads
        assert same_bits(yp[b:b + 1], forward(H[b:b + 1], hop, seed=SEED, offset=off))
        assert same_bits(dp[b:b + 1], backward(g[b:b + 1], hop, F, seed=SEED, offset=off))
    assert same_bits(y.flip(0), forward(H.flip(0), hop, uniform=u.flip(0)))                                     # the reversed batch
    assert same_bits(d.flip(0), backward(g.flip(0), hop, F, uniform=u.flip(0)))

    def shifted(t):                                               # the same values one float further on
        buf = torch.empty(t.numel() + 1, device="cuda", dtype=torch.float32)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 8 == 4 and view.is_contiguous()
        return view

    out = shifted(torch.zeros_like(y))
    forward(shifted(H), hop, uniform=shifted(u), out=out, accumulate=False)
    assert same_bits(y, out)
    assert same_bits(d, backward(shifted(g), hop, F, uniform=shifted(u)))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_nan_in_one_frame_reaches_its_window_only(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    u = cuda(c["u"])
    clean = forward(c["H"], hop, uniform=u)
    b, t = B - 1, T // 2
    bad = c["H"].copy()
    bad[b, t, F // 2] = np.nan
    y = forward(bad, hop, uniform=u)
    lo, hi = ref.reach(t, T, hop, F)
    hit = torch.zeros_like(y, dtype=torch.bool)
    hit[b, lo:hi] = True
    assert torch.isnan(y[hit]).all()
    assert torch.equal(bits(y)[~hit], bits(clean)[~hit])
    want, _ = ref.ola_fp64(bad, hop, uniform=c["u"])              # the fp64 definition has the same reach
    assert np.array_equal(np.isnan(want), hit.cpu().numpy())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_matches_fp64(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    g = cuda(c["g"])
    d = backward(g, hop, F, uniform=cuda(c["u"]))
    r = ref.ratio(d.cpu().numpy(), c["dH"], c["Yb"][..., None])
    dp = backward(g, hop, F, seed=SEED, offset=OFFSET)
    rp = ref.ratio(dp.cpu().numpy(), c["dHp"], c["Ybp"][..., None])
    print(f"{shape}: |dH - fp64| / Yb: injected draw {r:.3e}, in-kernel draw {rp:.3e} (TOL_DH {ref.TOL_DH:g})")
    WORST["backward"] = max(WORST.get("backward", 0.0), r, rp)
    assert d.shape == (B, T, F) and r <= ref.TOL_DH and rp <= ref.TOL_DH
    assert same_bits(dp, backward(g, hop, F, uniform=cuda(c["up"])))

    # a NaN in g[n] reaches the frames whose windows hold n, and nothing else
    b, n = B - 1, (T * hop) // 2
    bad = c["g"].copy()
    bad[b, n] = np.nan
    got = backward(bad, hop, F, uniform=cuda(c["u"]))
    hit = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    for t in range(T):
        lo, hi = ref.reach(t, T, hop, F)
        hit[b, t] = lo <= n < hi
    assert hit.any() and torch.isnan(got[hit]).all()
    assert torch.equal(bits(got)[~hit], bits(d)[~hit])
    want, _ = ref.ola_grad_fp64(bad, F, hop, uniform=c["u"])
    assert np.array_equal(np.isnan(want).all(axis=-1), hit.cpu().numpy()) and np.array_equal(np.isnan(want).any(axis=-1), hit.cpu().numpy())


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[6]], ids=str)
def test_the_module_returns_that_gradient(shape, cases):
    B, T, hop, F = shape
    c = cases[shape]
    u, g = cuda(c["u"]), cuda(c["g"])
    module = ddsp.FilteredNoise(hop_conf(hop), overlap_add=True).cuda()
    H = cuda(c["H"]).requires_grad_()
    y = module({"H": H}, noise=u)
    assert same_bits(y, forward(c["H"], hop, uniform=u))
    y.backward(g)
    assert same_bits(H.grad, backward(g, hop, F, uniform=u))
    assert ref.ratio(H.grad.cpu().numpy(), c["dH"], c["Yb"][..., None]) <= ref.TOL_DH
    # the in-kernel draw: forward and backward see the same samples, and the stream moves on between calls
    module = ddsp.FilteredNoise(hop_conf(hop), rng="device", seed=SEED, overlap_add=True).cuda()
    module.reseed(SEED, OFFSET)
    H = cuda(c["H"]).requires_grad_()
    module({"H": H}).backward(g)
    assert same_bits(H.grad, backward(g, hop, F, seed=SEED, offset=OFFSET))
    assert module._offset == OFFSET + module.draws(B, T)


def test_the_configuration_switches_the_mode_on():
    shape = SHAPES[0]
    B, T, hop, F = shape
    H, u = cuda(ref.gpu_H(shape)), cuda(ref.gpu_uniform(shape))
    on = ddsp.FilteredNoise(hop_conf(hop, noise_overlap_add=True))
    assert on.overlap_add and same_bits(on({"H": H}, noise=u), forward(H, hop, uniform=u))
    assert ddsp.Decoder(OlaConf).noise.overlap_add and not ddsp.Decoder(Conf).noise.overlap_add
    assert ddsp.Decoder(Conf, noise_overlap_add=True).noise.overlap_add and not ddsp.Decoder(OlaConf, noise_overlap_add=False).noise.overlap_add
    ae_conf = type("AEOla", (AEConf,), dict(noise_overlap_add=True))
    assert ddsp.AutoEncoder(ae_conf, tracker="yin").decoder.noise.overlap_add
    assert ddsp.AutoEncoder(AEConf, tracker="yin", noise_overlap_add=True).decoder.noise.overlap_add
    assert not ddsp.AutoEncoder(AEConf, tracker="yin").decoder.noise.overlap_add


def test_without_the_flag_nothing_changes():
    shape = SHAPES[0]
    B, T, hop, F = shape
    H, u = cuda(ref.gpu_H(shape)), cuda(ref.gpu_uniform(shape))
    module = ddsp.FilteredNoise(hop_conf(hop))
    assert module.overlap_add is False
    today = ddsp.noise_forward(H, hop, uniform=u)
    assert same_bits(module({"H": H}, noise=u), today)
    assert not same_bits(today, forward(H, hop, uniform=u))
    Hg = H.clone().requires_grad_()
    g = cuda(ref.gpu_grad(shape))
    module({"H": Hg}, noise=u).backward(g)
    assert same_bits(Hg.grad, ddsp.noise_backward(g, hop, F, uniform=u))


def controls(conf, B, T, seed=0):
    gen = torch.Generator("cuda").manual_seed(seed)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)           # noqa: E731
    return dict(f0=100.0 + 300.0 * rand(B, T, 1), c=rand(B, T, conf.n_harmonics) / conf.n_harmonics, a=rand(B, T, 1),
                H=0.1 * rand(B, T, conf.n_noise_filters))


def test_synthesize_keeps_its_fused_path():
    B, T = 2, 7
    dec = ddsp.Decoder(OlaConf, noise_rng="device", seed=SEED).cuda().eval()
    ctrl = controls(OlaConf, B, T)
    with torch.no_grad():
        dry = dec.harmonics(ctrl)
        y = dec.synthesize(ctrl)
    noise = forward(ctrl["H"], OlaConf.hop_length, seed=SEED, offset=0)
    assert same_bits(y, dry + noise)
    assert dec.noise._offset == dec.noise.draws(B, T)
    # under autograd the sum is torch's, of the same two terms
    ctrl["H"].requires_grad_()
    y2 = dec.synthesize(ctrl)
    assert same_bits(y2, dry + forward(ctrl["H"], OlaConf.hop_length, seed=SEED, offset=dec.noise.draws(B, T)))


def test_the_graphed_pass_replays_the_mode():
    B, T = 2, 5
    synth = ddsp.GraphedSynth(OlaConf, B, T, OlaConf.n_noise_filters, noise_seed=SEED)
    ctrl = controls(OlaConf, B, T, seed=1)
    draws = B * T * ((OlaConf.hop_length + 3) // 4)
    dry = ddsp.osc_forward(ctrl["f0"], ctrl["c"], ctrl["a"], OlaConf.hop_length, OlaConf.sample_rate)[0]
    for call in range(2):
        y = synth(ctrl).clone()
        assert same_bits(y, dry + forward(ctrl["H"], OlaConf.hop_length, seed=SEED, offset=call * draws))


def test_live_paths_and_the_truncated_analysis_refuse_the_mode():
    dec = ddsp.Decoder(OlaConf)
    with pytest.raises(ValueError, match="overlap-add"):
        dec.forward_live({}, None)
    with pytest.raises(ValueError, match="overlap-add"):
        ddsp.GraphedLiveDecoder(dec.cuda(), 4)
    with pytest.raises(ValueError, match="overlap-add"):
        ddsp.GraphedSynth(OlaConf, 1, 4, OlaConf.n_noise_filters, live=True)
    ae = ddsp.AutoEncoder(AEConf, tracker="yin", noise_overlap_add=True)
    x = torch.zeros(1, 4096)
    with pytest.raises(ValueError, match="truncated"):
        ae.analyse(x, noise=True)


def test_range_and_arguments():
    ones = lambda *s: torch.ones(*s, device="cuda")              # noqa: E731
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        forward(ones(1, 2, 258), 128)
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        forward(ones(1, 2, 65), 1025)
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_EINVAL"):
        forward(ones(1, 2, 1), 16)
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        backward(ones(1, 2 * 128), 128, 258)
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        backward(ones(1, 2 * 1025), 1025, 65)
    assert forward(ones(0, 2, 65), 128).shape == (0, 256) and backward(ones(0, 256), 128, 65).shape == (0, 2, 65)
    y = forward(ones(1, 3, 2), 5, seed=1)                         # the smallest filter: one tap, h[0] = (H0 + H1) / 2
    x = cuda(ref.draw(1, 3, 5, None, 1, 0).reshape(1, 15))
    assert same_bits(y, x)
    assert torch.isfinite(forward(ones(1, 2, 257), 1024, seed=1)).all() and torch.isfinite(forward(ones(1, 300, 257), 1, seed=1)).all()


def test_end_to_end_statistics():
    """rng='device', 2048 frames of the host test's low-pass H at (65, 128): the overlap-add output passes the host test's two
    conditions; the truncated form from the same module, same seed, fails both."""
    F, hop, T = 65, 128, 2048
    Hs = ref.lowpass_H(F)
    ctrl = {"H": cuda(np.tile(Hs.astype(np.float32), (1, T, 1)))}
    fig = {}
    for name, flag in (("overlap-add", True), ("truncated", False)):
        y = ddsp.FilteredNoise(hop_conf(hop), rng="device", seed=3, overlap_add=flag).cuda()(ctrl)[0].double().cpu().numpy()
        fig[name] = (ref.position_variance_ratio(y, hop), ref.welch_distance(y, Hs, hop))
        print(f"{name}: variance by position min / max {fig[name][0]:.3f}, Welch distance {fig[name][1]:.4f}")
    assert fig["overlap-add"][0] >= 0.8 and fig["overlap-add"][1] <= 0.05
    assert fig["truncated"][0] < 0.8 and fig["truncated"][1] > 0.05
