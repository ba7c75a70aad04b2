"""The overlap-add noise as a stream on the device (csrc/ddsp_noise_ola.hip: ola_stream_kernel; DESIGN.md section 5a, "Live"):
the blocks of a stream, with trailing silent blocks until the tail has left, against the offline `noise_forward(...,
overlap_add=True)` on the clip behind leading silent frames, shifted by the delay D = F - 2, IN BITS; against the fp64 stream of
tests/noise_ola_stream_reference.py to the offline form's derived bound TOL_Y (the chains are the offline form's); the delayed
dry signal, row independence, the reach of a non-finite value across blocks, and the modules and graphs that carry the state.
The worst ratio is printed at the end (pytest -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddsp_pytorch_amd as ddsp  # noqa: E402
import noise_ola_reference as ref  # noqa: E402
import noise_ola_stream_reference as sref  # noqa: E402

SHAPES = sref.GPU_SHAPES
SEED, OFFSET = 5, 5000
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\noverlap-add stream, worst error / yardstick: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def quads(hop):
    return (hop + 3) // 4


@pytest.fixture(scope="module")
def cases():
    """Per shape: the inputs, followed by the Z silent frames that flush the tail, and the fp64 stream; computed once, left unchanged."""
    out = {}
    for shape in SHAPES:
        B, T, hop, F, Tb = shape
        H, u = ref.gpu_H(shape[:4]), ref.gpu_uniform(shape[:4])
        dry = ref.gpu_grad(shape[:4], seed=1)
        y, Yf, Z = sref.run(H, hop, Tb, ref.draw(B, T, hop, u))
        out[shape] = dict(H=cuda(sref.padded(H, 0, Z)), u=cuda(sref.padded(u, 0, Z)), dry=cuda(np.pad(dry, [(0, 0), (0, Z * hop)])),
                          y=y, Yf=Yf, Z=Z)
    return out


def stream(H, hop, Tb, uniform=None, dry=None, seed=0, offset=0, counter=None, advance=None):
    """H [B, frames, F] in blocks of Tb frames through the raw launcher -> (the concatenated output, the last state).
    advance: 'offset' / 'counter' moves that one on by T_b ceil(hop / 4) after each block."""
    B, frames, F = H.shape
    state, outs = ddsp.ola_stream_state(B, F, H.device), []
    for a, b in sref.blocks_of(frames, Tb):
        o, state = ddsp.noise_ola_stream(H[:, a:b], hop, state, dry=None if dry is None else dry[:, a * hop:b * hop].contiguous(),
                                         uniform=None if uniform is None else uniform[:, a:b], seed=seed, offset=offset, counter=counter)
        outs.append(o)
        if advance == "offset":
            offset += (b - a) * quads(hop)
        elif advance == "counter":
            counter.add_((b - a) * quads(hop))
    return torch.cat(outs, dim=1), state


def offline(H, hop, uniform=None, **kw):
    """The existing offline form on H behind leading silent frames, as the stream it defines: stream[i] = y[i - D]."""
    B, frames, F = H.shape
    lead = sref.lead_frames(hop, F)
    front = lambda t: torch.cat([t.new_zeros((B, lead, t.shape[2])), t], dim=1)      # noqa: E731
    y = ddsp.noise_forward(front(H), hop, uniform=None if uniform is None else front(uniform), overlap_add=True, **kw)
    return sref.shifted(y, lead, hop, F, frames * hop)


def delayed(dry, F):
    D = sref.delay(F)
    return torch.cat([torch.zeros_like(dry[:, :D]), dry], dim=1)[:, :dry.shape[1]]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_blocks_are_the_offline_form_in_bits(shape, cases):
    B, T, hop, F, Tb = shape
    c = cases[shape]
    got, state = stream(c["H"], hop, Tb, uniform=c["u"])
    assert got.shape == (B, (T + c["Z"]) * hop) and state.shape == (B, sref.state_floats(F))
    assert same_bits(got, offline(c["H"], hop, uniform=c["u"]))
    assert (state == 0).all()                                     # the tail has left: what remains is the silence behind it
    r = ref.ratio(got.cpu().numpy(), c["y"], c["Yf"])
    print(f"{shape}: |stream - fp64| / Yf = {r:.3e} (TOL_Y {ref.TOL_Y:g}); {c['Z']} silent frames flush the tail")
    WORST["stream"] = max(WORST.get("stream", 0.0), r)
    assert r <= ref.TOL_Y
    if F > 2:
        assert got[:, :F - 2].abs().max() > 0                     # the pre-ring of the first frames, which the offline form crops
        _, mid = stream(c["H"][:, :Tb], hop, Tb, uniform=c["u"][:, :Tb])
        assert mid[:, :2 * F - 4].abs().max() > 0 and (mid[:, 2 * F - 4:] == 0).all()      # a tail, and no dry history


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_one_row_in_kernel_draw_is_one_long_clip(shape, cases):
    """Offset, and in a second run the device counter, advanced by T_b ceil(hop / 4) per block: the offline form at the offset
    that gives the first streamed frame the same counter."""
    B, T, hop, F, Tb = shape
    H = cases[shape]["H"][:1].contiguous()
    back = sref.lead_frames(hop, F) * quads(hop)
    assert OFFSET >= back
    want = offline(H, hop, seed=SEED, offset=OFFSET - back)
    got, _ = stream(H, hop, Tb, seed=SEED, offset=OFFSET, advance="offset")
    assert same_bits(got, want)
    counter = torch.tensor([OFFSET - 7], dtype=torch.int64, device="cuda")
    got, _ = stream(H, hop, Tb, seed=SEED, offset=7, counter=counter, advance="counter")
    assert same_bits(got, want)
    assert int(counter) == OFFSET - 7 + H.shape[1] * quads(hop)
    if T - Tb >= 2:                                               # (gpu_H silences one frame: two later frames leave one that sounds)
        assert not same_bits(stream(H, hop, Tb, seed=SEED, offset=OFFSET)[0], want)       # an offset that stands still repeats its draw


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dry_is_delayed_with_the_noise(shape, cases):
    """out = fl32(delayed dry + noise-only out); at (1, 9, 2, 65, 2) the history of 63 samples crosses blocks of 4."""
    B, T, hop, F, Tb = shape
    c = cases[shape]
    noise, _ = stream(c["H"], hop, Tb, uniform=c["u"])
    got, state = stream(c["H"], hop, Tb, uniform=c["u"], dry=c["dry"])
    assert same_bits(got, delayed(c["dry"], F) + noise)
    # the history is the last D samples of dry: after the first block, and after the silence that flushed the tail
    D, n = sref.delay(F), Tb * hop
    first = c["dry"][:, :n].contiguous()
    _, mid = stream(c["H"][:, :Tb], hop, Tb, uniform=c["u"][:, :Tb], dry=first)
    assert same_bits(mid[:, 2 * D:], torch.cat([torch.zeros_like(c["dry"][:, :D]), first], dim=1)[:, n:])
    assert (state[:, 2 * D:] == 0).all()


def test_arguments():
    H, st = torch.ones(1, 2, 9, device="cuda"), ddsp.ola_stream_state(1, 9, "cuda")
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_EINVAL"):
        ddsp.noise_ola_stream(H, 16, st, state_out=st)            # two distinct buffers: workgroups read what others overwrite
    with pytest.raises(ValueError, match="state"):
        ddsp.noise_ola_stream(H, 16, st[:, :-1])
    with pytest.raises(ValueError, match="dry"):
        ddsp.noise_ola_stream(H, 16, st, dry=torch.zeros(1, 31, device="cuda"))
    with pytest.raises(ddsp._lib.DdspHipError, match="DDSP_ERANGE"):
        ddsp.noise_ola_stream(torch.ones(1, 2, 258, device="cuda"), 16, ddsp.ola_stream_state(1, 258, "cuda"))
    out, new = ddsp.noise_ola_stream(H[:0], 16, st[:0])
    assert out.shape == (0, 32) and new.shape == (0, 21)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 1], ids=str)
def test_rows_do_not_depend_on_the_batch_or_the_run(shape, cases):
    B, T, hop, F, Tb = shape
    c = cases[shape]
    got, state = stream(c["H"], hop, Tb, uniform=c["u"], dry=c["dry"])
    again, state2 = stream(c["H"], hop, Tb, uniform=c["u"], dry=c["dry"])
    assert same_bits(got, again) and same_bits(state, state2)
    for b in range(B):
        alone, _ = stream(c["H"][b:b + 1], hop, Tb, uniform=c["u"][b:b + 1], dry=c["dry"][b:b + 1])
        assert same_bits(got[b:b + 1], alone)
    flipped, _ = stream(c["H"].flip(0), hop, Tb, uniform=c["u"].flip(0), dry=c["dry"].flip(0))
    assert same_bits(got.flip(0), flipped)
    # the state in the middle of the stream, too
    mid = stream(c["H"][:, :Tb], hop, Tb, uniform=c["u"][:, :Tb], dry=c["dry"][:, :Tb * hop].contiguous())[1]
    mid_flipped = stream(c["H"].flip(0)[:, :Tb], hop, Tb, uniform=c["u"].flip(0)[:, :Tb], dry=c["dry"].flip(0)[:, :Tb * hop].contiguous())[1]
    assert same_bits(mid.flip(0), mid_flipped)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_nan_reaches_its_interval_of_the_stream_only(shape, cases):
    """A non-finite H_t: the stream samples [t hop, (t + 1) hop + M - 3] of its row, across block boundaries, and nothing else --
    the blocks after the interval are the clean stream's again, in bits."""
    B, T, hop, F, Tb = shape
    c = cases[shape]
    clean, _ = stream(c["H"], hop, Tb, uniform=c["u"])
    b, t = B - 1, T // 2
    bad = c["H"].clone()
    bad[b, t, F // 2] = float("nan")
    got, state = stream(bad, hop, Tb, uniform=c["u"])
    lo, hi = t * hop, (t + 1) * hop + 2 * (F - 1) - 3
    assert hi < got.shape[1]
    hit = torch.zeros_like(got, dtype=torch.bool)
    hit[b, lo:hi + 1] = True
    assert torch.isnan(got[hit]).all() and hit.any()
    assert torch.equal(bits(got)[~hit], bits(clean)[~hit])
    assert torch.isfinite(state).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_silent_block_returns_exact_zeros_and_a_zero_state(shape, cases):
    B, T, hop, F, Tb = shape
    c = cases[shape]
    H = torch.zeros(B, Tb, F, device="cuda")
    for kw in (dict(uniform=c["u"][:, :Tb]), dict(seed=SEED, offset=OFFSET)):
        out, state = stream(H, hop, Tb, **kw)
        assert same_bits(out, torch.zeros(B, Tb * hop, device="cuda")) and same_bits(state, torch.zeros(B, sref.state_floats(F), device="cuda"))


# ---------------------------------------------------------------------------------------------------------- modules and graphs

def hop_conf(hop, **extra):
    return type("HopConf", (), dict(hop_length=hop, **extra))


def test_the_module_carries_the_state():
    shape = SHAPES[1]                                             # hop 64, 65 bands, one frame a block: the tail outlives the block
    B, T, hop, F, Tb = shape
    H, u = cuda(ref.gpu_H(shape[:4])), cuda(ref.gpu_uniform(shape[:4]))
    dry = cuda(ref.gpu_grad(shape[:4], seed=1))
    raw, _ = stream(H[:, :3], hop, Tb, uniform=u[:, :3], dry=dry[:, :3 * hop].contiguous())
    module = ddsp.FilteredNoise(hop_conf(hop), overlap_add=True).cuda()
    calls = lambda: torch.cat([module.live({"H": H[:, t:t + 1]}, noise=u[:, t:t + 1], dry=dry[:, t * hop:(t + 1) * hop].contiguous())   # noqa: E731
                               for t in range(3)], dim=1)
    first = calls()
    assert same_bits(first, raw) and module.stream_delay == F - 2 and module.state_dict() == {}
    address = module._stream_state.data_ptr()
    assert not same_bits(calls(), raw)                            # the stream goes on ...
    module.reset_stream()
    assert same_bits(calls(), raw) and module._stream_state.data_ptr() == address             # ... until it is restarted, in place
    with pytest.raises(ValueError, match="reset_stream"):
        module.live({"H": H[:, :1].repeat(2, 1, 1)}, noise=u[:, :1].repeat(2, 1, 1))
    module.reset_stream()
    assert module.live({"H": H[:, :1].repeat(2, 1, 1)}, noise=u[:, :1].repeat(2, 1, 1)).shape == (2, hop)
    # the in-kernel draw: the module's offset moves on by what each block consumes
    module = ddsp.FilteredNoise(hop_conf(hop), rng="device", seed=SEED, overlap_add=True).cuda()
    module.reseed(SEED, OFFSET)
    got = torch.cat([module.live({"H": H[:, t:t + 1]}) for t in range(3)], dim=1)
    assert same_bits(got, stream(H[:, :3], hop, Tb, seed=SEED, offset=OFFSET, advance="offset")[0])
    assert module._offset == OFFSET + 3 * quads(hop)
    assert ddsp.FilteredNoise(hop_conf(hop)).stream_delay == 0


class LiveConf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 16, 65, 16000, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 2, 128, 1
    noise_overlap_add = True


def test_the_live_decoder_and_its_graph():
    """forward_live(delayed=True) over three callbacks of one frame (block 64, tail 126) against the hand composition, in bits;
    GraphedLiveDecoder(delayed=True) against those eager callbacks within 1e-6, the figure of
    test_decoder_training.py::test_graphed_live_decoder_equals_eager_callbacks for the same composition."""
    C = LiveConf
    torch.manual_seed(11)
    dec = ddsp.Decoder(C, noise_rng="device", seed=SEED).cuda().eval()
    with torch.no_grad():
        dec.reverb.wet.fill_(0.3)
    hand = ddsp.Decoder(C, noise_rng="device", seed=SEED).cuda().eval()
    graphed_model = ddsp.Decoder(C, noise_rng="device", seed=SEED).cuda().eval()
    hand.load_state_dict(dec.state_dict())
    graphed_model.load_state_dict(dec.state_dict())
    live = ddsp.GraphedLiveDecoder(graphed_model, 1, noise_seed=SEED, delayed=True)
    assert live.delay == C.n_noise_filters - 2 == dec.noise.stream_delay
    assert (live.noise_state == 0).all()                          # the warm-up and the capture left no trace
    rng = np.random.default_rng(8)
    hidden = torch.zeros(1, 1, C.decoder_gru_units, device="cuda")
    state = ddsp.ola_stream_state(1, C.n_noise_filters, "cuda")
    for call in range(3):
        z = {"normalized_cents": rng.uniform(0, 1, (1, 1, 1)).astype(np.float32),
             "loudness": rng.uniform(-1, 1, (1, 1, 1)).astype(np.float32),
             "f0": rng.uniform(150, 400, (1, 1, 1)).astype(np.float32)}
        zc = {k: torch.from_numpy(v).cuda() for k, v in z.items()}
        with torch.no_grad():
            got, _ = dec.forward_live(zc, hidden, delayed=True)
            ctrl, _ = hand.controller(zc, hidden)
            out, state = ddsp.noise_ola_stream(ctrl["H"], C.hop_length, state, dry=hand.harmonics.live(ctrl), seed=SEED,
                                               offset=call * quads(C.hop_length))
            want = hand.reverb.live_forward(out).cpu().squeeze(0).numpy()
        assert got.shape == (C.hop_length,) and np.array_equal(got.view(np.int32), want.view(np.int32)), call
        replay = live.run(z)
        err = np.max(np.abs(replay - got))
        print(f"callback {call}: |graph - eager| = {err:.2e}")
        assert replay.shape == got.shape and err <= 1e-6, call
    assert torch.allclose(live.noise_state, dec.noise._stream_state, rtol=0, atol=1e-6)


def test_the_graphed_live_pass_replays_the_stream():
    C = type("SynthConf", (), dict(n_harmonics=8, sample_rate=16000, hop_length=64, noise_overlap_add=True))
    B, T, F = 2, 2, 65
    synth = ddsp.GraphedSynth(C, B, T, F, live=True, noise_seed=SEED, delayed=True)
    assert synth.delay == F - 2 and (synth.noise_state == 0).all()
    gen = torch.Generator("cuda").manual_seed(2)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)           # noqa: E731
    state, phases = ddsp.ola_stream_state(B, F, "cuda"), torch.zeros(C.n_harmonics, device="cuda")
    for call in range(3):
        ctrl = dict(f0=100.0 + 300.0 * rand(B, T, 1), c=rand(B, T, C.n_harmonics) / C.n_harmonics, a=rand(B, T, 1), H=0.1 * rand(B, T, F))
        y = synth(ctrl).clone()
        dry, phases, _ = ddsp.osc_forward(ctrl["f0"], ctrl["c"], ctrl["a"], C.hop_length, C.sample_rate, live_in=phases, want_live_out=True)
        want, state = ddsp.noise_ola_stream(ctrl["H"], C.hop_length, state, dry=dry, seed=SEED, offset=call * B * T * quads(C.hop_length))
        assert same_bits(y, want), call
    assert same_bits(synth.noise_state, state)
