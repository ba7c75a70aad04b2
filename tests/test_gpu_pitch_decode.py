"""The pitch decoders on the device (csrc/ddsp_pitch.hip) against the fp64 oracle of tests/pitch_decode_reference.py.

Tolerances.  Centered: the kernel's only fp32 quantity is the offset 20 (sum i w_i) / (sum w_i) (|offset| <= 80, nine-term
sums: ~1e-5 cents); cents, f0 and the normalised cents are formed from it in fp64 and rounded once, and the cents are read
back from the fp32 f0 (half an ulp = 5e-5 cents).  The bounds are the ones the definitions allow for an all-fp32 kernel:
cents 1e-3 (one fp32 rounding at 8000 cents is 2.4e-4, the offset adds ~1e-4), f0 2e-6 relative (5.8e-4 per cent times
1e-3, plus the exponential), normalised cents 3e-7; harmonicity is a gather, bit-exact.
Viterbi: the fp32 recurrence rounds three times per step at magnitudes below ~160 on near-optimal states, so the device
path's fp64 score is within 2e-4 T of the optimum (one wrong predecessor costs at least log(12 / 11) = 0.087); the path
itself may differ from the oracle's on at most 1 % of the frames (near-ties)."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import pitch_decode_reference as ref
from conftest import load_golden
from encoder_common import Conf, AEConf, crepe_weights

pytestmark = pytest.mark.gpu

SHARE_CAP = 0.01


@pytest.fixture(scope="module")
def log_a():
    return ref.log_transition()


def _check_centered(out, centre, p):
    """out = (f0, harmonicity, normalized_cents) [..., 1] from the device, centre [...] and p [..., 360] numpy, finite rows"""
    f, h, n = (v[..., 0].cpu().numpy() for v in out)
    want = ref.centered(centre, p)
    cents = 1200 * np.log2(f.astype(np.float64) / 10)
    assert np.abs(cents - want["cents"]).max() <= 1e-3, np.abs(cents - want["cents"]).max()
    assert np.abs(f / want["f0"] - 1).max() <= 2e-6
    assert np.abs(n - want["normalized_cents"]).max() <= 3e-7
    assert np.array_equal(h, np.take_along_axis(p, np.asarray(centre)[..., None], axis=-1)[..., 0])


def _check_paths(bins, rows, log_a):
    """bins [B, T] numpy from the device, rows the B inputs [T, 360]"""
    for r, p in enumerate(rows):
        T = p.shape[0]
        path, _ = ref.viterbi(p, None, log_a)
        got = bins[r]
        assert got.min() >= 0 and got.max() <= 359
        if T > 1:
            assert np.abs(np.diff(got)).max() <= 11
        gap = ref.path_score(path, p, log_a) - ref.path_score(got, p, log_a)
        share = float((got != path).mean())
        assert 0 <= gap <= 2e-4 * T, (r, T, gap)
        assert share <= SHARE_CAP, (r, T, share)


CENTRES = [0, 1, 3, 4, 180, 355, 356, 358, 359]


def test_centered_given_centres_at_both_edges():
    p = np.random.default_rng(3).random((2, len(CENTRES), 360), dtype=np.float32)
    c = np.array([CENTRES, CENTRES[::-1]])
    out = ddsp.pitch_centered(torch.from_numpy(c)[..., None].cuda(), torch.from_numpy(p).cuda())
    assert all(tuple(v.shape) == (2, 9, 1) and v.dtype == torch.float32 for v in out)
    _check_centered(out, c, p)


def test_centered_own_argmax_with_nan_frame_and_ties():
    p = np.random.default_rng(4).random((3, 37, 360), dtype=np.float32)
    for k, b in enumerate(CENTRES):                         # the maximum at both edges, and a tie (the lower bin wins)
        p[0, k, b] = 1.5
    p[1, 0, 200] = p[1, 0, 100] = 2.0
    p[2, 5] = np.nan                                        # all NaN: bin 0, NaN outputs
    p[2, 6, 300] = np.nan                                   # one NaN: it is the maximum
    dev = torch.from_numpy(p).cuda()
    f, h, n, bins = ddsp.encoder._centered_device(None, dev)
    bins = bins.cpu().numpy()
    want_bins = torch.from_numpy(p).argmax(dim=-1).numpy()
    assert np.array_equal(bins, want_bins) and bins[1, 0] == 100 and bins[2, 5] == 0 and bins[2, 6] == 300
    assert list(bins[0, :len(CENTRES)]) == CENTRES
    bad = np.isnan(p).any(axis=-1)
    for v in (f, h, n):
        assert np.isnan(v[..., 0].cpu().numpy()[bad]).all()
    ok = ~bad
    _check_centered([v[torch.from_numpy(ok).cuda()] for v in (f, h, n)], bins[ok], p[ok])
    again = ddsp.pitch_weighted(dev)
    assert all(torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) for a, b in zip(again, (f, h, n)))
    am = ddsp.pitch_argmax(dev[:2])                         # the reference's forward decode from the same bins
    cpu = ddsp.pitch_argmax(torch.from_numpy(p[:2]))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(am, cpu))


@pytest.mark.parametrize("kind", ["track", "rand"])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (3, 3), (2, 13), (3, 64), (2, 172)])
def test_viterbi_matches_oracle(B, T, kind, log_a):
    rows = [ref.make(kind, 1000 * T + 10 * B + r, T) for r in range(B)]
    bins = ddsp.pitch_viterbi(torch.from_numpy(np.stack(rows)).cuda())
    assert bins.dtype == torch.int64 and tuple(bins.shape) == (B, T, 1)
    _check_paths(bins[..., 0].cpu().numpy(), rows, log_a)


@pytest.mark.parametrize("kind", ["track", "rand"])
def test_viterbi_long_row_uses_the_workspace(kind, log_a):
    assert ddsp._lib.lib().ddsp_pitch_viterbi_workspace_bytes(1, 500) == 500 * 360          # back-pointers beyond LDS
    assert ddsp._lib.lib().ddsp_pitch_viterbi_workspace_bytes(1, 172) == 0
    rows = [ref.make(kind, 500, 500)]
    bins = ddsp.pitch_viterbi(torch.from_numpy(np.stack(rows)).cuda())
    _check_paths(bins[..., 0].cpu().numpy(), rows, log_a)


def test_viterbi_tie_rule():
    flat = torch.full((1, 1, 360), 0.25, device="cuda")
    assert int(ddsp.pitch_viterbi(flat)[0, 0, 0]) == 0


def test_viterbi_state_carries_the_recurrence():
    p = torch.from_numpy(np.stack([ref.make("track", 5, 64), ref.make("rand", 6, 64)])).cuda()
    whole, last = ddsp.pitch_viterbi(p, return_state=True)
    _, mid = ddsp.pitch_viterbi(p[:, :32], return_state=True)
    second, last2 = ddsp.pitch_viterbi(p[:, 32:], state=mid)
    assert tuple(last.shape) == (2, 360) and last.dtype == torch.float32
    a = last - last.max(dim=-1, keepdim=True).values
    b = last2 - last2.max(dim=-1, keepdim=True).values
    assert (a - b).abs().max().item() <= 1e-4
    assert torch.equal(second[:, -1], whole[:, -1])
    # the CPU branch carries the same scores
    _, cpu = ddsp.pitch_viterbi(p.cpu(), return_state=True)
    assert (a.cpu() - cpu).abs().max().item() <= 2e-4 * 64


def test_deterministic_rows_independent_and_capturable():
    p = torch.from_numpy(np.stack([ref.make("track", 21, 172), ref.make("rand", 22, 172), ref.make("track", 23, 172)])).cuda()

    def run(x):
        bins, state = ddsp.pitch_viterbi(x, return_state=True)
        return (bins, state) + tuple(ddsp.pitch_centered(bins, x))

    first, second, alone = run(p), run(p), run(p[1:2].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.equal(a[1:2], b) for a, b in zip(first, alone))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(p)                                              # warm-up on the capture stream (tables, one-time attribute calls)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = run(p)
    torch.cuda.current_stream().wait_stream(side)
    for v in captured:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, captured))


def test_silent_row_beside_a_normal_one():
    normal = torch.from_numpy(ref.make("track", 31, 64)).cuda()
    p = torch.stack([normal, torch.full_like(normal, float("nan"))])
    bins = ddsp.pitch_viterbi(p)
    f, h, n = ddsp.pitch_centered(bins, p)
    one = ddsp.pitch_viterbi(p[:1].contiguous())
    assert torch.equal(bins[:1], one)
    assert all(torch.equal(a[:1], b) for a, b in zip((f, h, n), ddsp.pitch_centered(one, p[:1].contiguous())))
    assert int(bins[1].min()) >= 0 and int(bins[1].max()) <= 359
    assert torch.isnan(f[1]).all() and torch.isnan(h[1]).all()
    assert torch.isfinite(f[0]).all()


@pytest.mark.parametrize("decoder", ["viterbi", "weighted"])
def test_f0_encoder_decodes_its_own_probabilities(decoder, log_a):
    g = load_golden("g21_f0_tiny")
    enc = ddsp.F0Encoder(Conf(44100, 2048, 512), weights=crepe_weights("tiny", g["crepe_seed"]), decoder=decoder).cuda()
    for tag in ("clips", "live"):
        f, h, probs, n = enc(torch.from_numpy(g[f"{tag}_x"]).cuda())
        assert probs.shape == g[f"{tag}_probabilities"].shape and f.shape == h.shape == n.shape == g[f"{tag}_f0"].shape
        p = probs.cpu().numpy()
        if decoder == "viterbi":
            centre = np.stack([ref.viterbi(row, None, log_a)[0] for row in p])
            dev_bins = ddsp.pitch_viterbi(probs)[..., 0].cpu().numpy()
            _check_paths(dev_bins, list(p), log_a)
            same = dev_bins == centre
        else:
            centre = p.argmax(axis=-1)
            same = np.ones(centre.shape, dtype=bool)
        assert same.mean() >= 1 - SHARE_CAP
        _check_centered([v[torch.from_numpy(same).cuda()] for v in (f, h, n)], centre[same], p[same])


def test_autoencoder_follows_conf_pitch_decoder():
    g = load_golden("g24_autoencoder_forward")
    w = crepe_weights("tiny", g["crepe_seed"])
    decoder_state = {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("dw__")}

    class ViterbiConf(AEConf):
        pitch_decoder = "viterbi"

    class ArgmaxConf(AEConf):
        pitch_decoder = "argmax"

    x = torch.from_numpy(g["x"]).cuda()
    out = {}
    for name, conf in (("default", AEConf), ("argmax", ArgmaxConf), ("viterbi", ViterbiConf)):
        ae = ddsp.AutoEncoder(conf, weights=w)
        ae.decoder.load_state_dict(decoder_state, strict=True)
        ae = ae.eval().cuda()
        with torch.no_grad():
            torch.manual_seed(77)
            out[name] = ae(x)
    assert torch.equal(out["default"], out["argmax"])
    assert out["viterbi"].shape == out["default"].shape and torch.isfinite(out["viterbi"]).all()
    assert not torch.equal(out["viterbi"], out["default"])
