"""Griffin-Lim on the CPU (no GPU needed): ddsp_pytorch_amd.griffinlim's stock-torch branch against the G27 fixtures
(tools/make_griffinlim_goldens.py: a labelled restatement of torchaudio 0.8.1's functional.griffinlim), bit for bit; the
checks that raise before any work; the seeded random start; the HIP dispatch table."""
import hashlib
import math

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import spectral

CASES = ["n2048_h256", "n1024_h128_p2", "n512_h64", "n512_w400_h100"]
N_ITERS = (0, 1, 4, 16)


def _args(g):
    n_fft, hop, win_length, length = (int(v) for v in g["params"])
    return dict(n_fft=n_fft, hop_length=hop, win_length=win_length, power=float(g["power"]), momentum=float(g["momentum"]),
                length=None if length < 0 else length, rand_init=False)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", ["32", "64"])
def test_cpu_branch_matches_g27(golden, case, dtype):
    g = golden("g27_" + case)
    spec, window, angles = (torch.from_numpy(g[k]) for k in ("spec", "window", "angles"))
    if dtype == "64":
        spec, window = spec.double(), window.double()
    for n in N_ITERS:
        y = ddsp.griffinlim(spec, window, n_iter=n, angles=angles, **_args(g))
        ref = g[f"y{dtype}_{n}"]
        assert y.dtype == torch.from_numpy(ref).dtype and tuple(y.shape) == ref.shape, (case, n)
        assert np.array_equal(y.numpy(), ref), (case, dtype, n, float(np.abs(y.numpy() - ref).max()))


def _small(n_fft=256, hop=64, frames=9, lead=(2,)):
    torch.manual_seed(0)
    return torch.rand(*lead, n_fft // 2 + 1, frames), torch.hann_window(n_fft)


def test_momentum_out_of_range_raises():
    spec, w = _small()
    for m in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 2, m, None, False)


def test_length_frame_mismatch_raises():
    spec, w = _small(frames=9)
    ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 1, 0.0, 8 * 64 + 63, False)      # 1 + 575 // 64 == 9: accepted
    for length in (7 * 64, 9 * 64, 100):
        with pytest.raises(ValueError, match="frames"):
            ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 1, 0.0, length, False)


def test_nola_violation_raises_once_before_work():
    spec, _ = _small(n_fft=256, hop=128, frames=9)
    w = torch.zeros(256)
    w[:64] = 1.0                                                   # frames 128 apart, window support 64: gaps in the envelope
    with pytest.raises(RuntimeError, match="window overlap add min"):
        ddsp.griffinlim(spec, w, 256, 128, 256, 1.0, 0, 0.0, None, False)


def test_too_short_for_reflect_padding_raises():
    spec, w = _small(n_fft=256, hop=64, frames=2)                  # 64 samples, reflect padding needs more than 128
    with pytest.raises(ValueError, match="too short"):
        ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 1, 0.0, None, False)


def test_bad_shape_raises():
    spec, w = _small()
    with pytest.raises(ValueError, match="specgram"):
        ddsp.griffinlim(spec[:, :-1], w, 256, 64, 256, 1.0, 1, 0.0, None, False)


def test_requires_grad_refused():
    spec, w = _small()
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.griffinlim(spec.requires_grad_(), w, 256, 64, 256, 1.0, 1, 0.0, None, False)


def test_rand_init_seeded_reproducible_and_unit_modulus():
    spec, w = _small()
    a = ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 3, 0.99, None, True, generator=torch.Generator().manual_seed(5))
    b = ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 3, 0.99, None, True, generator=torch.Generator().manual_seed(5))
    c = ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 3, 0.99, None, True, generator=torch.Generator().manual_seed(6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the start is 0.8.1's draw: 2 pi rand(batch, F, T) from the generator, as unit-modulus angles
    batch, freq, frames = spec.shape
    ang = spectral._initial_angles(batch, freq, frames, True, torch.Generator().manual_seed(5), None, spec.shape,
                                   torch.float32, torch.device("cpu"))
    phase = 2 * math.pi * torch.rand(batch, freq, frames, generator=torch.Generator().manual_seed(5))
    assert torch.equal(ang, torch.stack([phase.cos(), phase.sin()], dim=-1))
    assert torch.allclose(ang.pow(2).sum(-1), torch.ones(batch, freq, frames), atol=1e-6)
    # global generator by default
    torch.manual_seed(11)
    d = ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 3, 0.99, None, True)
    torch.manual_seed(11)
    assert torch.equal(d, ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 3, 0.99, None, True))
    # rand_init=False: every angle is 1, the same as explicit unit angles
    ones = torch.ones(spec.shape, dtype=torch.complex64)
    assert torch.equal(ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 2, 0.5, None, False),
                       ddsp.griffinlim(spec, w, 256, 64, 256, 1.0, 2, 0.5, None, True, angles=ones))


def test_leading_dims_round_trip():
    spec, w = _small(lead=(2, 3))
    y = ddsp.griffinlim(spec, w, 256, 64, 256, 2.0, 2, 0.9, None, False)
    assert y.shape == (2, 3, 8 * 64)
    flat = ddsp.griffinlim(spec.reshape(6, *spec.shape[-2:]), w, 256, 64, 256, 2.0, 2, 0.9, None, False)
    assert torch.equal(y.reshape(6, -1), flat)


def test_hip_dispatch_table():
    cuda, cpu = torch.device("cuda", 0), torch.device("cpu")
    for n_fft in (64, 128, 256, 512, 1024, 2048):
        assert spectral.griffinlim_uses_hip(cuda, torch.float32, n_fft, n_fft)
        assert spectral.griffinlim_uses_hip(cuda, torch.float32, n_fft, n_fft // 2)
        assert not spectral.griffinlim_uses_hip(cuda, torch.float64, n_fft, n_fft)
        assert not spectral.griffinlim_uses_hip(cpu, torch.float32, n_fft, n_fft)
    for n_fft in (32, 1000, 4096, 3 * 512):
        assert not spectral.griffinlim_uses_hip(cuda, torch.float32, n_fft, n_fft)
    assert not spectral.griffinlim_uses_hip(cuda, torch.float32, 512, 1024)


def test_window_envelope_matches_istft():
    n_fft, hop, frames = 512, 100, 12
    w = spectral._padded_window(torch.hann_window(400), n_fft, 400)
    env = spectral.window_envelope(w, n_fft, hop, frames, None)
    # istft of all-ones frames of the window: y * env = the overlap-add of w^2 ... recover env as istft(ones) = 1 where defined
    full = n_fft + hop * (frames - 1)
    ref = torch.zeros(full)
    for t in range(frames):
        ref[t * hop:t * hop + n_fft] += w.pow(2)
    assert torch.allclose(env, ref[n_fft // 2:n_fft // 2 + hop * (frames - 1)], rtol=1e-6, atol=0)


# ---- G28: style transfer (tools/make_style_goldens.py runs the reference's style_transfer.py) ---------------------------------
@pytest.fixture()
def native_cpu_conv():
    prev, threads = torch.backends.mkldnn.enabled, torch.get_num_threads()
    torch.backends.mkldnn.enabled = False          # the fixtures' CPU convolution path (tools/make_style_goldens.py): native
    torch.set_num_threads(1)                       # im2col + BLAS on one thread, whose blocking does not depend on the host
    yield
    torch.backends.mkldnn.enabled = prev
    torch.set_num_threads(threads)


def _assert_digest(a, g, name):
    """`a` is bit for bit the array G28 records as `name` (tools/make_style_goldens.py: SHA-256 of the C-ordered bytes)."""
    a = np.ascontiguousarray(a)
    assert a.shape == tuple(g[name + "_shape"]) and a.dtype.str == str(g[name + "_dtype"]), (name, a.shape, a.dtype)
    assert hashlib.sha256(a.tobytes()).hexdigest() == str(g[name + "_sha256"]), (
        name, "sum", float(a.astype(np.float64).sum()), float(g[name + "_sum"]), "absmax", float(np.abs(a).max()),
        float(g[name + "_absmax"]))


def test_prepare_spectra_matches_g28(golden):
    g = golden("g28_style")
    sr, win, hop = (int(v) for v in g["params"][:3])
    db, n = ddsp.prepare_spectra(g["content_audio"], sr, win, hop)
    assert db.dtype == np.float32 and n == int(g["content_length"])
    _assert_digest(db, g, "content_db")
    db_s, _ = ddsp.prepare_spectra(torch.from_numpy(g["style_audio"]), sr, win, hop)
    _assert_digest(db_s, g, "style_db")
    assert np.mean(db) == g["elem_mean"] and np.std(db) == g["elem_std"]
    with pytest.raises(ValueError):
        ddsp.prepare_spectra(g["content_audio"][:win // 2], sr, win, hop)


def test_features_gram_losses_match_g28(golden, native_cpu_conv):
    g = golden("g28_style")
    sr, win, hop, n_feat, ksize = (int(v) for v in g["params"])
    length, offset = (int(v) for v in g["trim"])
    content_db, _ = ddsp.prepare_spectra(g["content_audio"], sr, win, hop)
    style_db, _ = ddsp.prepare_spectra(g["style_audio"], sr, win, hop)
    mean, std = np.mean(content_db), np.std(content_db)
    assert min(content_db.shape[1], style_db.shape[1]) == length and style_db.shape[1] // 8 == offset
    content = torch.from_numpy(np.ascontiguousarray(((content_db - mean) / std)[:, :length])).unsqueeze(0)
    style = torch.from_numpy(np.ascontiguousarray(((style_db - mean) / std)[:, offset:offset + 4 * length])).unsqueeze(0)
    torch.manual_seed(28)
    fe = ddsp.FeatureExtractor(content.shape[1], n_feat, ksize)
    _assert_digest(fe.conv_kernel.numpy(), g, "conv_kernel")
    with torch.no_grad():
        cf, sf = fe(content), fe(style)
    _assert_digest(cf.numpy(), g, "content_features")
    _assert_digest(sf.numpy(), g, "style_features")
    _assert_digest(ddsp.gram_matrix(cf).numpy(), g, "gram_content")
    sl, cl = ddsp.StyleLoss(sf), ddsp.ContentLoss(cf)
    _assert_digest(sl.target.numpy(), g, "gram_style")
    with torch.no_grad():
        sl(content_f := fe(content))
        cl(content_f)
    assert float(sl.loss) == float(g["style_loss0"]) and float(cl.loss) == float(g["content_loss0"])


def test_style_transfer_matches_g28(golden, native_cpu_conv):
    """style_transfer end to end on the CPU against the reference's main() (3 LBFGS iterations, then the Griffin-Lim end)."""
    g = golden("g28_style")
    sr, win, hop, n_feat, ksize = (int(v) for v in g["params"])
    gl_iter, gl_seed = (int(v) for v in g["gl"])
    stats = {}
    torch.manual_seed(28)
    y = ddsp.style_transfer(g["content_audio"], g["style_audio"], sample_rate=sr, win_length=win, hop_length=hop, n_features=n_feat,
                            kernel_size=ksize, max_iter=3, gl_iter=gl_iter, device="cpu",
                            generator=torch.Generator().manual_seed(gl_seed), stats=stats)
    assert stats["losses"] == [float(v) for v in g["lbfgs_losses"]]
    assert y.shape == (int(g["content_length"]),)
    _assert_digest(y, g, "result")
    assert float(np.max(np.abs(y))) == 1.0
    # helper.py's variant: hop * (frames - 1) samples
    torch.manual_seed(28)
    y2 = ddsp.style_transfer(g["content_audio"], g["style_audio"], sample_rate=sr, win_length=win, hop_length=hop, n_features=n_feat,
                             kernel_size=ksize, max_iter=1, gl_iter=1, length=None, device="cpu")
    assert y2.shape == (hop * (int(g["content_db_shape"][1]) - 1),)
