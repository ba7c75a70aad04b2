"""CPU checks of the audio encoder (encoder.py / autoencoder.py): the stock-torch branch against the reference's own code
(fixtures G19-G25, tools/make_encoder_goldens.py) bit for bit, checkpoint compatibility, host tables, hop / length arithmetic
and refusals, and the new C entry points' argument validation.  The resampler kernel and the A-weighting table are
restatements of torchaudio / librosa (their parity with those libraries is not pinned here)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddsp_pytorch_amd as ddsp
from conftest import load_golden
from encoder_common import Conf, AEConf, crepe_weights, f0_encoder, autoencoder, loud_conf


@pytest.fixture(autouse=True)
def _native_conv():
    # the fixtures were captured with CPU convolutions on the native im2col + BLAS path (oneDNN's kernels depend on the ISA)
    with torch.backends.mkldnn.flags(enabled=False):
        yield


def test_loudness_cpu_matches_reference_bit_for_bit():
    g = load_golden("g19_loudness")
    for tag in ("a", "b"):
        enc = ddsp.LoudnessEncoder(loud_conf(g, tag))
        assert np.array_equal(enc.a_weight.detach().numpy(), g[f"{tag}_a_weight"])
        assert enc.a_weight.detach().numpy()[0] == -80.0 and not enc.a_weight.requires_grad
        assert np.array_equal(enc(torch.from_numpy(g[f"{tag}_x"])).numpy(), g[f"{tag}_loudness"]), tag


def test_resampler_cpu_matches_fixture_and_support_table():
    g = load_golden("g20_resample")
    for tag in ("a", "b"):
        rs = ddsp.encoder.Resample(int(g[f"{tag}_rate"]), 16000)
        y = rs(torch.from_numpy(g[f"{tag}_x"])).numpy()
        assert np.array_equal(y, g[f"{tag}_y"]), tag
    kernel, width, o, n = ddsp.encoder.sinc_resample_kernel(44100, 16000)
    assert (o, n, width) == (441, 160, 17) and kernel.shape == (160, 1, 475)
    table, first, K = ddsp.encoder.support_taps(44100, 16000)
    assert K == 34 and table.shape == (160, 34)
    # what the device table drops is the clamped window's residue only
    full = kernel[:, 0].clone()
    for r in range(160):
        full[r, int(first[r]) + width:int(first[r]) + width + K] = 0
    assert float(full.abs().max()) <= 1.8e-24
    # the table-based sum equals the full polyphase matrix on the fixture to float rounding
    x = torch.from_numpy(g["a_x"]).double()
    xp = F.pad(x, (width, width + o))
    L = x.shape[1]
    j = torch.arange(int(np.ceil(n * L / o)))
    win = (j // n)[:, None] * o + torch.arange(475)[None]
    ref = (xp[:, win] * kernel[:, 0].double()[j % n]).sum(-1)
    assert float((ref - torch.from_numpy(g["a_y"]).double()).abs().max()) <= 1e-6


def test_equal_rates_are_identity():
    rs = ddsp.encoder.Resample(16000, 16000)
    x = torch.randn(2, 100)
    assert rs(x) is x and not hasattr(rs, "kernel")


@pytest.mark.parametrize("name,capacity,conf", [("g21_f0_tiny", "tiny", Conf(44100, 2048, 512)),
                                                ("g22_f0_full", "full", Conf(16000, 1024, 256, "full"))])
def test_f0_encoder_cpu_matches_reference_bit_for_bit(name, capacity, conf):
    g = load_golden(name)
    enc = f0_encoder(g, conf)
    tags = ("clips", "live", "silent") if capacity == "tiny" else ("",)
    for tag in tags:
        p = f"{tag}_" if tag else ""
        f, h, probs, c = enc(torch.from_numpy(g[p + "x"]))
        for k, v in (("f0", f), ("harmonicity", h), ("probabilities", probs), ("normalized_cents", c)):
            assert v.shape == g[p + k].shape, (tag, k)
            assert np.array_equal(v.numpy(), g[p + k], equal_nan=True), (tag, k)
    if capacity == "tiny":     # the silent window: NaN probabilities, bin 0
        assert np.all(np.isnan(g["silent_probabilities"])) and np.all(g["silent_normalized_cents"] == 0)
        assert np.allclose(g["silent_f0"], 31.7, atol=0.05)


def test_encoder_state_dict_matches_reference_and_loads_crepe_pth(tmp_path):
    g = load_golden("g23_encoder_state_keys")
    for cap in ("tiny", "full"):
        enc = ddsp.Encoder(Conf(44100, 2048, 512, cap), weights=crepe_weights(cap, 0))
        sd = enc.state_dict()
        assert list(sd) == list(g[f"{cap}_keys"])
        assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(g[f"{cap}_shapes"])
        assert len(sd) == 45
        # a reference-format CREPE .pth (the keys of crepe/crepe.py) loads with strict=True from a path
        path = os.path.join(tmp_path, f"{cap}.pth")
        torch.save(crepe_weights(cap, 5), path)
        f0 = ddsp.F0Encoder(Conf(44100, 2048, 512, cap), weights=path)
        assert torch.equal(f0.model.conv3.weight, crepe_weights(cap, 5)["conv3.weight"])


def test_crepe_weights_are_required():
    with pytest.raises(ValueError, match="CREPE weights"):
        ddsp.F0Encoder(Conf(44100, 2048, 512))
    c = Conf(44100, 2048, 512)
    c.crepe_weights = crepe_weights("tiny", 1)
    assert ddsp.F0Encoder(c).model.capacity == "tiny"
    with pytest.raises(ValueError):
        ddsp.Crepe("small")


def test_pitch_tables_equal_reference_ops():
    f0_table, cents_table = ddsp.encoder.pitch_tables()
    assert f0_table.dtype == cents_table.dtype == torch.float32
    for shape in ((360,), (2, 180, 1), (360, 1, 1)):
        bins = torch.arange(360).reshape(shape)
        freq = 10 * 2 ** ((bins * 20 + 1997.3794084376191) / 1200)      # encoder.py:41-50, 120-128
        assert torch.equal(freq.flatten(), f0_table) and torch.equal((bins / 359.).flatten(), cents_table)
    assert abs(float(f0_table[0]) - 31.7) < 0.05


def test_hop_arithmetic_and_short_inputs():
    enc = ddsp.F0Encoder(Conf(44100, 2048, 512), weights=crepe_weights("tiny", 1))
    assert enc.resampled_hop(3584, 1301) == int(512 * ((1301 - 1024) / (3584 - 2048))) == 92
    assert ddsp.encoder.resampled_length(3584, 44100, 16000) == 1301
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 2048))                        # L == n_fft: the reference divides by zero
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 2600))                        # fewer than 1024 samples at 16 kHz
    with pytest.raises(ValueError):
        ddsp.LoudnessEncoder(Conf(44100, 2048, 512))(torch.zeros(1, 2000))
    with pytest.raises(RuntimeError, match="no backward"):
        enc(torch.zeros(1, 4096, requires_grad=True))
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.LoudnessEncoder(Conf(44100, 2048, 512))(torch.zeros(1, 4096, requires_grad=True))


@pytest.mark.parametrize("name", ["g24_autoencoder_forward", "g25_autoencoder_live"])
def test_autoencoder_front_matches_reference(name):
    """The encoder half of AutoEncoder.forward / forward_live (padding, trimming, Encoder) on the CPU against the features
    the reference fed its decoder; the decoder's synthesis is device-only (tests/test_gpu_encoder.py)."""
    g = load_golden(name)
    ae = autoencoder(g)
    sd = ae.state_dict()
    assert "encoder.f0_encoder.model.conv1.weight" in sd and "encoder.loudness_encoder.a_weight" in sd and "decoder.reverb.noise" in sd
    if name.startswith("g24"):
        p = ae.padding
        assert p == 1536
        z = ae.encoder(F.pad(torch.from_numpy(g["x"]), (p // 2, p - p // 2)))
        cases = [(z, "z_")]
    else:
        cases = []
        for call in range(3):
            w = ae.live_window(g[f"x_{call}"])
            assert w.shape == (1, 3584)
            cases.append((ae.encoder(w), f"z{call}_"))
    for z, pre in cases:
        assert z["f0"].shape[1] == z["loudness"].shape[1]
        for k, v in z.items():
            assert np.array_equal(v.numpy(), g[pre + k]), (pre, k)


def test_encoder_entry_points_validate_without_gpu():
    L = ddsp._lib.lib()
    assert L.ddsp_resample(None, None, None, None, 1, 100, 441, 160, 34, None) == -1
    assert L.ddsp_resample(None, None, None, None, 0, 100, 441, 160, 34, None) == 0
    assert L.ddsp_crepe_frames(None, None, None, 1, 2000, 92, 4, None) == -1
    assert L.ddsp_crepe_epilogue(None, None, None, None, None, None, None, 4, 16, 256, 0, None) == -1
    assert L.ddsp_pitch_decode(None, None, None, None, None, None, None, None, 4, None) == -1
    assert L.ddsp_loudness(None, None, None, 1, 4096, 2048, 512, None) == -1
    assert L.ddsp_loudness_supported(2048) == 1 and L.ddsp_loudness_supported(64) == 1
    assert L.ddsp_loudness_supported(3000) == 0 and L.ddsp_loudness_supported(4096) == 0 and L.ddsp_loudness_supported(32) == 0
