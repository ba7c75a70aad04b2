"""The MFCC front end and the timbre latent without a GPU: the CPU path of `mfcc` against the fp64 restatement
(tests/mfcc_reference.py), the filterbank's sparse form, ddsp_mfcc's argument checks, and the state-dict contract of the
opt-in `z_dims` (absent or 0: nothing changes)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import encoder as enc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfcc_reference as ref  # noqa: E402


class Conf:
    n_fft, hop_length, sample_rate = 256, 64, 16000
    n_harmonics, n_noise_filters = 16, 17
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 3, 64, 1
    crepe, pitch_tracker = 'tiny', 'yin'


class ConfZ0(Conf):
    z_dims = 0


class ConfZ(Conf):
    z_dims, z_gru_units = 4, 64


# ------------------------------------------------------------------------------------------------------- CPU path vs fp64

def test_cpu_path_meets_the_recorded_constant():
    """Every input of the MFCC tests but the long one: |fp32 torch evaluation - fp64| <= C_CPU x the element's bound."""
    worst = (0.0, None)
    for name, x, n_fft, hop, pairs in ref.cases():
        spec = ref.spectrum(x, n_fft, hop)
        for n_mels, n_mfcc in pairs:
            want = ref.from_spectrum(spec, n_fft, ref.SAMPLE_RATE, n_mels, n_mfcc)
            got, lm = ddsp.mfcc(torch.from_numpy(x), n_fft, hop, ref.SAMPLE_RATE, n_mels=n_mels, n_mfcc=n_mfcc, return_logmel=True)
            assert got.dtype == lm.dtype == torch.float32
            r, where = ref.worst_ratio(got.numpy(), lm.numpy(), want)
            if r > worst[0]:
                worst = (r, (name, n_mels, n_mfcc, where))
    print("CPU path: worst |error| / bound(c = 1) =", worst)
    assert worst[0] <= ref.C_CPU, worst


def test_cpu_path_zero_frame_and_defaults():
    x = torch.from_numpy(ref.content_inputs(256)["zero_beside_loud"])
    out, lm = ddsp.mfcc(x, 256, 256, 16000, return_logmel=True)
    assert out.shape == (2, 3, 30) and lm.shape == (2, 3, 128)
    floor = np.log(np.float64(np.float32(1e-5)))
    assert np.allclose(lm[0, 1].numpy(), floor, rtol=1e-6) and np.allclose(lm[1, 0].numpy(), floor, rtol=1e-6)
    assert torch.equal(ddsp.mfcc(x, 256, 256, 16000), out)
    with pytest.raises(ValueError):
        ddsp.mfcc(x, 96, 64, 16000)
    with pytest.raises(ValueError):
        ddsp.mfcc(x, 256, 0, 16000)
    with pytest.raises(ValueError):
        ddsp.mfcc(x, 256, 64, 16000, n_mels=129)
    with pytest.raises(ValueError):
        ddsp.mfcc(x, 256, 64, 16000, n_mels=128, n_mfcc=65)
    with pytest.raises(ValueError):
        ddsp.mfcc(x, 256, 64, 16000, n_mels=8, n_mfcc=9)
    with pytest.raises(ValueError):
        ddsp.mfcc(x[:, :100], 256, 64, 16000)
    y = x.clone().requires_grad_(True)                     # detached, as the docstring says: no gradient, no refusal
    assert not ddsp.mfcc(y, 256, 256, 16000).requires_grad


# ------------------------------------------------------------------------------------------------------------------ tables

@pytest.mark.parametrize("n_fft,rate,n_mels,fmin,fmax", [(64, 16000, 128, 20.0, 8000.0), (2048, 44100, 128, 20.0, 8000.0),
                                                        (256, 16000, 40, 20.0, 8000.0), (512, 8000, 8, 50.0, 8000.0),
                                                        (1024, 48000, 128, 0.0, 30000.0)])
def test_sparse_filterbank_expands_to_the_dense_definition(n_fft, rate, n_mels, fmin, fmax):
    dense, start, count, band_w = enc.mel_filterbank(n_fft, rate, n_mels, fmin, fmax)
    want = ref.filterbank(n_fft, rate, n_mels, fmin, fmax)
    assert dense.dtype == torch.float32 and np.array_equal(dense.numpy().view(np.uint32), want.view(np.uint32))
    assert start.dtype == count.dtype == torch.int32
    rebuilt = np.zeros_like(want)
    o = 0
    for m in range(n_mels):
        s, c = int(start[m]), int(count[m])
        assert 0 <= s and s + c <= n_fft // 2 + 1
        rebuilt[m, s:s + c] = band_w[o:o + c].numpy()
        if c:
            assert rebuilt[m, s] != 0 and rebuilt[m, s + c - 1] != 0 and s >= 1       # a tight run; bin 0 has weight 0
        o += c
    assert o == int(count.sum()) and (o == band_w.numel() or (o == 0 and band_w.numel() == 1))
    assert np.array_equal(rebuilt.view(np.uint32), want.view(np.uint32))
    assert np.all(want[:, 0] == 0) and np.all(want >= 0) and np.all(want <= 1)


def test_bands_that_cover_no_bin_and_clamped_fmax():
    # 128 bands on 33 bins: the low bands are narrower than a bin
    _, start, count, _ = enc.mel_filterbank(64, 16000, 128, 20.0, 8000.0)
    assert int((count == 0).sum()) > 0 and int((count > 0).sum()) > 0
    x = torch.from_numpy(ref.noise_input(64, 3, 16))
    _, lm = ddsp.mfcc(x, 64, 16, 16000, n_mels=128, n_mfcc=13, return_logmel=True)
    empty = (count == 0).nonzero().flatten()
    assert np.allclose(lm[..., empty].numpy(), np.log(np.float64(np.float32(1e-5))), rtol=1e-6)     # an empty band reads log(floor)
    # fmax above Nyquist is clamped to it
    a = enc.mel_filterbank(256, 8000, 40, 20.0, 8000.0)
    b = enc.mel_filterbank(256, 8000, 40, 20.0, 4000.0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert np.array_equal(ref.filterbank(256, 8000, 40, 20.0, 8000.0), ref.filterbank(256, 8000, 40, 20.0, 4000.0))
    assert int(a[1][-1]) + int(a[2][-1]) <= 129                # the last band ends at the Nyquist bin
    with pytest.raises(ValueError):
        enc.mel_filterbank(256, 8000, 40, 5000.0, 8000.0)      # fmin above the clamped top


def test_window_scale_and_dct():
    for n_fft in (64, 2048):
        w = enc.hann_window(n_fft).numpy()
        assert np.array_equal(w.view(np.uint32), ref.hann(n_fft).view(np.uint32)) and w[0] == 0
        t = enc.mfcc_tables(n_fft, 16000, 40, 13)
        assert t["scale"] == float(np.float32(2.0 / w.astype(np.float64).sum()))
    for n_mels, n_mfcc in ref.MEL_PAIRS:
        assert np.array_equal(enc.dct_table(n_mels, n_mfcc).numpy().view(np.uint32), ref.dct(n_mels, n_mfcc).view(np.uint32))
    # a full-scale sine on a bin centre reads 1 in its bin: the floor is a level relative to full scale
    n = np.arange(256)
    spec = ref.spectrum(np.sin(2 * np.pi * 32 * n / 256)[None].astype(np.float32), 256, 256)
    assert abs(spec[0][0, 0, 32] - 1.0) < 1e-6


# ------------------------------------------------------------------------------------------------------- argument checks

def test_ddsp_mfcc_argument_checks_without_a_gpu():
    L = ddsp._lib.lib()
    word = ctypes.c_uint64(0)                                  # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)

    def call(x=p, bs=p, bc=p, bw=p, dct=p, out=p, lm=p, B=1, Ls=4096, n_fft=1024, hop=256, n_mels=128, n_mfcc=30):
        return L.ddsp_mfcc(x, bs, bc, bw, dct, out, lm, B, Ls, n_fft, hop, n_mels, n_mfcc, 1.0, 1e-5, None)

    for name in ("x", "bs", "bc", "bw", "dct", "out"):
        assert call(**{name: None}) == -1, name                # a null pointer (logmel may be null: that launches)
    for n_fft in (0, 32, 96, 1000, 4096):
        assert call(n_fft=n_fft) == -1, n_fft
    assert call(hop=0) == -1 and call(hop=-3) == -1
    assert call(Ls=1023) == -1                                 # shorter than a frame
    assert call(n_mels=0) == -1 and call(n_mels=129) == -1
    assert call(n_mfcc=0) == -1 and call(n_mfcc=65) == -1 and call(n_mels=20, n_mfcc=21) == -1
    assert call(B=-1) == -1
    assert call(B=0) == 0 and call(B=0, x=None, out=None, Ls=10) == 0       # an empty batch: nothing to read or launch
    assert call(B=0, n_fft=96) == -1                           # ... with sizes that are still checked


def test_header_table_and_exports_agree_on_ddsp_mfcc():
    names = list(ddsp._lib.SIGNATURES)
    # behind the loudness kernel it is modelled on (tests/test_notes_host.py pins the table's last four entries, so the place
    # directly in front of ddsp_gather_batch is taken); ddsp_gather_batch stays the last symbol
    at = names.index("ddsp_loudness")
    assert names == list(ddsp._lib.EXPORTS) and names[at + 1] == "ddsp_mfcc" and names[-1] == "ddsp_gather_batch"
    restype, argtypes = ddsp._lib.SIGNATURES["ddsp_mfcc"]
    assert restype is ctypes.c_int and len(argtypes) == 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddsp_hip.h")).read()
    assert header.index("int ddsp_loudness(") < header.index("int ddsp_mfcc(") < header.index("int ddsp_pcm_to_mono(")
    assert ddsp._lib.ABI_VERSION == 5 and ddsp._lib.lib().ddsp_hip_abi_version() == 5


# ------------------------------------------------------------------------------------------------- the opt-in in the modules

def keys_of(conf):
    torch.manual_seed(0)
    return (list(ddsp.Controller(conf).state_dict()), list(ddsp.Decoder(conf).state_dict()), list(ddsp.AutoEncoder(conf).state_dict()))


TODAY_CONTROLLER = (["mlp_f0", "mlp_loudness"], ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0"],
                    ["mlp_gru"], ["dense_harmonic.weight", "dense_harmonic.bias", "dense_loudness.weight", "dense_loudness.bias",
                                  "dense_filter.weight", "dense_filter.bias"])


def stack_keys(name, depth=3):
    return [f"{name}.mlp_layer{i}.{j}.{w}" for i in range(1, depth + 1) for j in (0, 1) for w in ("weight", "bias")]


def test_without_z_dims_the_state_dicts_are_todays():
    plain, zero = keys_of(Conf), keys_of(ConfZ0)
    assert plain == zero
    controller = stack_keys("mlp_f0") + stack_keys("mlp_loudness") + TODAY_CONTROLLER[1] + stack_keys("mlp_gru") + TODAY_CONTROLLER[3]
    assert plain[0] == controller                              # spelled out: what the reference's checkpoints hold
    assert plain[1] == ["controller." + k for k in controller] + ["harmonics.harmonics", "harmonics.last_phases", "reverb.noise",
                                                                  "reverb.decay", "reverb.wet", "reverb.t", "reverb.buffer"]
    assert not any("z_encoder" in k or "mlp_z" in k for k in plain[2])
    for conf in (Conf, ConfZ0):
        dec = ddsp.Decoder(conf)
        assert dec.z_dims == 0 and not hasattr(dec, "z_encoder") and not hasattr(dec.controller, "mlp_z")
        assert dec.controller.gru.input_size == 512 and dec.controller.mlp_gru.mlp_layer1[0].in_features == 64 + 512
    # a checkpoint of a decoder without the latent loads with strict=True, and the same seed gives the same parameters
    torch.manual_seed(5)
    a = ddsp.Decoder(Conf)
    torch.manual_seed(5)
    b = ddsp.Decoder(ConfZ0)
    b.load_state_dict(a.state_dict(), strict=True)
    torch.manual_seed(5)
    c = ddsp.Decoder(ConfZ0)
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), c.state_dict().values()))


def test_with_z_dims_the_state_dicts_gain_mlp_z_and_z_encoder():
    plain, latent = keys_of(Conf), keys_of(ConfZ)
    z_encoder = ["norm.weight", "norm.bias", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "out.weight", "out.bias"]
    assert set(latent[0]) == set(plain[0]) | set(stack_keys("mlp_z"))
    assert set(latent[1]) == set(plain[1]) | {"controller." + k for k in stack_keys("mlp_z")} | {"z_encoder." + k for k in z_encoder}
    assert set(latent[2]) == set(plain[2]) | {"decoder.controller." + k for k in stack_keys("mlp_z")} | {"decoder.z_encoder." + k for k in z_encoder}
    dec = ddsp.Decoder(ConfZ)
    sd = dec.state_dict()
    assert sd["controller.mlp_z.mlp_layer1.0.weight"].shape == (256, 4)
    assert sd["controller.gru.weight_ih_l0"].shape == (3 * 64, 3 * 256)
    assert sd["controller.mlp_gru.mlp_layer1.0.weight"].shape == (256, 64 + 3 * 256)
    assert sd["z_encoder.norm.weight"].shape == (30,) and sd["z_encoder.gru.weight_ih_l0"].shape == (3 * 64, 30)
    assert sd["z_encoder.out.weight"].shape == (4, 64)
    assert not any("mfcc" in k for k in sd)                    # the tables are buffers outside the state dict
    assert dec.z_encoder.mfcc.dct.shape == (30, 128) and dec.z_encoder.mfcc.fbank.shape == (128, 129)
    assert ddsp.ZEncoder(type("C", (ConfZ,), dict(z_mels=40, z_mfcc=13))).mfcc.dct.shape == (13, 40)
    assert ddsp.ZEncoder(type("C", (Conf,), dict(z_dims=2))).gru.hidden_size == 512           # the default width
    with pytest.raises(ValueError):
        ddsp.ZEncoder(Conf)
    # the encoder's CPU path: [B, T hop] -> [B, T, z_dims], frames lined up with the decoder's
    z = dec.z_encoder(torch.randn(2, 8 * 64))
    assert z.shape == (2, 8, 4) and z.requires_grad
    zp = dec.z_encoder(torch.randn(2, 8 * 64 + 192), padded=True)
    assert zp.shape == (2, 8, 4)
    z1, state = dec.z_encoder.live(torch.randn(1, 256 + 3 * 64))
    assert z1.shape == (1, 4, 4) and state.shape == (1, 1, 64)


def test_decoder_forward_needs_z_or_audio():
    dec = ddsp.Decoder(ConfZ)
    batch = {"normalized_cents": torch.rand(2, 8, 1), "loudness": torch.rand(2, 8, 1), "f0": torch.full((2, 8, 1), 220.0)}
    with pytest.raises(ValueError, match="'z'.*'audio'|timbre latent"):
        dec(batch)
    with pytest.raises(ValueError, match="'z' must be"):
        dec.controller(dict(batch, z=torch.zeros(2, 7, 4)))
    with pytest.raises(ValueError, match="no 'z'"):
        dec.controller(batch)
    ae = ddsp.AutoEncoder(ConfZ)
    with pytest.raises(ValueError, match="timbre"):
        ae._with_timbre(dict(batch), None, None, "play")       # play without timbre= on a decoder with a latent
    assert ae._timbre(torch.zeros(2, 4), 8, "forward").shape == (2, 8, 4)
    assert ae.encode_timbre(torch.randn(2, 1024)).shape == (2, 4)
    with pytest.raises(ValueError, match="no timbre latent"):
        ddsp.AutoEncoder(Conf).encode_timbre(torch.randn(2, 1024))
