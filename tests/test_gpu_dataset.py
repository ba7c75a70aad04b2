"""The training set built on the device (csrc/ddsp_dataset.hip around the encoder) against torch and against the reference's own
dataset/audio_dataset.py on the CPU (fixtures G26, tools/make_dataset_goldens.py).  Tolerances are the encoder's: audio bit-exact
for files at the conf rate and 1e-6 where resampled, loudness 2e-6, CREPE probabilities 4x the fixture's fp32-vs-fp64 spread,
f0 and cents bit-exact wherever the top-1 margin is decisive."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import dataset
from crepe_seeded import top1_margin
from dataset_common import FIXTURES, KEYS, fixture, example_sources

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.float32])
def test_pcm_to_mono_matches_torch(dtype, C):
    g = torch.Generator().manual_seed(C * 10 + int(dtype == torch.int32) + 2 * int(dtype == torch.float32))
    L = 100003
    if dtype == torch.float32:
        pcm = 0.5 * torch.randn(L, C, generator=g)
    else:
        info = torch.iinfo(dtype)
        pcm = torch.randint(info.min, info.max, (L, C), generator=g, dtype=torch.int64).to(dtype)
        pcm[:4] = torch.tensor([info.min, info.max, 0, -1], dtype=dtype)[:, None]
    y = dataset.pcm_to_mono(pcm.cuda()).cpu()
    ref = dataset.pcm_to_float(pcm.numpy())                  # [C, L], torchaudio.load(normalize=True)'s values
    ref = ref[0] if C == 1 else ref.mean(dim=0)              # audio_dataset.py:31-37
    assert y.shape == (L,) and y.dtype == torch.float32
    if C <= 2:
        assert torch.equal(y, ref)
    else:
        # torch's CPU mean is a sum, then a division, but the order of that sum over channels depends on the host's vector
        # code (bit-exact up to C = 4 on the MI355X box's host, not from C = 5).  Bound: two recursive sums of C terms and their
        # divisions, each within ((C - 1) + 1) u sum |x| / C of the exact mean (u = 2^-24): 2^-23 sum over c of |x_c|
        x = dataset.pcm_to_float(pcm.numpy()).double()
        bound = 2.0 ** -23 * x.abs().sum(0) + 2.0 ** -149
        assert bool(((y.double() - ref.double()).abs() <= bound).all())


def _reference_examples(parts, hop, duration, step, p):
    """audio_dataset.py:46-59 and :86, 90 with stock ops, file by file."""
    audio = []
    for y in parts:
        pad = len(y) % hop
        audio.append(F.pad(y, (pad // 2, pad - pad // 2)).unfold(0, duration, step))
    audio = torch.cat(audio)
    return F.pad(audio, (p // 2, p - p // 2)), audio


def test_make_examples_matches_pad_unfold_pad():
    rng = np.random.default_rng(31)
    for case in range(24):
        hop = int(rng.choice([64, 100, 128, 256, 441, 512]))
        duration = hop * int(rng.integers(1, 12))
        step = int(rng.integers(1, 2 * duration + 1)) if case % 3 else int(rng.integers(duration + 1, 3 * duration))  # step > duration
        p = int(rng.choice([0, hop, 3 * hop, 2048 - hop, 7]))
        n_files = int(rng.integers(1, 6))
        lens = [int(duration + rng.integers(0, 4 * duration + 3 * hop)) for _ in range(n_files)]
        parts = [torch.randn(n, generator=torch.Generator().manual_seed(100 * case + i)) for i, n in enumerate(lens)]
        ref_in, ref_audio = _reference_examples(parts, hop, duration, step, p)
        counts = [(n + n % hop - duration) // step + 1 for n in lens]
        starts, firsts = np.cumsum([0] + lens)[:-1], np.cumsum([0] + counts)[:-1]
        files = torch.tensor([[s, n, (n % hop) // 2, f] for s, n, f in zip(starts, lens, firsts)], dtype=torch.int64).cuda()
        y = torch.cat(parts).cuda()
        E = sum(counts)
        assert E == ref_audio.shape[0]
        # one launch for everything, then chunks that start and end inside files, each output alone
        enc_in = torch.full((E, duration + p), float("nan"), device="cuda")
        audio = torch.full((E, duration), float("nan"), device="cuda")
        dataset.make_examples(y, files, 0, E, duration, step, p, enc_in=enc_in, audio=audio)
        assert torch.equal(enc_in.cpu(), ref_in) and torch.equal(audio.cpu(), ref_audio), case
        e0 = int(rng.integers(0, E))
        n = int(rng.integers(1, E - e0 + 1))
        part_in = torch.full((n, duration + p), float("nan"), device="cuda")
        part_audio = torch.full((n, duration), float("nan"), device="cuda")
        dataset.make_examples(y, files, e0, n, duration, step, p, enc_in=part_in)
        dataset.make_examples(y, files, e0, n, duration, step, p, audio=part_audio)
        assert torch.equal(part_in.cpu(), ref_in[e0:e0 + n]) and torch.equal(part_audio.cpu(), ref_audio[e0:e0 + n]), case


def _check_features(out, g, conf, what):
    tol = 4 * float(g["spread64"])
    src = example_sources(g, conf)
    same = src == conf.sample_rate
    a, ra = out["audio"].numpy(), g["out_audio"]
    assert a.shape == ra.shape and len(src) == a.shape[0]
    assert np.array_equal(a[same], ra[same]), what
    assert np.abs(a[~same] - ra[~same]).max(initial=0) <= 1e-6, what
    assert np.abs(out["loudness"].numpy() - g["out_loudness"]).max() <= 2e-6, what
    p, rp = out["probabilities"].numpy(), g["out_probabilities"]
    assert p.shape == rp.shape and np.abs(p - rp).max() <= tol, (what, np.abs(p - rp).max(), tol)
    sure = top1_margin(rp) > 10 * tol
    assert sure.mean() >= 0.9, (what, sure.mean())
    for k in ("f0", "normalized_cents"):
        assert out[k].shape == g[f"out_{k}"].shape
        assert np.array_equal(out[k].numpy()[sure], g[f"out_{k}"][sure]), (what, k)
    assert np.abs(out["harmonicity"].numpy() - g["out_harmonicity"]).max() <= tol, what


@pytest.mark.parametrize("name", FIXTURES)
def test_device_dataset_matches_reference(name, tmp_path):
    g, conf = fixture(name, tmp_path)
    plh = ddsp.PLHDataset(conf)                                   # the device is CUDA by default
    assert list(plh.final) == list(KEYS)
    for k in KEYS:
        assert not plh.final[k].is_cuda and plh.final[k].dtype == torch.float32
    _check_features(plh.final, g, conf, name)
    # both caches hold what was built, as plain CPU tensors
    cached = torch.load(conf.data_dir + "/plh_dataset.pth", weights_only=True)
    assert all(torch.equal(cached[k], plh.final[k]) for k in KEYS)
    assert torch.equal(torch.load(conf.data_dir + "/audio_dataset.pth", weights_only=True), plh.final["audio"])


def test_two_device_builds_agree(tmp_path):
    """The HIP stages are deterministic; MIOpen may pick another convolution algorithm per call, so the features are compared
    on decisive frames and within the fixture tolerance.  The second build also takes another encoder batch and starts from
    AudioData's cache (the cached examples uploaded as one-example files)."""
    g, conf = fixture("g26_dataset_mix", tmp_path)
    a = ddsp.PLHDataset(conf).final
    b = ddsp.PLHDataset(conf, clear=True, encode_batch=3).final
    (tmp_path / "g26_dataset_mix" / "plh_dataset.pth").unlink()
    c = ddsp.PLHDataset(conf, encode_batch=5).final
    tol = 4 * float(g["spread64"])
    sure = top1_margin(a["probabilities"].numpy()) > 10 * tol
    for u in (b, c):
        assert torch.equal(u["audio"], a["audio"])
        assert (u["probabilities"] - a["probabilities"]).abs().max().item() <= tol
        assert (u["loudness"] - a["loudness"]).abs().max().item() <= 2e-6
        for k in ("f0", "normalized_cents"):
            assert np.array_equal(u[k].numpy()[sure], a[k].numpy()[sure]), k


@pytest.mark.parametrize("orig", [16000, 48000])
def test_resampler_to_44k1_matches_cpu_restatement(orig):
    torch.manual_seed(orig)
    rs = ddsp.encoder.Resample(orig, 44100)
    assert rs.ntaps * rs.new <= 16384
    x = 0.3 * torch.randn(2, 3 * orig + 17)
    t = torch.arange(x.shape[1]) / orig
    x[1] = 0.4 * torch.sin(2 * np.pi * 440 * t) + 0.1 * torch.sin(2 * np.pi * 5000 * t)
    ref = rs(x)
    rsd = rs.cuda()
    y = rsd(x.cuda()).cpu()
    assert y.shape == ref.shape == (2, ddsp.encoder.resampled_length(x.shape[1], orig, 44100))
    assert (y - ref).abs().max().item() <= 1e-6
    # one long row, as the dataset resamples a whole file
    assert torch.equal(rsd(x[1:].cuda()).cpu()[0], y[1])


def test_dataloader_batch_trains_decoder(tmp_path):
    g, conf = fixture("g26_dataset_mix", tmp_path)
    plh = ddsp.PLHDataset(conf)

    class DecConf:
        n_harmonics, n_noise_filters, sample_rate, hop_length = 16, 9, conf.sample_rate, conf.hop_length
        decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1

    batch = next(iter(DataLoader(plh, batch_size=conf.batch_size, shuffle=False)))
    assert list(batch) == list(KEYS) and batch["audio"].shape == (conf.batch_size, 5376)
    batch = {k: v.cuda() for k, v in batch.items()}
    torch.manual_seed(0)
    dec = ddsp.Decoder(DecConf).cuda()
    before = [p.detach().clone() for p in dec.parameters()]
    opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    with torch.no_grad():
        assert dec(batch).shape == batch["audio"].shape
    loss, _ = ddsp.train_step(dec, ddsp.MSSLoss().cuda(), opt, batch)
    assert torch.isfinite(loss)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(dec.parameters(), before))
