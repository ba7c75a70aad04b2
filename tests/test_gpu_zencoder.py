"""The timbre latent on the device: ZEncoder against its own CPU path, a decoder conditioned on z through
training (eager fp32 and bf16, the captured step, Trainer.fit and resume), AutoEncoder's `timbre=`, the live pair of states, and
the refusal of the graphed live objects.

Tolerance of z: Z_ERR_CPU is the largest |z(fp32) - z(fp64)| of the module's CPU path over the sixteen seeded modules and inputs
of `cpu_z_error` (LayerNorm, GRU and Linear in fp64 on the fp64 MFCCs of tests/mfcc_reference.py); the device gets Z_MARGIN times
that against the CPU path.  Re-measure with `python tests/test_gpu_zencoder.py` (no GPU needed)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import ddsp_pytorch_amd as ddsp  # noqa: E402
import mfcc_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

Z_ERR_CPU = 1.82e-7          # measured 1.8180e-07: see the module docstring
Z_MARGIN = 3.0


class Conf:
    n_fft, hop_length, sample_rate = 256, 64, 16000
    n_harmonics, n_noise_filters = 16, 17
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 3, 64, 1
    batch_size = 2


class ConfZ(Conf):
    z_dims, z_gru_units = 4, 64


B, T, HOP = 2, 8, 64


def clip(seed, frames=T, rows=B):
    """a tone with some noise in row 0, noise in the others: [rows, frames hop]"""
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(frames * HOP)
    x = 0.3 * torch.randn(rows, frames * HOP, generator=g)
    x[0] = 0.5 * torch.sin(2 * np.pi * 440.0 * n / Conf.sample_rate) + 0.05 * torch.randn(frames * HOP, generator=g)
    return x


def z_encoder(seed):
    torch.manual_seed(seed)
    return ddsp.ZEncoder(ConfZ)


def z_fp64(ze, x):
    """the module in fp64 on the fp64 MFCCs of the padded clip"""
    p = ze.padding
    xp = torch.nn.functional.pad(x, (p // 2, p - p // 2)).numpy()
    want = ref.reference(xp, Conf.n_fft, HOP, Conf.sample_rate, ze.mfcc.n_mels, ze.mfcc.n_mfcc)
    zd = copy.deepcopy(ze).double()
    h, _ = zd.gru(zd.norm(torch.from_numpy(want["mfcc"])))
    return zd.out(h).detach(), want, xp


def cpu_z_error():
    worst = 0.0
    for seed in range(16):
        ze, x = z_encoder(100 + seed), clip(200 + seed)
        with torch.no_grad():
            worst = max(worst, float((ze(x).double() - z_fp64(ze, x)[0]).abs().max()))
    return worst


def make_decoder(conf=ConfZ):
    torch.manual_seed(11)
    return ddsp.Decoder(conf, noise_rng="device", seed=3).cuda()


def make_adam(model, lr=1e-3):
    return torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=torch.tensor(lr, device="cuda"), fused=True,
                            capturable=True)


def batch(i, rows=B, frames=T):
    g = torch.Generator().manual_seed(300 + i)
    return {"normalized_cents": torch.rand(rows, frames, 1, generator=g).cuda(), "loudness": (torch.rand(rows, frames, 1, generator=g) * 2 - 1).cuda(),
            "f0": (100 + 200 * torch.rand(rows, frames, 1, generator=g)).cuda(), "audio": clip(400 + i, frames, rows).cuda()}


def examples(E, frames=T):
    g = torch.Generator().manual_seed(5)
    return {"f0": 100 + 200 * torch.rand(E, frames, 1, generator=g), "harmonicity": torch.rand(E, frames, 1, generator=g),
            "loudness": torch.rand(E, frames, 1, generator=g) * 2 - 1, "probabilities": torch.rand(E, frames, 8, generator=g),
            "normalized_cents": torch.rand(E, frames, 1, generator=g), "audio": clip(6, frames, E)}


def latent_parameters(model):
    named = [(k, p) for k, p in model.named_parameters() if k.startswith("z_encoder.") or k.startswith("controller.mlp_z.")]
    assert len(named) == 8 + 12
    return named


# ------------------------------------------------------------------------------------------------------------ the encoder

def test_zencoder_device_against_its_cpu_path():
    ze = z_encoder(100)
    dev = copy.deepcopy(ze).cuda()
    x = clip(200)
    with torch.no_grad():
        z_cpu = ze(x)
        z_dev = dev(x.cuda())
        want64, want, xp = z_fp64(ze, x)
        got, lm = dev.mfcc(torch.from_numpy(xp).cuda(), return_logmel=True)
    assert z_dev.shape == (B, T, 4) and got.shape == (B, T, 30)
    r, where = ref.worst_ratio(got.cpu().numpy(), lm.cpu().numpy(), want)
    err = float((z_dev.cpu() - z_cpu).abs().max())
    print(f"MFCC: worst |error| / bound(c = 1) = {r:.3f} at {where}; z: |device - cpu| = {err:.3e}, |device - fp64| = "
          f"{float((z_dev.cpu().double() - want64).abs().max()):.3e}, |cpu - fp64| = {float((z_cpu.double() - want64).abs().max()):.3e} "
          f"(allowed {Z_MARGIN * Z_ERR_CPU:.3e})")
    assert r <= ref.KERNEL_FACTOR * ref.C_CPU, (r, where)
    assert err <= Z_MARGIN * Z_ERR_CPU
    # the padded form and the live form see the same frames
    with torch.no_grad():
        assert torch.equal(dev(torch.from_numpy(xp).cuda(), padded=True), z_dev)
        z_live, state = dev.live(torch.from_numpy(xp).cuda())
    assert torch.equal(z_live, z_dev) and state.shape == (1, B, 64)


def test_decoder_with_audio_equals_decoder_with_its_z():
    dec = make_decoder().eval()
    x = batch(0)
    with torch.no_grad():
        dec.noise.reseed(3, 0)
        from_audio = dec(x)
        z = dec.z_encoder(x["audio"])
        dec.noise.reseed(3, 0)
        from_z = dec({k: v for k, v in x.items() if k != "audio"} | {"z": z})
        dec.noise.reseed(3, 0)
        other = dec({k: v for k, v in x.items() if k != "audio"} | {"z": z + 0.5})
    assert from_audio.shape == (B, T * HOP) and bool(torch.isfinite(from_audio).all())
    assert torch.equal(from_audio, from_z)
    assert not torch.equal(from_audio, other)                  # the latent reaches the sound
    with pytest.raises(ValueError):
        dec({k: v for k, v in x.items() if k != "audio"})


def test_a_decoder_without_z_dims_is_untouched():
    class ConfZ0(Conf):
        z_dims = 0
    a, b = make_decoder(Conf).eval(), make_decoder(ConfZ0).eval()
    assert list(a.state_dict()) == list(b.state_dict()) and not hasattr(a, "z_encoder")
    x = batch(1)
    with torch.no_grad():
        ya, yb = a(x), b(x)                                    # (the audio key is not read)
    assert torch.equal(ya, yb)


# ----------------------------------------------------------------------------------------------------------------- training

@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_one_train_step_moves_the_latent_path(amp):
    model = make_decoder()
    loss_fn, opt = ddsp.MSSLoss((256, 128, 64)).cuda(), make_adam(model)
    before = {k: p.detach().clone() for k, p in latent_parameters(model)}
    loss, _ = ddsp.train_step(model, loss_fn, opt, batch(0), amp_dtype=amp)
    assert bool(torch.isfinite(loss)), float(loss)
    for k, p in latent_parameters(model):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
        assert not torch.equal(p.detach(), before[k]), k


def test_captured_step_equals_the_eager_step():
    m_e, m_g = make_decoder(), make_decoder()
    l_e, l_g = ddsp.MSSLoss((256, 128, 64)).cuda(), ddsp.MSSLoss((256, 128, 64)).cuda()
    o_e, o_g = make_adam(m_e), make_adam(m_g)
    graphed = ddsp.GraphedTrainStep(m_g, l_g, o_g, batch(0))
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k                            # construction left the model where it was
    tol = 1e-4                                                 # tests/test_gpu_trainer.py: graphed against eager in fp32
    for i in range(2):
        loss_e, _ = ddsp.train_step(m_e, l_e, o_e, batch(i))
        loss_g, _ = graphed.step(batch(i))
        print("step", i, loss_e.item(), loss_g.item())
        assert abs(loss_e.item() - loss_g.item()) <= tol * abs(loss_e.item()), (i, loss_e.item(), loss_g.item())


def test_fit_writes_a_checkpoint_that_resume_loads_strictly(tmp_path):
    data = examples(4)
    first = ddsp.Trainer(ConfZ, data, precision=32, n_ffts=(256, 128, 64), log_dir=str(tmp_path), decoder=make_decoder(), seed=3)
    history = first.fit(1)
    assert first.global_step == 2 and len(history) == 1 and np.isfinite(history[0]["train_loss"]) and first._step is not None
    path = ddsp.latest_checkpoint(first.version, first.log_dir)
    assert os.path.basename(path) == "epoch=0-step=2.ckpt"
    assert sorted(os.listdir(os.path.join(first.run_dir(), "audio"))) == ["0-0.wav", "0-1.wav"]       # validation read the audio too
    second = ddsp.Trainer(ConfZ, data, precision=32, n_ffts=(256, 128, 64), log_dir=first.log_dir, seed=99, version=first.version)
    second.load(path)                                          # strict=True inside
    assert second.epoch == 1 and second.global_step == 2
    keys = list(second.model.state_dict())
    assert any(k.startswith("z_encoder.") for k in keys) and any(k.startswith("controller.mlp_z.") for k in keys)
    for (k, a), (_, b) in zip(first.model.state_dict().items(), second.model.state_dict().items()):
        assert torch.equal(a, b), k
    assert len(second.optimizer.param_groups[0]["params"]) == len([p for p in second.model.parameters() if p.requires_grad])


# -------------------------------------------------------------------------------------------------------------- autoencoder

LONG = 32                    # frames: the pitch tracker needs more than 1024 samples, and at 32 its frames line up with the loudness's


def autoencoder():
    torch.manual_seed(12)
    return ddsp.AutoEncoder(ConfZ, noise_rng="device", seed=3, tracker="yin").cuda().eval()


def test_autoencoder_timbre_keyword():
    ae = autoencoder()
    x, y = clip(500, LONG).cuda(), clip(501, 20).cuda()

    def run(**kw):
        ae.decoder.noise.reseed(3, 0)
        with torch.no_grad():
            return ae(x, **kw)

    own = run()
    with torch.no_grad():
        z = ae.decoder.z_encoder(x)
        held = ae.encode_timbre(y)
    assert z.shape == (B, LONG, 4) and held.shape == (B, 4)
    assert own.shape == (B, LONG * HOP) and torch.equal(run(timbre=z), own)
    from_latent = run(timbre=held)
    assert torch.equal(from_latent, run(timbre=held.unsqueeze(1).expand(-1, LONG, -1).contiguous()))
    assert torch.equal(from_latent, run(timbre=y)) and not torch.equal(from_latent, own)
    with pytest.raises(ValueError):
        run(timbre=z[:, :5])
    torch.manual_seed(12)
    plain = ddsp.AutoEncoder(Conf, noise_rng="device", seed=3, tracker="yin").cuda().eval()
    with pytest.raises(ValueError, match="no timbre latent"):
        plain(x, timbre=held)


def test_transfer_and_play_take_the_timbre():
    ae = autoencoder()
    x, y = clip(500, LONG).cuda(), clip(501, 20).cuda()
    p = ae.padding
    with torch.no_grad():
        held = ae.encode_timbre(y)
        target = ddsp.conditioning_statistics(ae.encoder(torch.nn.functional.pad(x, (p // 2, p - p // 2))))
        notes = ae.transcribe(x)

        def run(call, *args, **kw):
            ae.decoder.noise.reseed(3, 0)
            return call(*args, **kw)

        own = run(ae.transfer, x, target)
        from_latent = run(ae.transfer, x, target, timbre=held)
        assert torch.equal(from_latent, run(ae.transfer, x, target, timbre=y)) and not torch.equal(from_latent, own)
        played = run(ae.play, notes, frames=LONG, timbre=held)
        assert torch.equal(played, run(ae.play, notes, frames=LONG, timbre=y))
        with pytest.raises(ValueError, match="needs timbre="):
            ae.play(notes, frames=LONG)
    for audio in (own, from_latent, played):
        assert audio.shape == (B, LONG * HOP) and bool(torch.isfinite(audio).all())


def test_forward_live_carries_both_states():
    ae = autoencoder()
    g = np.random.default_rng(7)
    blocks = [(0.3 * g.standard_normal(LONG * HOP + ConfZ.n_fft)).astype(np.float32) for _ in range(2)]
    hidden = (torch.zeros(1, 1, 64, device="cuda"), None)
    with torch.no_grad():
        audio0, hidden = ae.forward_live(blocks[0], hidden)
        z0 = hidden[1].clone()
        audio1, hidden = ae.forward_live(blocks[1], hidden)
    assert audio0.shape == audio1.shape == (LONG * HOP,) and np.isfinite(audio0).all() and np.isfinite(audio1).all()
    assert isinstance(hidden, tuple) and hidden[0].shape == (1, 1, 64) and hidden[1].shape == (1, 1, 64)
    assert not torch.equal(hidden[1], z0)
    with pytest.raises(ValueError, match="decoder_hidden, z_hidden"):
        ae.forward_live(blocks[0], torch.zeros(1, 1, 64, device="cuda"))


def test_graphed_live_objects_refuse_a_latent():
    with pytest.raises(ValueError, match="not wired into the graphed live objects"):
        ddsp.GraphedLiveDecoder(make_decoder(), frames=T)
    with pytest.raises(ValueError, match="not wired into the graphed live objects"):
        ddsp.GraphedSynth(ConfZ, 1, T, ConfZ.n_noise_filters, live=True)
    ddsp.GraphedSynth(ConfZ, 1, T, ConfZ.n_noise_filters)     # the whole-clip synth reads controls only: no latent in it


if __name__ == "__main__":
    print(f"CPU path of ZEncoder, fp32 against fp64: max |error| = {cpu_z_error():.4e}; Z_ERR_CPU in this file: {Z_ERR_CPU}")
