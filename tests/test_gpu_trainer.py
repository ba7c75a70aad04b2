"""The trainer on the device (ddsp_pytorch_amd.trainer): the batch gather kernel, fp16 + loss scaling inside the captured
step, a learning rate that changes between replays, fit() against the hand-written loop, resume, validation audio."""
import os

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import trainer as tr

pytestmark = pytest.mark.gpu


class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 16, 9, 4000, 16
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 2, 64, 1
    batch_size = 32


def make_decoder(conf=Conf):
    torch.manual_seed(11)
    return ddsp.Decoder(conf, noise_rng="device", seed=3).cuda()


def make_adam(model, lr=1e-3):
    """The optimiser the Trainer builds: fused (takes the loss scale on the device), capturable, the rate in a device tensor."""
    return torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=torch.tensor(lr, device="cuda"), fused=True,
                            capturable=True)


def batch(i, B=3, T=40):
    g = torch.Generator().manual_seed(100 + i)
    return {"normalized_cents": torch.rand(B, T, 1, generator=g).cuda(), "loudness": (torch.rand(B, T, 1, generator=g) * 2 - 1).cuda(),
            "f0": (100 + 200 * torch.rand(B, T, 1, generator=g)).cuda(), "audio": (0.1 * torch.randn(B, T * 16, generator=g)).cuda()}


def examples(E, T=40, hop=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {"f0": 100 + 200 * torch.rand(E, T, 1, generator=g), "harmonicity": torch.rand(E, T, 1, generator=g),
            "loudness": torch.rand(E, T, 1, generator=g) * 2 - 1, "probabilities": torch.rand(E, T, 8, generator=g),
            "normalized_cents": torch.rand(E, T, 1, generator=g), "audio": 0.1 * torch.randn(E, T * hop, generator=g)}


def close(a, b, tol):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) <= tol * max(1e-3, float(a.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ gather

def resident(E, lens, shift=0, seed=0):
    """Arrays [E, n] per row length; `shift` floats of offset from the allocation's (aligned) base."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n in lens:
        buf = torch.empty(E * n + shift, device="cuda")
        buf.copy_(torch.randn(E * n + shift, generator=g))
        out[f"n{n}"] = buf[shift:shift + E * n].view(E, n)
    return out


def run_gather(arrays, perm, cursor, rows, out_rows=None, shift=0):
    E = next(iter(arrays.values())).shape[0]
    out_rows = rows if out_rows is None else out_rows
    out = {}
    for k, v in arrays.items():
        buf = torch.full((out_rows * v.shape[1] + shift,), -7.0, device="cuda")
        out[k] = buf[shift:].view(out_rows, v.shape[1])
    perm_t = torch.tensor(perm, dtype=torch.int64, device="cuda")
    cur = torch.tensor([cursor], dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ddsp.gather_batch(arrays, out, perm_t, cur, rows, err)
    torch.cuda.synchronize()
    assert E == next(iter(arrays.values())).shape[0]
    return out, int(cur.item()), int(err.item())


LENS = (172, 173, 88064, 64003)


@pytest.mark.parametrize("shift", [0, 1])
def test_gather_equals_index_select(shift):
    """Every row length (16-byte and 4-byte path; shift = 1 takes even the aligned lengths off the 16-byte path), repeated
    indices, the first and last example, batch 1, a short batch, a cursor in the middle of the permutation."""
    E = 12
    arrays = resident(E, LENS, shift=shift)
    before = {k: v.clone() for k, v in arrays.items()}
    perm = [3, 3, 0, E - 1, 7, E - 1, 0, 5, 3, 1, 2, 4, 6, 8, 9, 10, 11]            # longer than E: indices repeat
    for cursor, rows in ((0, 8), (0, 1), (5, 6), (len(perm) - 3, 3), (2, 1), (0, len(perm))):
        out, cur, err = run_gather(arrays, perm, cursor, rows, shift=shift)
        assert err == 0 and cur == cursor + rows
        idx = torch.tensor(perm[cursor:cursor + rows], device="cuda")
        for k, v in arrays.items():
            assert torch.equal(out[k], v.index_select(0, idx)), (k, cursor, rows)
    # a short batch into the first rows of a full-size output: the rows behind it are not written
    out, cur, err = run_gather(arrays, perm, 4, 3, out_rows=8)
    idx = torch.tensor(perm[4:7], device="cuda")
    for k, v in arrays.items():
        assert torch.equal(out[k][:3], v.index_select(0, idx)) and bool((out[k][3:] == -7.0).all()), k
    for k, v in arrays.items():
        assert torch.equal(v, before[k]), k                                        # the resident arrays are only read


def test_gather_through_device_batches_all_keys_one_launch():
    data = examples(70)
    b = ddsp.DeviceBatches(data, 32, seed=3, device="cuda")
    host = ddsp.DeviceBatches(data, 32, seed=3, device="cpu")
    for epoch in range(2):
        got = [{k: v.clone() for k, v in x.items()} for x in b.epoch(epoch)]
        want = list(host.epoch(epoch))
        assert [x["audio"].shape[0] for x in got] == [32, 32, 6]
        for x, y in zip(got, want):
            for k in tr.KEYS:
                assert torch.equal(x[k].cpu(), y[k]), (epoch, k)
        assert int(b.cursor.item()) == 70
    b.check()


def test_captured_gather_walks_consecutive_batches():
    E, B = 12, 4
    arrays = resident(E, LENS, seed=1)
    out = {k: torch.zeros(B, v.shape[1], device="cuda") for k, v in arrays.items()}
    perm = torch.tensor([5, 0, 11, 3, 3, 7, 1, 2, 9, 10, 4, 6, 8, 0], dtype=torch.int64, device="cuda")
    cursor = torch.tensor([1], dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ddsp.gather_batch(arrays, out, perm, cursor, B, err, advance=False)             # (first launch outside a capture)
    torch.cuda.synchronize()
    assert int(cursor.item()) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ddsp.gather_batch(arrays, out, perm, cursor, B, err)
    assert int(cursor.item()) == 1                                                  # capturing ran nothing
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        idx = perm[1 + i * B:1 + (i + 1) * B]
        for k, v in arrays.items():
            assert torch.equal(out[k], v.index_select(0, idx)), (i, k)
        assert int(cursor.item()) == 1 + (i + 1) * B
    assert int(err.item()) == 0


def test_gather_never_reads_a_bad_index():
    """An example index outside [0, E) or a position outside the permutation: the row is zero-filled, the error word says
    which, every other row is right and nothing else changes.  (The kernel checks before it forms an address.)"""
    E = 6
    arrays = resident(E, (172, 173, 8192 + 4), seed=2)
    before = {k: v.clone() for k, v in arrays.items()}
    perm = [2, E, 1, -1, 5, 1 << 40]
    out, cur, err = run_gather(arrays, perm, 0, 6)
    assert err == tr.BAD_INDEX and cur == 6
    for k, v in arrays.items():
        for r, e in enumerate(perm):
            if 0 <= e < E:
                assert torch.equal(out[k][r], v[e]), (k, r)
            else:
                assert bool((out[k][r] == 0).all()), (k, r)
    out, cur, err = run_gather(arrays, [0, 1, 2, 3], 3, 3, out_rows=4)                # positions 3, 4, 5 of a permutation of 4
    assert err == tr.BAD_CURSOR
    for k, v in arrays.items():
        assert torch.equal(out[k][0], v[3]) and bool((out[k][1:3] == 0).all()) and bool((out[k][3] == -7.0).all()), k
    out, cur, err = run_gather(arrays, [0, 1, 2, 3], -2, 2)
    assert err == tr.BAD_CURSOR and all(bool((o == 0).all()) for o in out.values())
    for k, v in arrays.items():
        assert torch.equal(v, before[k]), k
    # DeviceBatches turns the word into an exception when the epoch's values are read
    b = ddsp.DeviceBatches(examples(8), 4, device="cuda")
    b.start_epoch(0)
    b.perm[1] = 99
    b.fetch()
    with pytest.raises(ddsp._lib.DdspHipError):
        b.check()
    b.check()                                                                       # (the word was cleared)


# ------------------------------------------------------------------------------------------------------- the captured step

def test_fp16_graph_equals_fp16_eager():
    def make():
        model = make_decoder()
        return model, ddsp.MSSLoss((256, 128, 64)).cuda(), make_adam(model), torch.amp.GradScaler("cuda")

    m_e, l_e, o_e, s_e = make()
    m_g, l_g, o_g, s_g = make()
    graphed = ddsp.GraphedTrainStep(m_g, l_g, o_g, batch(0), amp_dtype=torch.float16, scaler=s_g)
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k                                    # construction left the model where it was
    assert s_g.get_scale() == s_e.get_scale() == 65536.0               # ... and the scaler
    tol = 2e-2
    for i in range(4):
        loss_e, _ = ddsp.train_step(m_e, l_e, o_e, batch(i), amp_dtype=torch.float16, scaler=s_e)
        loss_g, _ = graphed.step(batch(i))
        print("fp16 step", i, loss_e.item(), loss_g.item(), s_e.get_scale(), s_g.get_scale())
        assert abs(loss_e.item() - loss_g.item()) <= tol * abs(loss_e.item()), (i, loss_e.item(), loss_g.item())
        assert s_e.get_scale() == s_g.get_scale()
    for (k, a), (_, b) in zip(m_e.named_parameters(), m_g.named_parameters()):
        assert close(a, b, tol), k
    # The default scale (65536) overflows fp16 on this loss at first, so those steps may all have been skipped on both sides.
    # Go on until updates are really taken (tests/test_decoder_training.py bounds the search for a finite scale by 23 halvings):
    # the decisions, the scales and then the updated weights must keep agreeing.
    start = {k: v.detach().clone() for k, v in m_g.named_parameters()}
    for i in range(4, 40):
        loss_e, _ = ddsp.train_step(m_e, l_e, o_e, batch(i), amp_dtype=torch.float16, scaler=s_e)
        loss_g, _ = graphed.step(batch(i))
        assert abs(loss_e.item() - loss_g.item()) <= tol * abs(loss_e.item()), (i, loss_e.item(), loss_g.item())
        assert s_e.get_scale() == s_g.get_scale(), i
    taken_e, taken_g = (int(next(iter(o.state.values()))["step"].item()) for o in (o_e, o_g))
    print("fp16: updates taken in 40 steps", taken_e, taken_g, "scale", s_g.get_scale())
    assert taken_e == taken_g >= 4
    for (k, a), (_, b) in zip(m_e.named_parameters(), m_g.named_parameters()):
        assert close(a, b, tol), k
        assert not b.requires_grad or not torch.equal(b, start[k]), k
    assert int(graphed.counters[0].item()) == m_e.noise._offset == m_g.noise._offset


def test_graphed_step_needs_an_optimiser_that_scales_on_the_device():
    model = make_decoder()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    with pytest.raises(ValueError):
        ddsp.GraphedTrainStep(model, ddsp.MSSLoss((256, 128, 64)).cuda(), opt, batch(0), amp_dtype=torch.float16,
                              scaler=torch.amp.GradScaler("cuda"))
    g = ddsp.GraphedTrainStep(model, ddsp.MSSLoss((256, 128, 64)).cuda(), opt, batch(0))
    with pytest.raises(ValueError):
        g.set_lr(5e-4)                                                 # a Python-float rate is a constant of the captured update


def test_graphed_fp16_step_skips_on_overflow_and_backs_off():
    class Big:
        n_harmonics, n_noise_filters, sample_rate, hop_length = 100, 65, 16000, 128
        decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 2, 128, 1

    rng = np.random.default_rng(4)
    B, T = 4, 40
    x = {"normalized_cents": torch.from_numpy(rng.uniform(0, 1, (B, T, 1)).astype(np.float32)).cuda(),
         "loudness": torch.from_numpy(rng.uniform(-1, 1, (B, T, 1)).astype(np.float32)).cuda(),
         "f0": torch.from_numpy(rng.uniform(80, 400, (B, T, 1)).astype(np.float32)).cuda(),
         "audio": torch.from_numpy((0.1 * rng.standard_normal((B, T * 128))).astype(np.float32)).cuda()}

    def make():
        torch.manual_seed(9)
        model = ddsp.Decoder(Big, noise_rng="device", seed=3).cuda()
        return model, ddsp.MSSLoss().cuda(), make_adam(model), torch.amp.GradScaler("cuda", init_scale=2.0 ** 24)

    m_e, l_e, o_e, s_e = make()
    m_g, l_g, o_g, s_g = make()
    graphed = ddsp.GraphedTrainStep(m_g, l_g, o_g, x, amp_dtype=torch.float16, scaler=s_g)
    assert s_g.get_scale() == 2.0 ** 24
    before = {k: v.clone() for k, v in m_g.state_dict().items()}
    loss, _ = graphed.step(x)
    assert np.isfinite(float(loss))
    assert s_g.get_scale() == 2.0 ** 24 * s_g.get_backoff_factor()                   # overflow seen inside the replay ...
    assert all(torch.equal(before[k], v) for k, v in m_g.state_dict().items())         # ... and the update skipped, bit for bit
    ddsp.train_step(m_e, l_e, o_e, x, amp_dtype=torch.float16, scaler=s_e)
    assert s_e.get_scale() == s_g.get_scale()
    for i in range(12):
        ddsp.train_step(m_e, l_e, o_e, x, amp_dtype=torch.float16, scaler=s_e)
        graphed.step(x)
        print("skip step", i, s_e.get_scale(), s_g.get_scale())
        assert s_e.get_scale() == s_g.get_scale(), i
    assert all(bool(torch.isfinite(v).all()) for v in m_g.state_dict().values())


def new_trainer(data, tmp, name, **kw):
    kw.setdefault("precision", 32)
    return ddsp.Trainer(Conf, data, n_ffts=(256, 128, 64), log_dir=os.path.join(str(tmp), name), decoder=make_decoder(), seed=3, **kw)


def test_a_changed_learning_rate_reaches_the_captured_update(tmp_path):
    data = examples(96)
    tol = 1e-4

    def run(graphed, halve):
        t = new_trainer(data, tmp_path, f"lr{int(graphed)}{int(halve)}", graphed=graphed)
        t.batches.start_epoch(0)
        t.train_batch()
        first = [p.detach().clone() for p in t.model.parameters()]
        if halve:
            t.set_lr(5e-4)
            assert t.lr == 5e-4
        t.train_batch()
        assert (t._step is not None) == graphed
        return first, [p.detach().clone() for p in t.model.parameters()]

    g1, g2 = run(True, True)
    e1, e2 = run(False, True)
    _, full = run(False, False)
    differs = 0
    for a1, a2, b1, b2, c2 in zip(g1, g2, e1, e2, full):
        assert close(b1, a1, tol) and close(b2, a2, tol)
        differs += not close(c2, a2, tol)
        # the second update itself is half the un-halved one's size, not just close in absolute terms
    assert differs >= len(g2) // 2, differs
    up_g = torch.cat([(b - a).reshape(-1) for a, b in zip(g1, g2)])
    up_e = torch.cat([(b - a).reshape(-1) for a, b in zip(e1, e2)])
    up_f = torch.cat([(b - a).reshape(-1) for a, b in zip(e1, full)])
    print("update norms", float(up_g.norm()), float(up_e.norm()), float(up_f.norm()))
    assert abs(float(up_g.norm()) / float(up_e.norm()) - 1.0) <= 1e-2 and float(up_g.norm()) < 0.75 * float(up_f.norm())


def hand_written_loop(data, epochs, batch_size=32, seed=3):
    model = make_decoder()
    loss_fn, opt = ddsp.MSSLoss((256, 128, 64)).cuda(), make_adam(model)
    order = ddsp.DeviceBatches(data, batch_size, seed=seed, device="cpu")
    means, steps = [], 0
    for epoch in range(epochs):
        losses = []
        for idx in order.permutation(epoch).split(batch_size):
            x = {k: data[k][idx].cuda() for k in tr.KEYS}
            loss, _ = ddsp.train_step(model, loss_fn, opt, x)
            losses.append(float(loss))
            steps += 1
        means.append(sum(losses) / len(losses))
    return model, means, steps


@pytest.mark.parametrize("graphed", [True, False])
def test_fit_equals_the_hand_written_loop(tmp_path, graphed):
    data = examples(70)
    t = new_trainer(data, tmp_path, "fit", graphed=graphed)
    history = t.fit(2)
    model, means, steps = hand_written_loop(data, 2)
    tol = 1e-4
    assert t.global_step == steps == 6 and t.epoch == 2 and (t._step is not None) == graphed
    for (k, a), (_, b) in zip(model.named_parameters(), t.model.named_parameters()):
        assert close(a, b, tol), k
    draws = 2 * (2 * model.noise.draws(32, 40) + model.noise.draws(6, 40))
    assert t.model.noise._offset == model.noise._offset == draws
    if graphed:
        assert int(t._step.counters[0].item()) == draws - model.noise.draws(6, 40)   # (the last, short batch ran eagerly)
    print("epoch means", [h["train_loss"] for h in history], means)
    assert [h["epoch"] for h in history] == [0, 1] and [h["steps"] for h in history] == [3, 3]
    for h, m in zip(history, means):
        assert abs(h["train_loss"] - m) <= tol * abs(m)
    assert sorted(os.listdir(os.path.join(t.run_dir(), "checkpoints"))) == ["epoch=0-step=3.ckpt", "epoch=1-step=6.ckpt"]


def test_resume_continues_as_the_uninterrupted_run(tmp_path):
    data = examples(70)
    whole = new_trainer(data, tmp_path, "whole")
    whole.fit(2)
    first = new_trainer(data, tmp_path, "parts")
    first.fit(1)
    path = ddsp.latest_checkpoint(first.version, first.log_dir)
    assert os.path.basename(path) == "epoch=0-step=3.ckpt"
    second = ddsp.Trainer(Conf, data, precision=32, n_ffts=(256, 128, 64), log_dir=first.log_dir, seed=99, version=first.version)
    second.load(path)
    assert second.epoch == 1 and second.global_step == 3 and second.batches.seed == 3
    assert second.model.noise._offset == first.model.noise._offset and second.model.noise.seed == 3
    second.fit(2)
    tol = 1e-4
    for (k, a), (_, b) in zip(whole.model.named_parameters(), second.model.named_parameters()):
        assert close(a, b, tol), k
    assert second.global_step == whole.global_step == 6 and second.model.noise._offset == whole.model.noise._offset
    assert [h["epoch"] for h in second.history] == [0, 1]
    assert abs(second.history[1]["train_loss"] - whole.history[1]["train_loss"]) <= tol * abs(whole.history[1]["train_loss"])
    # what the real-time program does with the result (rt/utils.py:load_checkpoint -> Decoder)
    state = ddsp.load_checkpoint(first.version, first.log_dir)
    dec = ddsp.Decoder(Conf, noise_rng="device", seed=0)
    dec.load_state_dict(state, strict=True)
    dec = dec.cuda().eval()
    for (k, a), (_, b) in zip(second.model.state_dict().items(), dec.state_dict().items()):
        assert torch.equal(a, b), k
    with torch.no_grad():
        y = dec({k: v for k, v in batch(0).items() if k != "audio"})
    assert y.shape == (3, 40 * 16) and bool(torch.isfinite(y).all())


def test_validation_writes_float32_wav_that_load_audio_reads_back(tmp_path):
    data = examples(70)
    t = new_trainer(data, tmp_path, "val")
    t.batches.start_epoch(0)
    offset = t.model.noise._offset
    paths = t.validate()
    assert t.model.noise._offset == offset and t.model.training          # validating does not move the training noise
    folder = os.path.join(t.run_dir(), "audio")
    assert sorted(os.listdir(folder)) == sorted(f"0-{i}.wav" for i in range(32))     # 1 % of 3 batches: at least one
    assert paths == [os.path.join(folder, f"0-{i}.wav") for i in range(32)]
    t.model.noise._offset = tr._VALIDATION_OFFSET
    audio = t.synthesize_batch(0).cpu().numpy()
    t.model.noise._offset = offset
    assert audio.shape == (32, 640) and float(np.abs(audio).max()) > 0
    for i, p in enumerate(paths):
        pcm, sr = ddsp.load_audio(p)
        assert sr == Conf.sample_rate and pcm.dtype == np.float32 and pcm.shape == (640, 1)
        assert np.array_equal(pcm[:, 0], audio[i]), i
    t2 = new_trainer(data, tmp_path, "val2", limit_val_batches=0.67)
    assert len(t2.validate()) == 64                                      # int(3 * 0.67) = 2 batches
