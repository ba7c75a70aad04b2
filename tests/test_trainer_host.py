"""CPU-side checks of the trainer (ddsp_pytorch_amd.trainer): the loader's ordering logic, the checkpoint layout
rt/utils.py:load_checkpoint of the reference reads, the plateau schedule on a tensor-valued rate, and the new C symbol."""
import ctypes
import os
import re

import torch
import torch.nn as nn

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import trainer as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 16, 9, 4000, 16
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 256, 2, 64, 1


def examples(E, T=40, hop=16, seed=5):
    """Synthetic examples with PLHDataset's keys and shapes; row e of every array carries e in its first element."""
    g = torch.Generator().manual_seed(seed)
    data = {"f0": 100 + 200 * torch.rand(E, T, 1, generator=g), "harmonicity": torch.rand(E, T, 1, generator=g),
            "loudness": torch.rand(E, T, 1, generator=g) * 2 - 1, "probabilities": torch.rand(E, T, 8, generator=g),
            "normalized_cents": torch.rand(E, T, 1, generator=g), "audio": 0.1 * torch.randn(E, T * hop, generator=g)}
    for k in tr.KEYS:
        data[k].view(E, -1)[:, 0] = torch.arange(E, dtype=torch.float32)
    return data


def test_device_batches_on_cpu_orders_like_a_shuffled_dataloader():
    data = examples(70)
    b = ddsp.DeviceBatches(data, 32, shuffle=True, seed=3, device="cpu")
    assert len(b) == 3 and b.batch_sizes() == [32, 32, 6]
    assert set(b.data) == set(tr.KEYS)                       # harmonicity / probabilities stay where they were
    epochs = []
    for epoch in range(3):
        rows, sizes = [], []
        for batch in b.epoch(epoch):
            sizes.append(batch["audio"].shape[0])
            ids = batch["audio"][:, 0].long()
            for k in tr.KEYS:                                # every key's rows are the same examples, whole
                assert torch.equal(batch[k].view(len(ids), -1)[:, 0].long(), ids), k
                assert torch.equal(batch[k], data[k].index_select(0, ids)), k
            rows.append(ids)
        assert sizes == [32, 32, 6]
        order = torch.cat(rows)
        assert torch.equal(order, b.permutation(epoch))
        assert sorted(order.tolist()) == list(range(70))
        epochs.append(order)
    assert not torch.equal(epochs[0], epochs[1]) and not torch.equal(epochs[1], epochs[2]) and not torch.equal(epochs[0], epochs[2])
    again = ddsp.DeviceBatches(data, 32, shuffle=True, seed=3, device="cpu")
    for epoch in (2, 0, 1):                                  # reproducible from (seed, epoch), in any order of asking
        assert torch.equal(torch.cat([x["audio"][:, 0].long() for x in again.epoch(epoch)]), epochs[epoch])
    other = ddsp.DeviceBatches(data, 32, shuffle=True, seed=4, device="cpu")
    assert not torch.equal(other.permutation(0), epochs[0])
    plain = ddsp.DeviceBatches(data, 32, shuffle=False, device="cpu")
    for epoch in range(2):
        assert torch.equal(torch.cat([x["f0"][:, 0, 0].long() for x in plain.epoch(epoch)]), torch.arange(70))
    # asking for more than the epoch has left is an error, not a wrap-around
    plain.start_epoch(0)
    plain.fetch(), plain.fetch()
    try:
        plain.fetch(7)
        raise AssertionError("7 rows out of 6")
    except IndexError:
        pass
    assert plain.fetch()["f0"].shape[0] == 6


def test_checkpoint_layout_and_highest_epoch_is_numeric(tmp_path):
    torch.manual_seed(2)
    model = ddsp.Decoder(Conf)
    loss_fn = ddsp.MSSLoss((256, 128, 64))
    opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(1e-3))
    rate = ddsp.PlateauRate(opt, patience=5, lr=1e-3)
    root = str(tmp_path / "lightning_logs")
    wanted = None
    for epochs_done, step in ((10, 30), (11, 33), (3, 9)):       # files epoch=9, epoch=10 and epoch=2
        with torch.no_grad():
            model.controller.dense_loudness.bias.fill_(float(epochs_done))
        state = tr.checkpoint_state(model, loss_fn, opt, rate, None, epoch=epochs_done, global_step=step,
                                    loader={"seed": 7, "batch_size": 32}, precision=32, history=[])
        path = tr.write_checkpoint(state, root, 4)
        assert os.path.basename(path) == f"epoch={epochs_done - 1}-step={step}.ckpt"
        assert os.path.dirname(path) == os.path.join(root, "version_4", "checkpoints")
        if epochs_done == 11:
            wanted = {k: v.clone() for k, v in model.state_dict().items()}
    assert sorted(os.listdir(os.path.join(root, "version_4", "checkpoints"))) == ["epoch=10-step=33.ckpt", "epoch=2-step=9.ckpt",
                                                                                  "epoch=9-step=30.ckpt"]
    assert os.path.basename(ddsp.latest_checkpoint(4, root)) == "epoch=10-step=33.ckpt"      # lexically, epoch=9 sorts last
    raw = torch.load(ddsp.latest_checkpoint(4, root), weights_only=True)
    assert raw["epoch"] == 11 and raw["global_step"] == 33 and raw["loader"]["seed"] == 7 and raw["noise"] == {"seed": 0, "offset": 0}
    assert {k for k in raw["state_dict"] if k.startswith("model.")} == {"model." + k for k in model.state_dict()}
    assert all(k.startswith(("model.", "loss.")) for k in raw["state_dict"])
    state = ddsp.load_checkpoint(4, root)
    assert list(state) == list(model.state_dict())
    fresh = ddsp.Decoder(Conf)
    fresh.load_state_dict(state, strict=True)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, wanted[k]), k
    assert float(fresh.controller.dense_loudness.bias.detach()[0]) == 11.0
    # the default root is ./lightning_logs, as for the reference's real-time program
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert list(ddsp.load_checkpoint(4)) == list(state)
    finally:
        os.chdir(cwd)
    try:
        ddsp.load_checkpoint(5, root)
        raise AssertionError("version 5 does not exist")
    except FileNotFoundError:
        pass


def test_plateau_rate_equals_stock_reduce_lr_on_plateau():
    losses = [5.0, 4.0, 4.1, 4.2, 4.05, 4.3, 4.4, 4.5, 4.6, 3.0, 3.1, 3.2, 3.3, 3.4, 3.5, 3.6, 3.7, 3.8, 3.9, 4.0, 4.1, 4.2, 2.0,
              float("inf"), 2.5, 2.5, 2.5, 2.5, 2.5, 2.5, 2.5, 2.5]
    stock_opt = torch.optim.Adam(nn.Linear(2, 2).parameters(), lr=1e-3)
    stock = torch.optim.lr_scheduler.ReduceLROnPlateau(stock_opt, patience=5)
    want = []
    for v in losses:
        stock.step(v)
        want.append(stock_opt.param_groups[0]["lr"])
    assert len(set(want)) >= 3                                # the list makes the rate drop more than once
    lr = torch.tensor(1e-3)
    opt = torch.optim.Adam(nn.Linear(2, 2).parameters(), lr=lr)
    rate = ddsp.PlateauRate(opt, patience=5, lr=1e-3)
    got = []
    for v in losses:
        got.append(rate.step(v))
        assert opt.param_groups[0]["lr"] is lr                # the optimiser keeps reading the one tensor ...
        assert float(lr) == float(torch.tensor(got[-1]))      # ... which holds the new rate (rounded to fp32)
    assert got == want
    # a resumed schedule continues where the saved one stood
    half = len(losses) // 2
    a = ddsp.PlateauRate(torch.optim.Adam(nn.Linear(2, 2).parameters(), lr=torch.tensor(1e-3)), patience=5, lr=1e-3)
    for v in losses[:half]:
        a.step(v)
    b = ddsp.PlateauRate(torch.optim.Adam(nn.Linear(2, 2).parameters(), lr=torch.tensor(1e-3)), patience=5, lr=1e-3)
    b.load_state_dict(a.state_dict())
    assert [b.step(v) for v in losses[half:]] == want[half:]
    b.set(5e-4)
    assert b.lr == 5e-4 and float(b.opt.param_groups[0]["lr"]) == float(torch.tensor(5e-4))


def test_gather_symbol_is_declared_bound_and_the_abi_is_still_5():
    text = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert re.search(r"\bint\s+ddsp_gather_batch\s*\(", text)
    assert "ddsp_gather_batch" in ddsp._lib.SIGNATURES and list(ddsp._lib.SIGNATURES)[-1] == "ddsp_gather_batch"
    assert "ddsp_trainer.hip" in open(os.path.join(ROOT, "ddsp-pytorch_amd", "csrc", "Makefile")).read()
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION
    assert hasattr(ctypes.CDLL(ddsp._lib.SO_PATH), "ddsp_gather_batch")
    # argument validation happens before anything touches a device
    word = ctypes.c_long(0)
    p = ctypes.addressof(word)
    one = (ctypes.c_void_p * 1)(p)
    lens = (ctypes.c_long * 1)(4)
    assert L.ddsp_gather_batch(None, None, None, 1, None, None, 8, 8, 0, 1, None, None) == 0        # no rows: nothing to do
    assert L.ddsp_gather_batch(None, None, None, 1, None, None, 8, 8, 2, 1, None, None) == -1
    assert L.ddsp_gather_batch(one, one, lens, 9, p, p, 8, 8, 2, 1, p, None) == -1                  # more arrays than the plan holds
    assert L.ddsp_gather_batch(one, one, lens, 1, p, p, -1, 8, 2, 1, p, None) == -1
    bad = (ctypes.c_long * 1)(0)
    assert L.ddsp_gather_batch(one, one, bad, 1, p, p, 8, 8, 2, 1, p, None) == -1                   # an empty row
    odd = (ctypes.c_void_p * 1)(p + 2)
    assert L.ddsp_gather_batch(odd, one, lens, 1, p, p, 8, 8, 2, 1, p, None) == -1                  # not even 4-byte aligned
    assert {"DeviceBatches", "Trainer", "load_checkpoint"} <= set(ddsp.__all__)
