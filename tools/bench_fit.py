"""Time one training epoch at the reference's shape (config/default.py: batch 16, 2 s at 44.1 kHz = 88 064 samples = 172
frames of hop 512, 180 harmonics, 195 noise bands, the six-scale spectral loss) in the forms a user can choose between:

  loader_bf16_graph   DataLoader(PLHDataset, 16, shuffle=True, num_workers=4) -> .cuda() -> GraphedTrainStep.step(batch), bf16
  loader_fp16_eager   the same loader -> eager train_step(..., amp_dtype=fp16, scaler): the reference's precision without a trainer
  fit_bf16_eager      Trainer(precision='bf16', graphed=False): device-resident batches, every step eager
  fit_fp16_eager      Trainer(precision=16, graphed=False)
  fit_bf16_graph      Trainer(precision='bf16', graphed=True): gather -> step as one graph replay
  fit_fp16_graph      Trainer(precision=16, graphed=True): ... with the loss scaling inside the replay

The dataset is synthetic (seeded random tensors with PLHDataset's keys and shapes): nothing is read from disk.  Every form runs
one untimed epoch, then `--epochs` timed ones; within each repeat the forms run in an order rotated by one, so that no form
always follows the same neighbour.  An epoch is timed on the host between two device synchronisations and includes what the
form really pays per epoch (the loader's worker start, the permutation upload, the loss read).  Prints one JSON line;
`--out FILE` also writes it.  `--gather N` instead launches the batch gather N times at this shape (for a kernel trace) and
prints its event-timed mean.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as ddsp  # noqa: E402
from ddsp_pytorch_amd import trainer as tr  # noqa: E402


class Config:                     # config/default.py of the reference
    sample_rate, n_fft, hop_length = 44100, 2048, 512
    n_harmonics, n_noise_filters = 180, 195
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 512, 3, 512, 1
    batch_size = 16


SAMPLES, FRAMES = 88064, 172


def synthetic_dataset(E, seed=0, all_keys=True):
    g = torch.Generator().manual_seed(seed)
    final = {"f0": 100 + 300 * torch.rand(E, FRAMES, 1, generator=g), "loudness": torch.rand(E, FRAMES, 1, generator=g) * 2 - 1,
             "normalized_cents": torch.rand(E, FRAMES, 1, generator=g), "audio": 0.1 * torch.randn(E, SAMPLES, generator=g)}
    if all_keys:                  # what PLHDataset also holds and a DataLoader collates: [E, T, 1] and CREPE's 360 pitch bins
        final["harmonicity"] = torch.rand(E, FRAMES, 1, generator=g)
        final["probabilities"] = torch.rand(E, FRAMES, 360, generator=g)
    ds = ddsp.PLHDataset.__new__(ddsp.PLHDataset)          # the class's own __getitem__ / __len__ over ready-made features
    ds.final = final
    return ds


def make_model():
    torch.manual_seed(0)
    return ddsp.Decoder(Config, noise_rng="device", seed=1).cuda()


class LoaderForm:
    """What the package offered before the trainer: the reference's DataLoader in front of one of the step functions."""

    def __init__(self, ds, graphed):
        from torch.utils.data import DataLoader
        self.loader = DataLoader(ds, batch_size=Config.batch_size, shuffle=True, num_workers=4)
        self.model, self.loss_fn = make_model(), ddsp.MSSLoss().cuda()
        self.steps = len(self.loader)
        if graphed:
            self.opt = torch.optim.Adam(self.model.parameters(), lr=1e-3, capturable=True)
            example = {k: ds.final[k][:Config.batch_size].cuda() for k in tr.KEYS}
            self.graph = ddsp.GraphedTrainStep(self.model, self.loss_fn, self.opt, example, amp_dtype=torch.bfloat16)
        else:
            self.opt = torch.optim.Adam(self.model.parameters(), lr=1e-3)
            self.graph, self.scaler = None, torch.amp.GradScaler("cuda")

    def epoch(self):
        total = torch.zeros((), device="cuda")
        for x in self.loader:
            x = {k: x[k].cuda(non_blocking=True) for k in tr.KEYS}
            if self.graph is not None:
                loss, _ = self.graph.step(x)
            else:
                loss, _ = ddsp.train_step(self.model, self.loss_fn, self.opt, x, amp_dtype=torch.float16, scaler=self.scaler)
            total += loss
        return float(total) / self.steps


class FitForm:
    def __init__(self, ds, precision, graphed):
        self.t = ddsp.Trainer(Config, ds, precision=precision, graphed=graphed, decoder=make_model(), log_dir=os.devnull)
        self.steps = len(self.t.batches)

    def epoch(self):
        mean = self.t.train_epoch()
        self.t.epoch += 1
        return mean


FORMS = {"loader_bf16_graph": lambda ds: LoaderForm(ds, True), "loader_fp16_eager": lambda ds: LoaderForm(ds, False),
         "fit_bf16_eager": lambda ds: FitForm(ds, "bf16", False), "fit_fp16_eager": lambda ds: FitForm(ds, 16, False),
         "fit_bf16_graph": lambda ds: FitForm(ds, "bf16", True), "fit_fp16_graph": lambda ds: FitForm(ds, 16, True)}


def time_gather(ds, n):
    b = ddsp.DeviceBatches(ds, Config.batch_size, device="cuda")
    nbytes = 2 * sum(v[0].numel() * 4 for v in b.data.values()) * Config.batch_size
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_epoch = len(b.batch_sizes())
    for i in range(n + per_epoch):
        if i % per_epoch == 0:
            b.start_epoch(i // per_epoch)
        if i == per_epoch:
            start.record()
        b.fetch(Config.batch_size)
    stop.record()
    torch.cuda.synchronize()
    b.check()
    us = 1e3 * start.elapsed_time(stop) / n
    return {"gather_launches": n, "bytes_moved_per_launch": nbytes, "gather_plus_cursor_us_event_timed": us,
            "note": "event-timed back-to-back launches include the one-thread cursor launch and launch gaps; the kernel's own "
                    "time is the kernel trace's"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--examples", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--gather", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.examples % Config.batch_size:
        raise SystemExit("--examples must be a multiple of 16: GraphedTrainStep.step takes full batches only")
    torch.cuda.set_device(0)
    if args.gather:
        result = time_gather(synthetic_dataset(args.examples, all_keys=False), args.gather)
        result["resident_bytes"] = args.examples * (SAMPLES + 3 * FRAMES) * 4
    else:
        ds = synthetic_dataset(args.examples)
        names = [n for n in args.forms.split(",") if n]
        forms = {n: FORMS[n](ds) for n in names}
        losses = {}
        for n, f in forms.items():                          # untimed: captures, allocator pools, the loader's first fork
            losses[n] = [f.epoch()]
        times = {n: [] for n in names}
        for r in range(args.epochs):
            for n in names[r % len(names):] + names[:r % len(names)]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses[n].append(forms[n].epoch())
                torch.cuda.synchronize()
                times[n].append(time.perf_counter() - t0)
                print(f"repeat {r} {n}: {times[n][-1]:.4f} s", file=sys.stderr, flush=True)
        result = {"shape": {"batch": Config.batch_size, "samples": SAMPLES, "frames": FRAMES, "harmonics": Config.n_harmonics,
                            "noise_bands": Config.n_noise_filters, "examples": args.examples, "steps_per_epoch": args.examples // 16},
                  "epochs_timed": args.epochs, "forms": {}}
        for n in names:
            t = times[n]
            med = statistics.median(t)
            result["forms"][n] = {"epoch_s": [round(v, 5) for v in t], "median_s": round(med, 5), "min_s": round(min(t), 5),
                                  "max_s": round(max(t), 5), "spread_pct": round(100 * (max(t) - min(t)) / med, 2),
                                  "ms_per_step_median": round(1e3 * med / forms[n].steps, 4),
                                  "first_and_last_epoch_loss": [losses[n][0], losses[n][-1]]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
