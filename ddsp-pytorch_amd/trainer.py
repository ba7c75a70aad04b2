"""The reference's trainer (train/train.py: the `Zak` LightningModule and its `main()`), restated on this package's pieces.

  DeviceBatches    `DataLoader(dataset, batch_size, shuffle=True)` for a training set that lives on the device: the four arrays
                   a step reads stay resident, each epoch is one fresh seeded permutation (uploaded once), and a batch is ONE
                   launch of ddsp_gather_batch that fills the step's static input tensors from perm[cursor ..] -- perm and cursor
                   are device memory, so the launch is captured and every graph replay fetches the next batch by itself
  PlateauRate      Adam's learning rate in a device tensor (what a captured update can follow) under the reference's
                   ReduceLROnPlateau(patience=5), which keeps working on the exact host-side float
  Trainer / fit    epochs of gather -> forward -> multi-scale spectral loss -> backward -> Adam as graph replays (a short last
                   batch runs the same maths eagerly), `train_loss` accumulated on the device and read once per epoch, a
                   validation pass that writes audio, Lightning-layout checkpoints that also carry what a resume needs
  load_checkpoint  rt/utils.py:load_checkpoint: the decoder's state of the highest epoch of a version

Single process, as the reference (`gpus=1`).  Documented departures: validation audio is written as float32 WAV through
scipy.io.wavfile (the reference's 16-bit rounding is soundfile's; `load_audio` reads these files back bit-exactly); the
validation batches are the first ones of the epoch's own permutation and draw their noise from a stream of their own, so that
validating does not move the training noise; precision=16 trains with a fused capturable Adam, whose step takes the loss scale
and the overflow flag on the device.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch

from . import _lib
from .decoder import Decoder
from .graphed import GraphedTrainStep
from .training import MSSLoss, train_step

KEYS = ('f0', 'loudness', 'normalized_cents', 'audio')      # decoder.py:333-349 reads the first three, the loss the last
BAD_INDEX, BAD_CURSOR = 1, 2                                # include/ddsp_hip.h: DDSP_GATHER_BAD_*
_VALIDATION_OFFSET = 1 << 60                                # Philox offsets of the validation draws: far from any training draw


def gather_batch(arrays, out, perm, cursor, rows: int, error, advance: bool = True) -> None:
    """ddsp_gather_batch: out[k][r] = arrays[k][perm[cursor + r]] for r < rows and every key of `out`, in one launch; then
    cursor += rows (a second, one-thread launch) when `advance`.  arrays[k] [E, ...] and out[k] [>= rows, ...] contiguous fp32
    CUDA tensors with equal row shapes, perm int64 [n], cursor int64 [1], error int32 [1] (bits BAD_INDEX / BAD_CURSOR are OR-ed
    in; such rows are zero-filled and nothing is read for them)."""
    keys = list(out)
    n = len(keys)
    E = arrays[keys[0]].shape[0]
    for k in keys:
        a, o = arrays[k], out[k]
        if not (a.is_cuda and o.is_cuda and a.dtype == o.dtype == torch.float32 and a.is_contiguous() and o.is_contiguous()):
            raise ValueError(f"gather_batch: '{k}' must be contiguous float32 CUDA tensors")
        if a.shape[0] != E or o.shape[0] < rows or a.shape[1:] != o.shape[1:]:
            raise ValueError(f"gather_batch: '{k}' has shapes {tuple(a.shape)} -> {tuple(o.shape)} for {rows} rows of {E} examples")
    if perm.dtype != torch.int64 or cursor.dtype != torch.int64 or error.dtype != torch.int32 or not perm.is_contiguous():
        raise ValueError("gather_batch: perm and cursor are int64, error is int32")
    src = (ctypes.c_void_p * n)(*[arrays[k].data_ptr() for k in keys])
    dst = (ctypes.c_void_p * n)(*[out[k].data_ptr() for k in keys])
    lens = (ctypes.c_long * n)(*[arrays[k][0].numel() for k in keys])
    with torch.cuda.device(perm.device):
        rc = _lib.lib().ddsp_gather_batch(src, dst, lens, n, perm.data_ptr(), cursor.data_ptr(), perm.numel(), E, int(rows),
                                          1 if advance else 0, error.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ddsp_gather_batch")


class DeviceBatches:
    """The training loader: `dataset` is a PLHDataset or a dict of equally long tensors with its keys; `f0`, `loudness`,
    `normalized_cents` and `audio` move to `device` once and stay there (`harmonicity` and `probabilities` are inputs of neither
    the decoder nor the loss).  Order as DataLoader(shuffle=True, drop_last=False): per epoch one permutation of all examples
    from a torch.Generator seeded by (seed, epoch); the last batch may be short.

    On CUDA `fetch()` is one ddsp_gather_batch launch into the static tensors `self.batch` (full batches) or into fresh ones (a
    short batch); the cursor advances on the device.  On CPU tensors it is index_select with a host cursor: the same order."""

    def __init__(self, dataset, batch_size: int, shuffle: bool = True, seed: int = 0, device=None):
        data = dataset.final if hasattr(dataset, 'final') else dataset
        missing = [k for k in KEYS if k not in data]
        if missing:
            raise ValueError(f"DeviceBatches: the dataset lacks {missing}")
        if device is None:
            device = data['audio'].device if data['audio'].is_cuda else ('cuda' if torch.cuda.is_available() else 'cpu')
        self.device = torch.device(device)
        self.data = {k: data[k].detach().to(device=self.device, dtype=torch.float32).contiguous() for k in KEYS}
        self.n_examples = int(self.data['audio'].shape[0])
        if any(v.shape[0] != self.n_examples for v in self.data.values()) or self.n_examples == 0:
            raise ValueError("DeviceBatches: the arrays must hold the same, positive number of examples")
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        if self.batch_size <= 0:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        self.batch = {k: torch.zeros((self.batch_size,) + tuple(v.shape[1:]), device=self.device) for k, v in self.data.items()}
        self.perm = torch.arange(self.n_examples, dtype=torch.int64, device=self.device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.error = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._pos = 0                                       # what the cursor holds (host-side knowledge)

    def __len__(self):
        return (self.n_examples + self.batch_size - 1) // self.batch_size

    def batch_sizes(self):
        full, rest = divmod(self.n_examples, self.batch_size)
        return [self.batch_size] * full + ([rest] if rest else [])

    def permutation(self, epoch: int) -> torch.Tensor:
        """The order of epoch `epoch` (CPU int64): reproducible from (seed, epoch) alone."""
        if not self.shuffle:
            return torch.arange(self.n_examples, dtype=torch.int64)
        g = torch.Generator()
        g.manual_seed((self.seed * 1_000_003 + int(epoch)) & ((1 << 63) - 1))
        return torch.randperm(self.n_examples, generator=g)

    def start_epoch(self, epoch: int) -> None:
        """Upload the epoch's permutation (the one host-to-device copy of the epoch) and rewind the cursor."""
        self.perm.copy_(self.permutation(epoch), non_blocking=True)
        self.cursor.zero_()
        self._pos = 0

    def remaining(self) -> int:
        return self.n_examples - self._pos

    def advanced(self, rows: int) -> None:
        """A captured fetch was replayed: the device cursor moved by `rows`."""
        self._pos += rows

    def fetch(self, rows: int | None = None):
        """The next `rows` examples (default: a full batch, or what is left of the epoch).  A full batch comes in the static
        tensors `self.batch`, which the next full fetch overwrites; a short one in tensors of its own."""
        rows = min(self.batch_size, self.remaining()) if rows is None else int(rows)
        if rows <= 0 or rows > self.remaining():
            raise IndexError(f"DeviceBatches: {rows} rows asked for, {self.remaining()} left in this epoch")
        if self.device.type != 'cuda':
            idx = self.perm[self._pos:self._pos + rows]
            self._pos += rows
            return {k: v.index_select(0, idx) for k, v in self.data.items()}
        out = self.batch if rows == self.batch_size else \
            {k: torch.empty((rows,) + tuple(v.shape[1:]), device=self.device) for k, v in self.data.items()}
        gather_batch(self.data, out, self.perm, self.cursor, rows, self.error)
        self._pos += rows
        return out

    def fetch_static(self) -> None:
        """The launch a graph captures: a full batch into `self.batch`, cursor advanced on the device (host side: `advanced`)."""
        gather_batch(self.data, self.batch, self.perm, self.cursor, self.batch_size, self.error)

    def epoch(self, epoch: int):
        """Iterate the batches of one epoch (dicts; a full batch's tensors are overwritten by the next full batch)."""
        self.start_epoch(epoch)
        while self.remaining():
            yield self.fetch()

    def check(self, error_word: int | None = None) -> None:
        """Raise if a fetch met an index it could not use (`error_word`: the word if the caller has already read it)."""
        word = int(self.error.item()) if error_word is None else int(error_word)
        if word:
            self.error.zero_()
            what = [name for bit, name in ((BAD_INDEX, "an example index outside the training set"),
                                           (BAD_CURSOR, "a cursor outside the permutation")) if word & bit]
            raise _lib.DdspHipError("DeviceBatches: " + " and ".join(what) + " (the rows were zero-filled, nothing was read)")


class PlateauRate:
    """The learning rate of `optimizer` under torch's ReduceLROnPlateau, for an optimiser whose rate is a tensor (a captured
    update reads it; `Adam(lr=torch.tensor(...))`) or a plain float.  The scheduler always works on the exact Python float, so
    the sequence is stock ReduceLROnPlateau's; every new value is then written into the tensor in place."""

    def __init__(self, optimizer, patience: int = 5, lr: float | None = None, **kwargs):
        self.opt = optimizer
        self._tensors = [g['lr'] if torch.is_tensor(g['lr']) else None for g in optimizer.param_groups]
        # (`lr`: the exact initial rate -- an fp32 tensor holds 1e-3 only to 24 bits, and the schedule continues from this float)
        self._floats = [float(g['lr']) if lr is None else float(lr) for g in optimizer.param_groups]
        with self._as_floats():
            self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=patience, **kwargs)

    class _Swap:
        def __init__(self, owner):
            self.o = owner

        def __enter__(self):
            for g, f in zip(self.o.opt.param_groups, self.o._floats):
                g['lr'] = f

        def __exit__(self, *exc):
            o = self.o
            o._floats = [float(g['lr']) for g in o.opt.param_groups]
            for g, t, f in zip(o.opt.param_groups, o._tensors, o._floats):
                if t is not None:
                    t.fill_(f)
                    g['lr'] = t

    def _as_floats(self):
        return PlateauRate._Swap(self)

    @property
    def lr(self):
        return self._floats[0] if len(self._floats) == 1 else list(self._floats)

    def step(self, metric: float):
        """One epoch's monitored value (train/train.py:21-30: `train_loss`, once per epoch) -> the rate from here on."""
        with self._as_floats():
            self.scheduler.step(float(metric))
        return self.lr

    def set(self, value: float) -> None:
        with self._as_floats():
            for g in self.opt.param_groups:
                g['lr'] = float(value)

    def state_dict(self):
        return {'scheduler': self.scheduler.state_dict(), 'lr': list(self._floats)}

    def load_state_dict(self, state) -> None:
        self.scheduler.load_state_dict(state['scheduler'])
        with self._as_floats():
            for g, f in zip(self.opt.param_groups, state['lr']):
                g['lr'] = float(f)


# ------------------------------------------------------------------------------------------------------------ checkpoints

def checkpoint_dir(root, version: int) -> str:
    return os.path.join(root, f'version_{version}', 'checkpoints')


def checkpoint_name(epoch: int, step: int) -> str:
    return f'epoch={epoch}-step={step}.ckpt'


def _checkpoint_epoch(name: str) -> int:
    m = re.match(r'epoch=(\d+)', os.path.basename(name))
    return int(m.group(1)) if m else -1


def latest_checkpoint(version: int, root=None) -> str:
    """The checkpoint of the highest epoch (compared as a number) under root/version_N/checkpoints; root defaults to
    ./lightning_logs, where the reference's trainer writes."""
    root = os.path.join(os.getcwd(), 'lightning_logs') if root is None else root
    folder = checkpoint_dir(root, version)
    files = [f for f in (os.listdir(folder) if os.path.isdir(folder) else []) if f.endswith('.ckpt') and _checkpoint_epoch(f) >= 0]
    if not files:
        raise FileNotFoundError(f"no checkpoint under {folder}")
    return os.path.join(folder, max(files, key=_checkpoint_epoch))


def load_checkpoint(version: int, root=None, map_location='cpu'):
    """rt/utils.py:load_checkpoint: the newest checkpoint of `version` -> the decoder's state dict (the entries stored under the
    LightningModule's attribute name `model.`, prefix removed), for `Decoder.load_state_dict(strict=True)`."""
    state = torch.load(latest_checkpoint(version, root), map_location=map_location, weights_only=True)['state_dict']
    return {k[len('model.'):]: v for k, v in state.items() if k.startswith('model.')}


def checkpoint_state(model, loss_fn, optimizer, rate, scaler, *, epoch: int, global_step: int, loader: dict, precision, history) -> dict:
    """What a checkpoint holds, on the CPU: Lightning's entries (`state_dict` with the decoder under `model.` and the loss under
    `loss.`, `epoch` = epochs finished, `global_step`, `optimizer_states`, `lr_schedulers`) plus what a resume needs beyond
    them: the scaler, the loader's seed, the FilteredNoise Philox seed and offset, the epoch history."""
    sd = {'model.' + k: v.detach().cpu() for k, v in model.state_dict().items()}
    sd.update({'loss.' + k: v.detach().cpu() for k, v in loss_fn.state_dict().items()})
    opt = optimizer.state_dict()
    opt = {'state': {i: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in opt['state'].items()},
           'param_groups': [{k: (float(v) if torch.is_tensor(v) else v) for k, v in g.items()} for g in opt['param_groups']]}
    return {'epoch': int(epoch), 'global_step': int(global_step), 'state_dict': sd, 'optimizer_states': [opt],
            'lr_schedulers': [rate.state_dict()], 'scaler': None if scaler is None else scaler.state_dict(),
            'loader': dict(loader), 'noise': {'seed': int(model.noise.seed), 'offset': int(model.noise._offset)},
            'precision': str(precision), 'history': list(history)}


def write_checkpoint(state: dict, root, version: int) -> str:
    """root/version_N/checkpoints/epoch=E-step=S.ckpt, E the last finished epoch counted from 0 (as Lightning names them)."""
    folder = checkpoint_dir(root, version)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, checkpoint_name(state['epoch'] - 1, state['global_step']))
    torch.save(state, path)
    return path


def _next_version(root) -> int:
    taken = [int(m.group(1)) for m in (re.fullmatch(r'version_(\d+)', d) for d in (os.listdir(root) if os.path.isdir(root) else [])) if m]
    return max(taken) + 1 if taken else 0


# ---------------------------------------------------------------------------------------------------------------- trainer

_PRECISIONS = {16: torch.float16, 'bf16': torch.bfloat16, 32: None}


class Trainer:
    """`pl.Trainer(gpus=1, limit_val_batches=0.01, precision=16).fit(Zak(), loader, loader)` of train/train.py:46-51.

    conf: the reference's Config fields the Decoder reads, plus `batch_size`.  dataset: a PLHDataset or a dict with its keys.
    precision: 16 (fp16 autocast + GradScaler, the reference's), 'bf16' or 32.  graphed: full batches as hipGraph replays of
    gather -> step (False: every batch eagerly through `train_step`, the same maths).  The optimiser is Adam(lr) fused and
    capturable with its rate in a device tensor; `patience` is ReduceLROnPlateau's.  `decoder`: train this one instead of a
    fresh `Decoder(conf, noise_rng='device', seed=seed)`.  `log_dir/version_N` (N: the first unused number unless `version` is
    given) receives `checkpoints/epoch=E-step=S.ckpt` after every epoch and `audio/{batch}-{i}.wav` from the validation pass."""

    def __init__(self, conf, dataset, *, precision=16, graphed: bool = True, lr: float = 1e-3, patience: int = 5, seed: int = 0,
                 log_dir='lightning_logs', version: int | None = None, batch_size: int | None = None,
                 n_ffts=(2048, 1024, 512, 256, 128, 64), limit_val_batches: float = 0.01, decoder=None, device='cuda'):
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be 16, 'bf16' or 32, got {precision!r}")
        self.conf, self.precision, self.graphed = conf, precision, bool(graphed)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.DdspHipError("Trainer needs a GPU (the decoder has no CPU path)")
        self.amp_dtype = _PRECISIONS[precision]
        self.model = (decoder if decoder is not None else Decoder(conf, noise_rng='device', seed=seed)).to(self.device)
        self.loss_fn = MSSLoss(tuple(n_ffts)).to(self.device)
        self.batches = DeviceBatches(dataset, batch_size or conf.batch_size, shuffle=True, seed=seed, device=self.device)
        params = [p for p in self.model.parameters() if p.requires_grad]
        self.optimizer = torch.optim.Adam(params, lr=torch.tensor(float(lr), device=self.device), fused=True, capturable=True)
        self.rate = PlateauRate(self.optimizer, patience=patience, lr=float(lr))
        self.scaler = torch.amp.GradScaler('cuda') if self.amp_dtype is torch.float16 else None
        self.log_dir, self.version = log_dir, version
        self.limit_val_batches = limit_val_batches
        self.sample_rate = conf.sample_rate
        self.epoch, self.global_step = 0, 0
        self.history = []                                   # per epoch: {'epoch', 'train_loss', 'lr', 'steps'}
        self._loss_sum = torch.zeros((), device=self.device)
        self._step = None                                   # GraphedTrainStep, captured at the first full batch

    # ---- learning rate
    @property
    def lr(self) -> float:
        return self.rate.lr

    def set_lr(self, value: float) -> None:
        """A new learning rate from the next step on, eager or replayed (the captured update reads the tensor this writes)."""
        self.rate.set(value)

    # ---- one batch
    def train_batch(self, rows: int | None = None) -> torch.Tensor:
        """The next batch of the running epoch -> its loss (a device scalar).  Full batches replay the graph when `graphed`."""
        b = self.batches
        rows = min(b.batch_size, b.remaining()) if rows is None else rows
        if self.graphed and rows == b.batch_size:
            if self._step is None:
                self._build_graph()
            loss, _ = self._step.step()
            b.advanced(rows)
        else:
            loss, _ = train_step(self.model, self.loss_fn, self.optimizer, b.fetch(rows), amp_dtype=self.amp_dtype, scaler=self.scaler)
        self._loss_sum += loss
        self.global_step += 1
        return loss

    def _build_graph(self) -> None:
        b = self.batches
        cursor, pos = b.cursor.clone(), b._pos
        b.fetch_static()                                    # eagerly once: the warm-up needs real rows in the static inputs
        b.cursor.copy_(cursor)
        self._step = GraphedTrainStep(self.model, self.loss_fn, self.optimizer, b.batch, amp_dtype=self.amp_dtype, scaler=self.scaler,
                                      prologue=b.fetch_static, static_batch=True)
        b.cursor.copy_(cursor)                              # (capturing executes nothing; the eager fetch above was rewound)
        b._pos = pos

    # ---- epochs
    def fit(self, max_epochs: int):
        """Train until `max_epochs` epochs are done (counting those of a resumed checkpoint).  Returns the history."""
        while self.epoch < max_epochs:
            self.train_epoch()
            self.validate()
            self.epoch += 1
            self.save_checkpoint()
        return self.history

    def train_epoch(self) -> float:
        """Every batch of epoch `self.epoch` once, then the epoch's ONE device-to-host read (the loss sum and the loader's error
        word together) and the plateau schedule's step on the mean `train_loss`, which is returned and logged in `history`."""
        b = self.batches
        self.model.train()
        b.start_epoch(self.epoch)
        self._loss_sum.zero_()
        sizes = b.batch_sizes()
        for rows in sizes:
            self.train_batch(rows)
        loss_sum, error = torch.stack((self._loss_sum.double(), b.error[0].double())).tolist()
        b.check(int(error))
        mean = loss_sum / len(sizes)
        lr_used = self.lr
        self.rate.step(mean)
        self.history.append({'epoch': self.epoch, 'train_loss': mean, 'lr': lr_used, 'steps': len(sizes)})
        return mean

    # ---- validation (train.py:39-44 with limit_val_batches of the training loader)
    def run_dir(self) -> str:
        if self.version is None:
            self.version = _next_version(self.log_dir)
        return os.path.join(self.log_dir, f'version_{self.version}')

    def validate(self):
        """Synthesise limit_val_batches of the loader's batches (at least one) without gradients and write every row as
        audio/{batch}-{i}.wav (float32).  Returns the paths."""
        from scipy.io import wavfile
        b = self.batches
        n_val = max(1, int(len(b) * self.limit_val_batches))
        folder = os.path.join(self.run_dir(), 'audio')
        os.makedirs(folder, exist_ok=True)
        noise = self.model.noise
        seed, offset = noise.seed, noise._offset
        noise._offset = _VALIDATION_OFFSET
        paths = []
        self.model.eval()
        try:
            for i_batch in range(n_val):
                audio = self.synthesize_batch(i_batch).cpu().numpy()
                for i, row in enumerate(audio):
                    paths.append(os.path.join(folder, f'{i_batch}-{i}.wav'))
                    wavfile.write(paths[-1], self.sample_rate, row)
        finally:
            noise.reseed(seed, offset)
            self.model.train()
        return paths

    def synthesize_batch(self, i_batch: int) -> torch.Tensor:
        """The decoder's audio [rows, samples] (fp32) for batch `i_batch` of the current epoch's order, without gradients, under
        the trainer's autocast.  Draws noise from the model's current offset like any eager forward."""
        b = self.batches
        idx = b.permutation(self.epoch)[i_batch * b.batch_size:(i_batch + 1) * b.batch_size].to(self.device)
        keys = KEYS if getattr(self.model, 'z_dims', 0) > 0 else KEYS[:3]      # a timbre latent is computed from the audio
        z = {k: b.data[k].index_select(0, idx) for k in keys}
        with torch.no_grad(), torch.autocast('cuda', dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None):
            return self.model(z).float()

    # ---- checkpoints
    def state(self) -> dict:
        return checkpoint_state(self.model, self.loss_fn, self.optimizer, self.rate, self.scaler, epoch=self.epoch,
                                global_step=self.global_step, loader={'seed': self.batches.seed, 'batch_size': self.batches.batch_size},
                                precision=self.precision, history=self.history)

    def save_checkpoint(self) -> str:
        self.run_dir()
        return write_checkpoint(self.state(), self.log_dir, self.version)

    def load(self, path: str) -> None:
        """Continue from a checkpoint this class wrote: weights, optimiser, rate schedule, scaler, counters, loader seed and the
        noise stream.  The next `fit(n)` runs epochs `epoch .. n - 1` as the uninterrupted run would have."""
        ck = torch.load(path, map_location='cpu', weights_only=True)
        self.model.load_state_dict({k[len('model.'):]: v for k, v in ck['state_dict'].items() if k.startswith('model.')}, strict=True)
        self._step = None                                   # (the optimiser's state tensors are replaced: capture again)
        self.optimizer.load_state_dict(ck['optimizer_states'][0])
        for g, t in zip(self.optimizer.param_groups, self.rate._tensors):
            g['lr'] = t                                     # (load_state_dict put the saved floats there; the tensor stays the rate's home)
        self.rate.load_state_dict(ck['lr_schedulers'][0])
        if self.scaler is not None and ck.get('scaler'):
            self.scaler.load_state_dict(ck['scaler'])
        self.epoch, self.global_step, self.history = int(ck['epoch']), int(ck['global_step']), list(ck['history'])
        self.batches.seed = int(ck['loader']['seed'])
        self.model.noise.reseed(ck['noise']['seed'], ck['noise']['offset'])

