"""hipGraph-captured synthesis for launch-bound shapes (small batches, the real-time path).

One `harmonics + noise` pass is 7 short kernel launches; at batch 1 their launch gaps and the Python between
them cost more than the kernels.  `GraphedSynth` captures the pass once for a fixed control shape into a
`torch.cuda.CUDAGraph` (the launch path allocates nothing and never synchronises) and replays it per call;
the caller writes the controls into the static input tensors (`f0`, `c`, `a`, `H`) and reads `out`.

With `live=True` the oscillator runs as `OscillatorBank.live` (harmonic_oscillator.py:64-75): the phase state
of batch row 0 is carried from replay to replay inside the graph (state_out -> state_in copy node).  With the overlap-add noise
the live pass runs only `delayed=True`: the noise is the stream of `noise_ola_stream`, whose state (`noise_state`) is advanced by a
copy node in the same way, and `out` is the signal `delay` = n_noise_filters - 2 samples late.
"""
from __future__ import annotations

import torch

from . import _lib
from . import dense
from .filtered_noise import FilteredNoise, noise_forward, noise_ola_stream, ola_stream_state
from .harmonic_oscillator import osc_forward
from .sinusoids import refuse_inharmonic
from .wavetable import refuse_wavetable


_NO_LATENT = ("{what}: the timbre latent (conf.z_dims > 0) is not wired into the graphed live objects -- the z-encoder's GRU state "
              "would have to be carried by the graph; run AutoEncoder.forward_live / Decoder.forward_live, which carry "
              "(decoder_hidden, z_hidden), or build the decoder without z_dims")


class GraphedSynth:
    def __init__(self, conf, batch: int, frames: int, n_noise_filters: int, device="cuda", live: bool = False,
                 noise_seed: int = 0, delayed: bool = False):
        if live and int(getattr(conf, 'z_dims', 0) or 0) > 0:
            raise ValueError(_NO_LATENT.format(what="GraphedSynth(live=True)"))
        if live:
            refuse_wavetable((getattr(conf, 'synth', None) or 'harmonic') == 'wavetable', "GraphedSynth(live=True)")
            refuse_inharmonic((getattr(conf, 'synth', None) or 'harmonic') == 'inharmonic', "GraphedSynth(live=True)")
        self.hop, self.sample_rate, self.live = conf.hop_length, conf.sample_rate, live
        dev = torch.device(device)
        H = conf.n_harmonics
        self.f0 = torch.full((batch, frames, 1), 100.0, device=dev)
        self.c = torch.ones((batch, frames, H), device=dev)
        self.a = torch.ones((batch, frames, 1), device=dev)
        self.H = torch.ones((batch, frames, n_noise_filters), device=dev)
        self.state = torch.zeros(H, device=dev)           # last_phases (fp32, as after the reference's first live call)
        self.seed = noise_seed
        self.overlap_add = bool(getattr(conf, 'noise_overlap_add', False))
        if live and self.overlap_add and not delayed:
            raise ValueError("the live pass runs the overlap-add noise (noise_overlap_add) only as a stream that carries its tail from "
                             "block to block and emits the audio n_noise_filters - 2 samples late: pass delayed=True to accept that")
        if delayed and not (live and self.overlap_add):
            raise ValueError("delayed=True is the stream form of the overlap-add noise (noise_overlap_add) in the live pass (live=True); "
                             "the truncated noise has nothing to delay")
        self.delayed = delayed
        self.delay = n_noise_filters - 2 if delayed else 0
        self.noise_state = ola_stream_state(batch, n_noise_filters, dev) if delayed else None
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)     # Philox offset of the next call's draw
        self._draws_per_call = batch * frames * ((conf.hop_length + 3) // 4)
        self.out = None
        self._graph = None
        self._capture()

    def _pass(self):
        if self.live:
            y, new_state, _ = osc_forward(self.f0, self.c, self.a, self.hop, self.sample_rate, live_in=self.state,
                                          want_live_out=True)
            self.state.copy_(new_state)
        else:
            y, _, _ = osc_forward(self.f0, self.c, self.a, self.hop, self.sample_rate)
        # the Philox offset of the draw lives on the device and advances inside the graph: every replay is fresh noise,
        # the same sequence as un-captured calls with offset = call index x draws per call
        if self.delayed:
            y, new_noise = noise_ola_stream(self.H, self.hop, self.noise_state, dry=y, seed=self.seed, counter=self._step)
            self.noise_state.copy_(new_noise)
        else:
            y = noise_forward(self.H, self.hop, seed=self.seed, out=y, accumulate=True, counter=self._step, overlap_add=self.overlap_add)
        self._step.add_(self._draws_per_call)
        return y

    def _capture(self):
        if not self.f0.is_cuda:
            raise _lib.DdspHipError("GraphedSynth needs a GPU")
        saved = self.state.clone()

        def restore():
            self.state.copy_(saved)
            self._step.zero_()
            if self.noise_state is not None:
                self.noise_state.zero_()

        restore()
        side = torch.cuda.Stream(device=self.f0.device)
        side.wait_stream(torch.cuda.current_stream(self.f0.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._pass()                      # warm-up: lazy one-time attribute calls, allocator pools
        torch.cuda.current_stream(self.f0.device).wait_stream(side)
        restore()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self.out = self._pass()
        restore()

    def run(self):
        """Replay the captured pass on the current controls; returns the static output tensor [B, T*hop]."""
        self._graph.replay()
        return self.out

    def __call__(self, ctrl):
        for name in ("f0", "c", "a", "H"):
            getattr(self, name).copy_(ctrl[name], non_blocking=True)
        return self.run()


class GraphedLiveDecoder:
    """The whole real-time callback (rt/synth.py:40-55 -> `Decoder.forward_live`, decoder.py:139-147) as ONE hipGraph:
    controller (MLPs, GRU recurrence, heads) -> harmonics.live + noise -> reverb.live_forward.  Per callback the host does
    three small H2D copies into the static inputs, one replay and one D2H of the audio.  Every piece of state stays on
    the device and is advanced by nodes of the graph: the oscillator phases (`state`), the reverb's one-second history
    (`decoder.reverb.buffer`), the Philox offset of the noise draw, with `delayed=True` (a decoder with the overlap-add noise: the
    audio comes `delay` = n_noise_filters - 2 samples late) the noise stream's tail and dry history (`noise_state`), and
    the GRU state (`hidden_out`; the reference hands the callback's INPUT state back, SURVEY App. C.7 -- `carry_hidden=True` feeds the new one forward instead).
    """

    def __init__(self, decoder, frames: int, noise_seed: int = 0, carry_hidden: bool = False, delayed: bool = False):
        if getattr(decoder, 'z_dims', 0) > 0:
            raise ValueError(_NO_LATENT.format(what="GraphedLiveDecoder"))
        refuse_wavetable(decoder, "GraphedLiveDecoder")
        refuse_inharmonic(decoder, "GraphedLiveDecoder")
        decoder.check_live(delayed, "GraphedLiveDecoder")
        self.dec = decoder.eval()
        dev = next(decoder.parameters()).device
        if dev.type != "cuda":
            raise _lib.DdspHipError("GraphedLiveDecoder needs the decoder on a GPU")
        osc = decoder.harmonics
        self.hop, self.sample_rate = osc.hop_size, osc.sample_rate
        self.frames, self.seed, self.carry_hidden = frames, noise_seed, carry_hidden
        self.z = {k: torch.zeros(1, frames, 1, device=dev) for k in ("normalized_cents", "loudness", "f0")}
        self.z["f0"].fill_(100.0)
        units = decoder.controller.gru.hidden_size
        self.hidden = torch.zeros(1, 1, units, device=dev)
        self.hidden_out = torch.zeros(1, 1, units, device=dev)
        self.state = osc.last_phases.data.detach().to(device=dev, dtype=torch.float32).clone()
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)
        self._draws_per_call = frames * ((self.hop + 3) // 4)
        n_filters = decoder.controller.dense_filter.out_features
        self.delayed = delayed
        self.delay = n_filters - 2 if delayed else 0
        self.noise_state = ola_stream_state(1, n_filters, dev) if delayed else None
        self.out = None
        self._capture()

    def _pass(self):
        with torch.no_grad():
            ctrl, _ = self.dec.controller(self.z, self.hidden)
            y, new_state, _ = osc_forward(ctrl["f0"], ctrl["c"], ctrl["a"], self.hop, self.sample_rate, live_in=self.state,
                                          want_live_out=True)
            self.state.copy_(new_state)
            if self.delayed:
                y, new_noise = noise_ola_stream(ctrl["H"], self.hop, self.noise_state, dry=y, seed=self.seed, counter=self._step)
                self.noise_state.copy_(new_noise)
            else:
                noise_forward(ctrl["H"], self.hop, seed=self.seed, out=y, accumulate=True, counter=self._step)
            self._step.add_(self._draws_per_call)
            audio = self.dec.reverb.live_forward(y)
            self.hidden_out.copy_(ctrl["hidden"])
            if self.carry_hidden:
                self.hidden.copy_(ctrl["hidden"])
            return audio.contiguous()

    def _capture(self):
        dev = self.state.device
        keep = (self.state.clone(), self.dec.reverb.buffer.data.clone(), self.hidden.clone())

        def restore():
            self.state.copy_(keep[0])
            self.dec.reverb.buffer.data.copy_(keep[1])
            self.hidden.copy_(keep[2])
            self._step.zero_()
            if self.noise_state is not None:
                self.noise_state.zero_()

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._pass()                      # warm-up: FFT plans, library handles, allocator pools
        torch.cuda.current_stream(dev).wait_stream(side)
        restore()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self.out = self._pass()
        restore()

    def run(self, z):
        """z: dict of `normalized_cents`, `loudness`, `f0`, each [1, frames, 1] (numpy or tensor) -> audio [frames*hop] (numpy)."""
        for k, buf in self.z.items():
            v = z[k]
            buf.copy_(v if torch.is_tensor(v) else torch.from_numpy(v), non_blocking=True)
        self._graph.replay()
        return self.out.cpu().squeeze(0).numpy()


class GraphedTrainStep:
    """`training.train_step` for a FIXED batch shape as hipGraph replays: forward, spectral loss, backward and the optimiser
    update of one step are captured once (about 280 launches at the training shape, whose host-side issue time had become as
    long as the GPU's work); a step is then the copies of the batch into the static input tensors and one replay (with more
    than one rank: replay forward + backward, ONE eager flat all-reduce, replay the update).

    * `optimizer` must be capturable (`torch.optim.Adam(..., capturable=True)`; `fused=True` as well if wanted).
    * Constructing the object does not advance training: the warm-up steps capture needs (library handles, FFT plans,
      allocator pools, optimiser state) are undone -- parameters, buffers and optimiser state are put back in place; state the
      optimiser did not have yet is zeroed, which is what Adam-style optimisers start from.
    * A `FilteredNoise(rng='device')` inside the model draws from a device-resident Philox counter from here on (read by the
      forward and the backward kernel, advanced by a node of the graph): every replay gets fresh noise, the same sequence as
      the eager steps; `step()` also advances the modules' host-side offsets by the same amount, so eager calls of the model
      between graphed steps continue the stream.
    * fp32 or `amp_dtype=torch.bfloat16` without a scaler; every rank must hold rows.
    * `scaler=torch.amp.GradScaler("cuda")` (with `amp_dtype=torch.float16`: the reference's precision=16) puts the loss scaling
      inside the replay: the scaled backward, the non-finite check, the taken-or-skipped update and the scale's growth / back-off
      are all nodes of the graph, with no host read per step.  That needs an optimiser whose step takes the scale and the
      found-inf flag as device tensors (`torch.optim.Adam(..., fused=True, capturable=True)`); any other raises.  Single rank only.
    * `prologue`: a callable captured in front of the forward, e.g. the gather of the next batch into the static inputs
      (trainer.DeviceBatches).  It is NOT run during the warm-up, which steps on the example batch: run it once eagerly before.
      With `static_batch=True` the example batch's own tensors become the static inputs (the prologue writes them) instead of copies.
    * A learning rate that changes between replays must live in a device tensor (`Adam(lr=torch.tensor(1e-3, device=...))`): a
      Python float is a constant of the captured update.  `set_lr` writes that tensor.
    * The persistent GRU launches inside a graph are ordered by the graph only: do not run another recurrence on a second
      stream of the same device while a replay is in flight (DESIGN.md par. 9a).
    """

    def __init__(self, model, loss_fn, optimizer, example_batch, group=None, amp_dtype=None, warmup: int = 3,
                 scaler=None, prologue=None, static_batch: bool = False):
        import torch.distributed as dist
        self.model, self.loss_fn, self.opt, self.group, self.amp_dtype = model, loss_fn, optimizer, group, amp_dtype
        self.scaler = scaler if scaler is not None and scaler.is_enabled() else None
        self.prologue = prologue
        self.params = [p for p in model.parameters() if p.requires_grad]
        if not self.params or not self.params[0].is_cuda:
            raise _lib.DdspHipError("GraphedTrainStep needs the model on a GPU")
        if not all(g.get("capturable", True) for g in optimizer.param_groups):     # (optimisers without the option, e.g. SGD, never synchronise)
            raise ValueError("GraphedTrainStep needs a capturable optimiser, e.g. torch.optim.Adam(params, capturable=True)")
        dev = self.params[0].device
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if self.scaler is not None:
            if self.world > 1:
                raise ValueError("GraphedTrainStep: scaler= is single-rank only (the skip decision would have to follow the all-reduce)")
            if not getattr(optimizer, "_step_supports_amp_scaling", False):
                raise ValueError("GraphedTrainStep: scaler= needs an optimiser that takes the scale on the device, "
                                 "e.g. torch.optim.Adam(params, fused=True, capturable=True)")
        # (static_batch: the example's own CUDA tensors ARE the static inputs -- whoever fills them, e.g. the prologue, owns them)
        self.batch = dict(example_batch) if static_batch else \
            {k: (v.detach().to(dev).clone() if torch.is_tensor(v) else v) for k, v in example_batch.items()}
        if next((v.shape[0] for v in self.batch.values() if torch.is_tensor(v)), 0) == 0:
            raise ValueError("GraphedTrainStep cannot capture an empty shard")
        self.noises = [m for m in model.modules() if isinstance(m, FilteredNoise) and m.rng == "device"]
        # band-limited wavetable banks keep the mip levels of their tables for live(): a replayed update rewrites the tables
        # without touching the parameter's version, so every step tells them
        self.level_caches = [m for m in model.modules() if hasattr(m, 'invalidate_levels')]
        # (the modules see their counter only inside this object's steps; eager calls keep the host-side offset)
        self.counters = [torch.tensor([m._offset], dtype=torch.int64, device=dev) for m in self.noises]
        self._mirror = [int(m._offset) for m in self.noises]    # what each device counter holds (host-side knowledge)
        self.loss = None
        self.nbytes = sum(p.numel() * p.element_size() for p in self.params)
        self._capture(dev, warmup)

    # one step in two halves (a collective sits between them when there is more than one rank)
    def _forward_backward(self, prologue: bool = False):
        for m, c in zip(self.noises, self.counters):
            m.counter, m._last_draws = c, 0
        try:
            if prologue and self.prologue is not None:
                self.prologue()
            if self.amp_dtype is not None:
                dense.lowp_weights.refresh(self.amp_dtype)
            with torch.autocast("cuda", dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None):
                audio = self.model(self.batch)
            dense.lowp_weights.release()               # (the copies the captured forward uses are refreshed by the graph itself)
            loss = self.loss_fn(audio.float(), self.batch)
            (self.scaler.scale(loss) if self.scaler is not None else loss).backward()
            self._draws = [m._last_draws for m in self.noises]     # host constants of the captured shape
            for m, c in zip(self.noises, self.counters):
                if m._last_draws:                      # (0: the caller injected its own draw, the counter was not read)
                    c.add_(m._last_draws)
        finally:
            dense.lowp_weights.release()
            for m in self.noises:
                m.counter = None
        return loss.detach()

    def _update(self):
        if self.scaler is not None:
            self.scaler.step(self.opt)        # (a fused optimiser: unscale, found-inf and the skip happen inside its kernels)
            self.scaler.update()
        else:
            self.opt.step()

    def set_lr(self, value: float) -> None:
        """A new learning rate for the following replays: written into the device tensor(s) the captured update reads."""
        for g in self.opt.param_groups:
            if not torch.is_tensor(g["lr"]) or not g["lr"].is_cuda:
                raise ValueError("GraphedTrainStep.set_lr: the captured update holds this optimiser's Python-float learning rate as a "
                                 "constant; construct it with lr=torch.tensor(value, device=...)")
            g["lr"].fill_(float(value))

    def _reduce(self):
        import torch.distributed as dist
        grads = [p.grad for p in self.params]
        flat = torch.cat([g.reshape(-1) for g in grads])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
        flat /= self.world
        torch._foreach_copy_(grads, [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in grads]), grads)])

    def _capture(self, dev, warmup):
        model_state = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        had = {id(p): {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in self.opt.state.get(p, {}).items()}
               for g in self.opt.param_groups for p in g["params"]}
        counters = [c.clone() for c in self.counters]
        sc = self.scaler
        # (a scaler that has not scaled anything yet has no tensors: the warm-up creates them, from these initial values)
        sc_state = None if sc is None else ((float(sc._scale), int(sc._growth_tracker)) if sc._scale is not None
                                            else (sc._init_scale, sc._init_growth_tracker))

        def restore():
            with torch.no_grad():
                live = self.model.state_dict()
                for k, v in model_state.items():
                    live[k].copy_(v)
                for g in self.opt.param_groups:
                    for p in g["params"]:
                        for k, v in self.opt.state.get(p, {}).items():
                            if torch.is_tensor(v):
                                old = had[id(p)].get(k)
                                v.copy_(old) if old is not None else v.zero_()
                for live_c, c in zip(self.counters, counters):
                    live_c.copy_(c)
                if sc is not None:
                    sc._scale.fill_(sc_state[0])
                    sc._growth_tracker.fill_(sc_state[1])

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self.opt.zero_grad(set_to_none=True)
                self._forward_backward()
                if self.world > 1:
                    self._reduce()
                self._update()
        torch.cuda.current_stream(dev).wait_stream(side)
        restore()
        self.opt.zero_grad(set_to_none=True)          # the captured backward allocates the gradients inside the graph's pool
        self._graph = torch.cuda.CUDAGraph()
        self._graph_update = None
        with torch.cuda.graph(self._graph):
            self.loss = self._forward_backward(prologue=True)
            if self.world == 1:
                self._update()
        if self.world > 1:
            self._graph_update = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph_update, pool=self._graph.pool()):
                self.opt.step()
        restore()

    def step(self, batch=None):
        """One optimisation step on `batch` (same keys and shapes as the example; None = whatever the static inputs hold).
        Returns (loss tensor -- static, overwritten by the next step --, all-reduce bytes)."""
        if batch is not None:
            for k, v in batch.items():
                if torch.is_tensor(v):
                    self.batch[k].copy_(v, non_blocking=True)
        # eager calls of the same model between graphed steps (validation, an eager train_step) advance only the modules'
        # host-side offsets: bring the device counters up to them first, so that this replay does not redraw that noise
        for i, (m, c) in enumerate(zip(self.noises, self.counters)):
            if int(m._offset) != self._mirror[i]:
                c.fill_(int(m._offset))                 # an async fill from a host integer, outside the graph
                self._mirror[i] = int(m._offset)
        self._graph.replay()
        if self.world > 1:
            self._reduce()
            self._graph_update.replay()
        # ... and keep the host-side offsets in step with the device counters, so that an eager call after graphed steps
        # continues the stream instead of replaying its start
        for i, (m, d) in enumerate(zip(self.noises, self._draws)):
            self._mirror[i] += d
            m._offset = self._mirror[i]
        for m in self.level_caches:
            m.invalidate_levels()
        return self.loss, self.nbytes

    __call__ = step
