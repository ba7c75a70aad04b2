"""`AutoEncoder` (model/autoencoder/autoencoder.py): the encoder of `encoder.py` in front of this package's `Decoder`.

  forward(x)                 audio [B, L] -> audio: pads (p // 2, p - p // 2) with p = n_fft - hop so that the loudness frames
                             and the CREPE frames line up with the decoder's hop grid (autoencoder.py:17-22)
  analyse(x, noise=False, refine=0)
                             the control dict of x without the decoder's network: f0, a, c by harmonic analysis and, with noise=True
                             (the truncated noise model) or noise='overlap_add', H by noise analysis of the residual (analysis.py);
                             refine=N first moves the decoded f0 off its 20-cent grid by N steps of analysis.refine_f0
  transform(x, stretch=1.0, transpose=0.0, formant=0.0, positions=None, noise=True, refine=0, reverb=False)
                             analyse, analysis.transform_controls (time stretch, transposition, formant shift), synthesize:
                             audio [B, T' hop]
  morph(x, y, mix=0.5, mix_f0=None, mix_harmonics=None, mix_noise=None, coordinates='hz', frames=None, positions_a=None,
        positions_b=None, noise=True, refine=0, reverb=False, align=False, timing=0.0, radius=None, penalty=0.0)
                             analyse both clips, analysis.morph_controls (pitch, envelope and noise between the two), synthesize:
                             audio [B, T' hop]; align=True first finds which frame of x goes with which frame of y
                             (analysis.align_controls: dynamic time warping) instead of stretching both linearly
  transfer(x, target, **fit_options)
                             forward with conditioning.fit_conditioning between encoder and decoder: the clip's register moved by
                             whole octaves towards, and its loudness quantile-mapped onto, `target` (the ConditioningStatistics of
                             the decoder's training set)
  transcribe(x, **extract_options)
                             the encoder followed by notes.extract_notes: the clip's note events (notes.Notes)
  play(notes, frames=None, target=None, voices=None, **render_options)
                             notes.render_notes, fit_conditioning where a target is given, the decoder: a score -> audio;
                             voices=V plays chords: voices.allocate_voices in front, the B V rows as one batch, voices.mix_voices
                             behind
  forward_live(x, hidden, delayed=False, conditioning=None)
                             the real-time callback of rt/synth.py:40-55: a numpy window (4096 samples by default) -> one H2D
                             copy, hop // 2 samples dropped at the front and hop - hop // 2 at the back (autoencoder.py:26-32),
                             encoder, then Decoder.forward_live -> (audio as numpy, hidden); conditioning=(target, source) maps
                             the block (one launch) between the two

With a decoder that has a timbre latent (conf.z_dims > 0) `forward`, `transfer` and `play` take
`timbre=`: another clip [B, L'] (its z averaged over time and held for every frame), a latent [B, z_dims] (held) or
[B, T, z_dims] (per frame).  Without it forward and transfer take the timbre from x itself, frame by frame; play has no audio
and requires it.  `encode_timbre(y)` is the time average on its own, and forward_live's `hidden` is the pair
(decoder_hidden, z_hidden).

State-dict keys are the reference's (`encoder.f0_encoder.model.*`, `encoder.loudness_encoder.a_weight`, `decoder.*`).  CREPE
weights come from `weights` or `conf.crepe_weights` (see encoder.F0Encoder); `voicing` and `tracker` are handed to `Encoder`.
With tracker 'yin' (the argument, else `conf.pitch_tracker`) no weights are needed and the state dict has no
`encoder.f0_encoder.model.*` keys; decoder checkpoints load as before.  The decoder's synthesis runs on the device only.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .conditioning import fit_conditioning
from .tuning import tune_pitch
from .notes import Expression, extract_notes, note_expression, render_notes
from .voices import allocate_voices, mix_voices
from .analysis import (align_controls, harmonic_analysis, harmonic_residual, morph_controls, noise_analysis, refine_f0,
                       transform_controls)
from .decoder import Decoder
from .encoder import Encoder
from .partials import inharmonic_analysis, partial_residual
from .sinusoids import is_inharmonic, refuse_inharmonic
from .wavetable import refuse_wavetable


class AutoEncoder(nn.Module):
    def __init__(self, conf, noise_rng: str = 'host', seed: int = 0, weights=None, voicing=None, tracker=None, noise_overlap_add=None,
                 synth=None, band_limited=None):
        super().__init__()
        self.encoder = Encoder(conf, weights, voicing=voicing, tracker=tracker)
        self.decoder = Decoder(conf, noise_rng=noise_rng, seed=seed, noise_overlap_add=noise_overlap_add, synth=synth,
                               band_limited=band_limited)
        self.padding = conf.n_fft - conf.hop_length
        self.hop_length = conf.hop_length
        self.n_noise_filters = conf.n_noise_filters

    def encode_timbre(self, y: torch.Tensor) -> torch.Tensor:
        """clip [B, L'] -> [B, z_dims]: the decoder's z_encoder on the clip, averaged over its frames."""
        self._need_latent("encode_timbre")
        return self.decoder.z_encoder(y).mean(dim=1)

    def _need_latent(self, what: str) -> None:
        if self.decoder.z_dims <= 0:
            raise ValueError(f"{what}: this decoder has no timbre latent (it was built without conf.z_dims)")

    def _timbre(self, timbre, frames: int, what: str) -> torch.Tensor:
        """`timbre` (a clip [B, L'], a latent [B, z_dims] or [B, T, z_dims]) -> z [B, frames, z_dims]"""
        self._need_latent(f"{what}(timbre=...)")
        d = self.decoder.z_dims
        if timbre.dim() == 2 and timbre.shape[-1] != d:
            timbre = self.encode_timbre(timbre)
        if timbre.dim() == 2:
            return timbre.unsqueeze(1).expand(-1, frames, -1).contiguous()
        if timbre.dim() != 3 or timbre.shape[1] != frames or timbre.shape[2] != d:
            raise ValueError(f"{what}: timbre must be a clip [B, L], a latent [B, {d}] or [B, {frames}, {d}], got {tuple(timbre.shape)}")
        return timbre

    def _with_timbre(self, z: dict, x, timbre, what: str) -> dict:
        """The encoder's dict with what a decoder with a latent reads besides: `z` from `timbre`, else the clip itself as `audio`."""
        if timbre is not None:
            z['z'] = self._timbre(timbre, z['f0'].shape[1], what)
        elif self.decoder.z_dims > 0:
            if x is None:
                raise ValueError(f"{what}: a decoder with a timbre latent needs timbre= here (there is no audio to take it from)")
            z['audio'] = x
        return z

    def forward(self, x: torch.Tensor, timbre=None) -> torch.Tensor:
        z = self.encoder(F.pad(x, (self.padding // 2, self.padding - self.padding // 2)))
        return self.decoder(self._with_timbre(z, x, timbre, "forward"))

    def transfer(self, x: torch.Tensor, target, **fit_options) -> torch.Tensor:
        """audio [B, L] -> audio: `forward` with the encoder's controls brought into `target`'s range on the way
        (conditioning.fit_conditioning and its options: source, octaves, max_octaves, strength, min_frames).  Without a
        `source` every clip is measured by itself, over its whole length.  One more keyword is taken out of the options:
        tune=True, or a dict of tuning.tune_pitch's options, moves the fitted controls' notes onto a scale before the decoder
        (the chain's last step: octave shift, loudness match, auto-tune); tune=None is the path without it.  `timbre=` (taken
        out of the options as well) is forward's, for a decoder with a timbre latent."""
        tune = fit_options.pop('tune', None)
        timbre = fit_options.pop('timbre', None)
        if fit_options.get('return_info'):
            raise ValueError("transfer returns audio; ask fit_conditioning itself for the info")
        if tune is not None and tune is not True and tune is not False and not isinstance(tune, dict):
            raise ValueError(f"transfer: tune must be None, a bool or a dict of tune_pitch options, got {type(tune).__name__}")
        if isinstance(tune, dict) and tune.get('return_info'):
            raise ValueError("transfer returns audio; ask tune_pitch itself for the info")
        z = fit_conditioning(self.encoder(F.pad(x, (self.padding // 2, self.padding - self.padding // 2))), target, **fit_options)
        if tune:
            z = tune_pitch(z, **(tune if isinstance(tune, dict) else {}))
        return self.decoder(self._with_timbre(dict(z), x, timbre, "transfer"))

    def transcribe(self, x: torch.Tensor, expression: bool = False, **extract_options):
        """audio [B, L] -> notes.Notes: the encoder (on the clip padded as forward() pads it) followed by notes.extract_notes
        and its options (tuning, scale, root, hysteresis, min_note_frames, max_notes).  expression=True -> (notes, expression):
        notes.note_expression of the same controls, the pitch and loudness curve of every note, for play(notes, expression=...)."""
        with torch.no_grad():
            z = self.encoder(F.pad(x, (self.padding // 2, self.padding - self.padding // 2)))
        found = extract_notes(z, **extract_options)
        return (found, note_expression(z, found)) if expression else found

    def play(self, notes, frames=None, target=None, timbre=None, voices=None, voice_options=None, mix_options=None,
             **render_options) -> torch.Tensor:
        """notes.Notes -> audio [B, frames hop]: notes.render_notes (and its options, `expression`, `source`, `bend_amount`,
        `dynamics_amount`, `keep_attack` and `keep_release` among them) at the decoder's sample rate and hop, then
        `fit_conditioning(z, target)` where a ConditioningStatistics `target` is given (the decoder's training set: the score's
        register and levels brought into its range), then the decoder's ordinary forward.  frames=None takes the end of the last
        note (that reads the notes back from the device).  `timbre` (a clip or a latent, see the module docstring) is required
        when the decoder has a timbre latent: a score has no audio to take it from.

        voices=V plays a score whose notes overlap: voices.allocate_voices (with `voice_options`) gives
        each of V monophonic voices its notes, the B V rows go through the steps above as one batch -- `expression` and `timbre`
        repeated per voice, every voice note finding its curve through the allocation's `index` -- and voices.mix_voices (with
        `mix_options`: gain, pan, hold, fade; gate=True passes the render's `voiced` as the gate) sums them: [B, frames hop], or
        [B, 2, frames hop] with a pan.  voices=None is the monophonic call as it always was."""
        if render_options.get('return_info'):
            raise ValueError("play returns audio; ask render_notes itself for the info")
        if voices is None and (voice_options is not None or mix_options is not None):
            raise ValueError("play: voice_options and mix_options belong to voices=V")
        if frames is None:
            used = notes._used()
            ends = torch.where(used, notes.onset.to(torch.int64) + notes.frames, torch.zeros_like(notes.onset, dtype=torch.int64))
            frames = max(int(ends.max()) if ends.numel() else 0, 1)
        if voices is not None:
            return self._play_voices(notes, frames, target, timbre, voices, dict(voice_options or {}), dict(mix_options or {}),
                                     render_options)
        z = render_notes(notes, frames, self.decoder.harmonics.sample_rate, self.hop_length, **render_options)
        if target is not None:
            z = fit_conditioning(z, target)
        return self.decoder(self._with_timbre(dict(z), None, timbre, "play"))

    def _play_voices(self, notes, frames, target, timbre, voices, voice_options, mix_options, render_options):
        """play(voices=V): allocate, render and decode the B V voice rows as one batch, mix"""
        if voice_options.pop('return_info', False) or 'out' in mix_options:
            raise ValueError("play returns audio; ask allocate_voices and mix_voices themselves for their info and `out`")
        rows, info = allocate_voices(notes, voices, return_info=True, **voice_options)
        V = rows.rows // notes.rows
        render_options = dict(render_options)
        e = render_options.get('expression')
        if isinstance(e, Expression):
            if e.rows != notes.rows:
                raise ValueError(f"play: the expression has {e.rows} rows, the notes {notes.rows}")
            per_voice = lambda x: None if x is None else x.repeat_interleave(V, dim=0)     # noqa: E731
            render_options['expression'] = Expression(**{k: per_voice(x) for k, x in e._tensors().items()})
            index, given = info['index'], render_options.get('source')
            if given is not None:                                               # the caller's map first: voice note -> note -> curve
                given = per_voice(torch.as_tensor(given, dtype=torch.int32, device=notes.device).reshape(notes.rows, notes.max_notes))
                index = torch.where(index >= 0, torch.gather(given, 1, index.clamp(min=0).long()), index)
            render_options['source'] = index
        z = render_notes(rows, frames, self.decoder.harmonics.sample_rate, self.hop_length, **render_options)
        active = z['voiced'] if mix_options.pop('gate', False) else None
        if target is not None:
            z = fit_conditioning(z, target)
        if timbre is not None:
            timbre = self._timbre(timbre, frames, "play").repeat_interleave(V, dim=0)
        audio = self.decoder(self._with_timbre(dict(z), None, timbre, "play"))
        return mix_voices(audio.detach(), V, active=active, hop_length=self.hop_length if active is not None else None,     # (no backward)
                          **mix_options)

    def analyse(self, x: torch.Tensor, return_complex: bool = False, noise=False, average: int = 1, iterations=None,
                refine: int = 0) -> dict:
        """audio [B, L] -> the oscillator bank's control dict without the decoder's network: the encoder's pitch track (and its
        voicing, where that is on) of the clip padded as forward() pads it, then analysis.harmonic_analysis of the clip cropped to
        its T = L // hop whole frames.  `self.decoder.harmonics(self.analyse(x))` is the harmonic resynthesis of x.

        noise=True adds 'H' [B, T, n_noise_filters]: analysis.noise_analysis (with `average` and `iterations`) of the residual
        analysis.harmonic_residual leaves, so that `self.decoder.synthesize(self.analyse(x, noise=True))` is the parametric
        harmonic-plus-noise resynthesis of x.  noise=True and noise='truncated' invert the truncated noise model (16 iterations
        unless told otherwise), noise='overlap_add' the overlap-add one (8); each is refused on a decoder built with the other
        form, whose synthesis would play its H at the wrong level.

        refine=N runs N steps of analysis.refine_f0 on the encoder's track before the analysis (a decoded track is a bin centre,
        up to 10 cents off); the dict's f0 is then the refined track.  refine=0 is the analysis along the encoder's own track."""
        refuse_wavetable(self.decoder, "analyse")
        refuse_inharmonic(self.decoder, "analyse")
        overlap_add = self._noise_form(noise, "analyse")
        bank = self.decoder.harmonics
        with torch.no_grad():
            z = self.encoder(F.pad(x, (self.padding // 2, self.padding - self.padding // 2)))
        f0 = z['f0']
        frames = f0.shape[1]
        if frames * self.hop_length > x.shape[-1]:
            raise ValueError(f"the encoder returned {frames} frames of hop {self.hop_length} for {x.shape[-1]} samples")
        args = (x[:, :frames * self.hop_length], f0, self.hop_length, bank.sample_rate, bank.n_harmonics, self.padding + self.hop_length)
        if not noise:
            return harmonic_analysis(*args, voiced=z.get('voiced'), return_complex=return_complex, refine=refine)
        _, resid, ctrl = harmonic_residual(*args, voiced=z.get('voiced'), return_complex=return_complex, refine=refine)
        ctrl['H'] = noise_analysis(resid, self.hop_length, self.n_noise_filters, average=average,
                                   iterations=iterations, overlap_add=overlap_add)
        return ctrl

    def _noise_form(self, noise, what: str) -> bool:
        """The `noise` argument of the analysis entry points against the decoder's noise form -> whether it is the overlap-add one."""
        if noise not in (False, True, 'truncated', 'overlap_add'):
            raise ValueError(f"{what}: noise must be False, True, 'truncated' or 'overlap_add', got {noise!r}")
        overlap_add = noise == 'overlap_add'
        if noise and not overlap_add and self.decoder.noise.overlap_add:
            # the truncated model's H played through the overlap-add would come out too strong
            raise ValueError(f"{what}(noise=True) inverts the truncated noise model; it does not apply to a decoder with noise_overlap_add: "
                             "ask for noise='overlap_add'")
        if overlap_add and not self.decoder.noise.overlap_add:
            raise ValueError(f"{what}(noise='overlap_add') inverts the overlap-add noise model; on a decoder without noise_overlap_add its H "
                             "would come out too weak: ask for noise=True")
        return overlap_add

    def analyse_partials(self, x: torch.Tensor, iterations: int = 4, model: str = 'stiff', noise=False, refine: int = 0,
                         return_complex: bool = False, average: int = 1, noise_iterations=None, max_cents: float = 50.0) -> dict:
        """audio [B, L] -> the inharmonic bank's control dict without the decoder's network (a `synth='inharmonic'` decoder only):
        the encoder's pitch track (and its voicing, where that is on) as `analyse` takes it, after `refine` steps of
        analysis.refine_f0, then partials.inharmonic_analysis with the bank's partial count, base ratios and current
        inharmonicity as the start: dict(f0, ratios, a, c, inharmonicity[, C]).  `self.decoder.harmonics(d)` is the resynthesis
        of x's partials, and `self.decoder.harmonics.init_from(d)` starts the bank's trainable parameters there.

        noise follows `analyse`'s rules and adds 'H' [B, T, n_noise_filters]: analysis.noise_analysis (with `average` and
        `noise_iterations`) of the residual partials.partial_residual leaves along the dict's tracks, so that
        `self.decoder.synthesize(self.analyse_partials(x, noise=True))` is the partials-plus-noise resynthesis of x."""
        if not is_inharmonic(self.decoder):
            raise ValueError("analyse_partials: needs the inharmonic synthesiser (build the model with synth='inharmonic'); a harmonic "
                             "decoder is analysed by analyse()")
        overlap_add = self._noise_form(noise, "analyse_partials")
        bank = self.decoder.harmonics
        with torch.no_grad():
            z = self.encoder(F.pad(x, (self.padding // 2, self.padding - self.padding // 2)))
        f0, voiced = z['f0'], z.get('voiced')
        frames = f0.shape[1]
        if frames * self.hop_length > x.shape[-1]:
            raise ValueError(f"the encoder returned {frames} frames of hop {self.hop_length} for {x.shape[-1]} samples")
        clip, window, K = x[:, :frames * self.hop_length], self.padding + self.hop_length, bank.n_partials
        if refine:
            f0 = refine_f0(clip, f0, self.hop_length, bank.sample_rate, K, window, voiced=voiced, iterations=refine, max_cents=max_cents)
        ctrl = inharmonic_analysis(clip, f0, self.hop_length, bank.sample_rate, K, window, voiced=voiced,
                                   inharmonicity=bank.inharmonicity.detach().clamp(min=0), base_ratios=bank.base_ratios,
                                   iterations=iterations, max_cents=max_cents, model=model, return_complex=return_complex)
        if noise:
            f = ctrl['f0'].float() * ctrl['ratios'].float()
            _, resid, _ = partial_residual(clip, f, self.hop_length, bank.sample_rate, window, voiced=voiced)
            ctrl['H'] = noise_analysis(resid, self.hop_length, self.n_noise_filters, average=average, iterations=noise_iterations,
                                       overlap_add=overlap_add)
        return ctrl

    def transform(self, x: torch.Tensor, stretch=1.0, transpose=0.0, formant=0.0, positions=None, noise=True, refine: int = 0,
                  reverb: bool = False) -> torch.Tensor:
        """audio [B, L] -> audio [B, T' hop], stretched in time, transposed and formant-shifted (semitones) without the decoder's
        network: `analyse(x, noise=noise, refine=refine)`, analysis.transform_controls on that dict (its `stretch`, `transpose`,
        `formant` -- 0 keeps the formants in place, None lets them follow the pitch -- and `positions`), then
        `decoder.synthesize`, and `decoder.reverb` only when asked.  noise follows analyse's rules (True / 'truncated' /
        'overlap_add' must be the decoder's noise form); noise=False plays the harmonics alone (`decoder.harmonics`)."""
        refuse_wavetable(self.decoder, "transform")
        refuse_inharmonic(self.decoder, "transform")
        ctrl = transform_controls(self.analyse(x, noise=noise, refine=refine), self.decoder.harmonics.sample_rate, stretch=stretch,
                                  transpose=transpose, formant=formant, positions=positions)
        with torch.no_grad():
            y = self.decoder.synthesize(ctrl) if noise else self.decoder.harmonics(ctrl)
            return self.decoder.reverb(y) if reverb else y

    def morph(self, x: torch.Tensor, y: torch.Tensor, mix=0.5, mix_f0=None, mix_harmonics=None, mix_noise=None, coordinates='hz',
              frames=None, positions_a=None, positions_b=None, noise=True, refine: int = 0, reverb: bool = False, align: bool = False,
              timing=0.0, radius=None, penalty=0.0) -> torch.Tensor:
        """audio x [B, L_x] and y [B, L_y] (the lengths may differ) -> audio [B, T' hop] between the two, without the decoder's
        network: `analyse` of both (noise and refine as in `transform`), analysis.morph_controls on the two dicts (`mix`, 0 is x and
        1 is y, a float or per output frame; `mix_f0`, `mix_harmonics`, `mix_noise`, `coordinates`, `frames` -- None: x's frames --,
        `positions_a`, `positions_b`), then `decoder.synthesize`, and `decoder.reverb` only when asked.  noise=False plays the
        harmonics alone (`decoder.harmonics`).  align=True finds the two positions by analysis.align_controls (dynamic time warping
        of the two analysed dicts; `timing`, 0 is x's clock and 1 is y's, `radius`, `penalty`; `frames` is then the timeline's T')
        instead of stretching both clips linearly; positions_a / positions_b must then be left out."""
        refuse_wavetable(self.decoder, "morph")
        refuse_inharmonic(self.decoder, "morph")
        if align and (positions_a is not None or positions_b is not None):
            raise ValueError("morph: align=True finds positions_a and positions_b; give one or the other")
        ctrl_x, ctrl_y = self.analyse(x, noise=noise, refine=refine), self.analyse(y, noise=noise, refine=refine)
        if align:
            positions_a, positions_b = align_controls(ctrl_x, ctrl_y, self.decoder.harmonics.sample_rate, radius=radius, penalty=penalty,
                                                      timing=timing, frames=frames)
            frames = None
        ctrl = morph_controls(ctrl_x, ctrl_y, self.decoder.harmonics.sample_rate, mix=mix, mix_f0=mix_f0, mix_harmonics=mix_harmonics, mix_noise=mix_noise,
                              coordinates=coordinates, frames=frames, positions_a=positions_a, positions_b=positions_b)
        with torch.no_grad():
            out = self.decoder.synthesize(ctrl) if noise else self.decoder.harmonics(ctrl)
            return self.decoder.reverb(out) if reverb else out

    def live_window(self, x: np.ndarray) -> torch.Tensor:
        """The callback's window on the module's device, trimmed as autoencoder.py:28-30 trims it: [1, len - hop]."""
        device = self.encoder.loudness_encoder.a_weight.device
        audio_in = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).unsqueeze(0).to(device, non_blocking=False)
        return audio_in[:, self.hop_length // 2:-(self.hop_length - self.hop_length // 2)]

    def forward_live(self, x: np.ndarray, hidden, delayed: bool = False, conditioning=None):
        """On a decoder with a timbre latent `hidden` is the pair (decoder_hidden, z_hidden), taken and returned.
        `delayed`: Decoder.forward_live's (the overlap-add noise as a stream, the audio n_noise_filters - 2 samples late).
        `conditioning`: None, or (target, source) ConditioningStatistics on the module's device -- the block's controls go
        through fit_conditioning(z, target, source=source), one launch, before the decoder (calibrate `source` once on a few
        seconds of the player; a source of None would measure each short block by itself)."""
        self.decoder.check_live(delayed, "forward_live")
        window = self.live_window(x)
        z = self.encoder(window)
        if conditioning is not None:
            target, source = conditioning
            z = fit_conditioning(z, target, source=source)
        if self.decoder.z_dims > 0:
            z = dict(z)
            z['audio'] = window           # the block's frames are the window's own: Decoder.forward_live encodes it with z_hidden
        return self.decoder.forward_live(z, hidden, delayed=delayed)
