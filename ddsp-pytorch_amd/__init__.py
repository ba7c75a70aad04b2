"""MI355X-native DDSP synthesis hot path (harmonic oscillator bank + filtered noise).

Drop-in for `model/ddsp/harmonic_oscillator.py` and `model/ddsp/filtered_noise.py`
of kureta/ddsp-pytorch: same constructors, `forward()` / `live()` signatures,
control-dict keys and state-dict keys, with the compute in hand-written HIP
kernels (gfx950) behind the C ABI declared in `include/ddsp_hip.h`.
"""
from . import synthetic  # noqa: F401
from . import _lib  # noqa: F401
from . import sharding  # noqa: F401
from . import training  # noqa: F401
from .harmonic_oscillator import OscillatorBank, osc_forward, osc_backward  # noqa: F401
from . import wavetable  # noqa: F401
from .wavetable import WavetableBank, wavetable_forward, wavetable_backward, wavetable_form  # noqa: F401
from .wavetable import (dirichlet_kernels, wavetable_mipmaps, wavetable_forward_bl, wavetable_backward_bl,  # noqa: F401
                        wavetable_form_bl)
from . import sinusoids  # noqa: F401
from .sinusoids import InharmonicBank, sinusoids_forward, sinusoids_backward, stretched_ratios  # noqa: F401
from .filtered_noise import FilteredNoise, noise_forward, noise_backward, noise_ola_stream, ola_stream_state, calibrate_noise_residency  # noqa: F401
from .reverb import Reverb, causal_fft_convolve  # noqa: F401
from .graphed import GraphedSynth, GraphedLiveDecoder, GraphedTrainStep  # noqa: F401
from .gru import GRU, gru_forward, gru_backward, gru_status  # noqa: F401
from .decoder import Controller, Decoder  # noqa: F401
from .encoder import Crepe, F0Encoder, LoudnessEncoder, Encoder  # noqa: F401
from .encoder import mfcc, MFCC, ZEncoder  # noqa: F401
from .encoder import pitch_argmax, pitch_centered, pitch_weighted, pitch_viterbi, pitch_voicing, pitch_salience_yin  # noqa: F401
from . import conditioning  # noqa: F401
from .conditioning import ConditioningStatistics, conditioning_statistics, fit_conditioning  # noqa: F401
from . import tuning  # noqa: F401
from .tuning import TuningStatistics, tuning_statistics, tune_pitch  # noqa: F401
from . import notes  # noqa: F401
from .notes import Expression, Notes, extract_notes, note_expression, render_notes  # noqa: F401
from . import voices  # noqa: F401
from .voices import allocate_voices, mix_voices  # noqa: F401
from . import analysis  # noqa: F401
from .analysis import HarmonicAnalyzer, harmonic_analysis, harmonic_resynthesis, harmonic_residual, refine_f0  # noqa: F401
from .analysis import NoiseAnalyzer, noise_analysis  # noqa: F401
from .analysis import ControlTransform, transform_controls  # noqa: F401
from .analysis import ControlMorph, morph_controls  # noqa: F401
from .analysis import ControlAlign, align_controls, control_features, dtw_align  # noqa: F401
from . import partials  # noqa: F401
from .partials import (PartialAnalyzer, partial_analysis, partial_resynthesis, partial_residual, refine_partials,  # noqa: F401
                       fit_inharmonicity, inharmonic_analysis)
from .autoencoder import AutoEncoder  # noqa: F401
from .dataset import AudioData, PLHDataset, load_audio, example_geometry  # noqa: F401
from .spectral import griffinlim  # noqa: F401
from . import style  # noqa: F401
from .style import (normalize_audio, prepare_spectra, gram_matrix, FeatureExtractor, ContentLoss, StyleLoss,  # noqa: F401
                    style_transfer)
from . import trainer  # noqa: F401
from .trainer import DeviceBatches, PlateauRate, Trainer, gather_batch, load_checkpoint, latest_checkpoint  # noqa: F401
from .training import MSSLoss, train_step, allreduce_gradients, OverlappedGradientReducer  # noqa: F401

__all__ = ["OscillatorBank", "FilteredNoise", "Reverb", "causal_fft_convolve", "GraphedSynth", "GraphedLiveDecoder", "GraphedTrainStep", "Controller", "Decoder", "Crepe", "F0Encoder", "LoudnessEncoder", "Encoder", "pitch_voicing", "pitch_salience_yin", "conditioning", "ConditioningStatistics", "conditioning_statistics", "fit_conditioning", "tuning", "TuningStatistics", "tuning_statistics", "tune_pitch", "notes", "Notes", "extract_notes", "render_notes", "Expression", "note_expression", "AutoEncoder", "AudioData", "PLHDataset", "load_audio", "example_geometry", "GRU", "MSSLoss", "train_step", "allreduce_gradients", "OverlappedGradientReducer", "osc_forward", "osc_backward", "noise_forward", "noise_backward", "calibrate_noise_residency", "griffinlim",
           "normalize_audio", "prepare_spectra", "gram_matrix", "FeatureExtractor", "ContentLoss", "StyleLoss", "style_transfer",
           "analysis", "HarmonicAnalyzer", "harmonic_analysis", "harmonic_resynthesis", "harmonic_residual", "refine_f0", "NoiseAnalyzer", "noise_analysis",
           "ControlTransform", "transform_controls", "ControlMorph", "morph_controls", "ControlAlign", "align_controls", "control_features", "dtw_align",
           "synthetic", "trainer", "DeviceBatches", "PlateauRate", "Trainer", "gather_batch", "load_checkpoint",
           "latest_checkpoint", "mfcc", "MFCC", "ZEncoder", "voices", "allocate_voices", "mix_voices",
           "wavetable", "WavetableBank", "wavetable_forward", "wavetable_backward", "wavetable_form",
           "dirichlet_kernels", "wavetable_mipmaps", "wavetable_forward_bl", "wavetable_backward_bl", "wavetable_form_bl",
           "sinusoids", "InharmonicBank", "sinusoids_forward", "sinusoids_backward", "stretched_ratios",
           "partials", "PartialAnalyzer", "partial_analysis", "partial_resynthesis", "partial_residual", "refine_partials",
           "fit_inharmonicity", "inharmonic_analysis"]
