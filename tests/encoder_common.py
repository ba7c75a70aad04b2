"""Shared by the encoder tests: the fixture configurations of tools/make_encoder_goldens.py and module builders with the
seeded CREPE weights (tests/crepe_seeded.py)."""
import numpy as np
import torch

import ddsp_pytorch_amd as ddsp
from crepe_seeded import seeded_crepe_state, crepe_shapes


class Conf:
    def __init__(self, sample_rate, n_fft, hop_length, crepe_capacity="tiny"):
        self.sample_rate, self.n_fft, self.hop_length, self.crepe_capacity = sample_rate, n_fft, hop_length, crepe_capacity


class AEConf:
    n_harmonics, n_noise_filters, sample_rate, hop_length, n_fft = 16, 9, 44100, 512, 2048
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1
    crepe_capacity = "tiny"


def crepe_weights(capacity, seed):
    return seeded_crepe_state(crepe_shapes(ddsp.Crepe(capacity)), int(seed))


def f0_encoder(g, conf):
    return ddsp.F0Encoder(conf, weights=crepe_weights(conf.crepe_capacity, g["crepe_seed"]))


def autoencoder(g):
    ae = ddsp.AutoEncoder(AEConf, weights=crepe_weights("tiny", g["crepe_seed"]))
    ae.decoder.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("dw__")}, strict=True)
    return ae.eval()


def loud_conf(g, tag):
    sr, n_fft, hop = (int(v) for v in g[f"{tag}_conf"])
    return Conf(sr, n_fft, hop)
