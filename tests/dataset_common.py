"""Shared by the training-set tests: the fixtures of tools/make_dataset_goldens.py (G26) written back out as WAV folders, their
configurations and seeded CREPE weights."""
import os

import numpy as np
from scipy.io import wavfile

from conftest import load_golden
from encoder_common import crepe_weights

FIXTURES = ("g26_dataset_mix", "g26_dataset_default")
KEYS = ("f0", "harmonicity", "loudness", "probabilities", "normalized_cents", "audio")


class DataConf:
    def __init__(self, data_dir, sample_rate, n_fft, hop_length, batch_size, example_duration, example_overlap,
                 crepe_capacity="tiny", crepe_weights=None):
        self.data_dir, self.sample_rate, self.n_fft, self.hop_length = data_dir, sample_rate, n_fft, hop_length
        self.batch_size, self.example_duration, self.example_overlap = batch_size, example_duration, example_overlap
        self.crepe_capacity, self.crepe_weights = crepe_capacity, crepe_weights


def files_of(g):
    """[(relative path, rate, pcm)] in the fixture's order."""
    return [(str(g[f"file{i}_path"]), int(g[f"file{i}_rate"]), g[f"file{i}_pcm"]) for i in range(int(g["n_files"]))]


def write_folder(g, root):
    for rel, sr, pcm in files_of(g):
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        wavfile.write(os.path.join(root, rel), sr, pcm)
    return str(root)


def fixture_conf(g, data_dir):
    sr, n_fft, hop, batch = (int(v) for v in g["conf"])
    duration, overlap = (float(v) for v in g["durations"])
    return DataConf(str(data_dir), sr, n_fft, hop, batch, int(duration) if duration.is_integer() else duration, overlap,
                    crepe_weights=crepe_weights("tiny", g["crepe_seed"]))


def fixture(name, tmp_path):
    """-> (fixture arrays, conf with data_dir = a fresh folder holding the fixture's WAVs)."""
    g = load_golden(name)
    d = tmp_path / name
    d.mkdir()
    return g, fixture_conf(g, write_folder(g, d))


def example_sources(g, conf):
    """Per example: the rate of the file it came from (the files sorted, as the datasets find them; decoys skipped)."""
    from ddsp_pytorch_amd import dataset
    import ddsp_pytorch_amd.encoder as enc
    rates = []
    for rel, sr, pcm in sorted(files_of(g)):
        if rel.count("/") != 1:
            continue
        n = enc.resampled_length(pcm.shape[0], sr, conf.sample_rate)
        rates += [sr] * dataset.count_examples(rel, n, conf)
    return np.array(rates)
