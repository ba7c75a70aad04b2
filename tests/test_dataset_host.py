"""CPU checks of the training set (dataset.py): the reference's example arithmetic, the stock-torch AudioData / PLHDataset
against the reference's own dataset/audio_dataset.py bit for bit (fixtures G26, tools/make_dataset_goldens.py), the cache files
both ways, the refusals, and the new C entry points' argument validation."""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import dataset
from dataset_common import FIXTURES, KEYS, DataConf, fixture, fixture_conf, write_folder
from conftest import load_golden


@pytest.fixture(autouse=True)
def _native_conv():
    # the fixtures were captured with CPU convolutions on the native im2col + BLAS path (oneDNN's kernels depend on the ISA)
    with torch.backends.mkldnn.flags(enabled=False):
        yield


def reference_geometry(conf):
    """audio_dataset.py:50-57, verbatim."""
    duration = int(conf.example_duration * conf.sample_rate)
    diff = duration % conf.hop_length
    duration -= diff
    overlap = int(conf.example_overlap * conf.sample_rate)
    diff = duration % conf.hop_length
    overlap -= diff
    return duration, overlap


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 48000])
@pytest.mark.parametrize("hop", [64, 100, 256, 441, 512])
@pytest.mark.parametrize("dur,ovl", [(2, 0.5), (0.25, 0.1), (1.3, 1.7), (3, 0.05)])
def test_example_geometry_matches_reference_arithmetic(sr, hop, dur, ovl):
    conf = DataConf(None, sr, 2048, hop, 4, dur, ovl)
    duration, step = ddsp.example_geometry(conf)
    assert (duration, step) == reference_geometry(conf)
    assert duration % hop == 0
    # unfold's row count over any hop-padded length
    for n in (duration, duration + 1, duration + step - 1, duration + step, 5 * duration + 17):
        padded = n + sum(dataset.hop_pad(n, hop))
        if padded < duration:
            continue
        assert dataset.count_examples("x", n, conf) == torch.zeros(padded).unfold(0, duration, step).shape[0]


def test_default_config_geometry_and_hop_pad():
    conf = DataConf(None, 44100, 2048, 512, 16, 2, 0.5)
    assert ddsp.example_geometry(conf) == (88064, 22050)          # the step is not hop-aligned
    assert dataset.hop_pad(1024, 512) == (0, 0) and dataset.hop_pad(1027, 512) == (1, 2) and dataset.hop_pad(1030, 512) == (3, 3)
    with pytest.raises(ValueError):
        ddsp.example_geometry(DataConf(None, 44100, 2048, 512, 16, 0.001, 0.5))


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_datasets_match_reference_bit_for_bit(name, tmp_path):
    g, conf = fixture(name, tmp_path)
    plh = ddsp.PLHDataset(conf, device="cpu")
    assert list(plh.final) == [str(k) for k in g["out_keys"]] == list(KEYS)
    for k in KEYS:
        assert plh.final[k].dtype == torch.float32 and not plh.final[k].is_cuda
        assert np.array_equal(plh.final[k].numpy(), g[f"out_{k}"], equal_nan=True), k
    # both caches on disk, as the reference writes them
    audios = torch.load(conf.data_dir + "/audio_dataset.pth", weights_only=True)
    assert np.array_equal(audios.numpy(), g["out_audio"])
    cached = torch.load(conf.data_dir + "/plh_dataset.pth", weights_only=True)
    assert list(cached) == list(KEYS) and all(torch.equal(cached[k], plh.final[k]) for k in KEYS)
    # Dataset semantics
    assert len(plh) == g["out_f0"].shape[0]
    item = plh[len(plh) - 1]
    assert list(item) == list(KEYS) and np.array_equal(item["loudness"].numpy(), g["out_loudness"][-1])


def test_audio_data_alone_and_file_order(tmp_path):
    g, conf = fixture("g26_dataset_mix", tmp_path)
    a = ddsp.AudioData(conf, device="cpu")
    assert len(a) == g["out_audio"].shape[0] and np.array_equal(a[2].numpy(), g["out_audio"][2])
    # sorted discovery, one sub-directory level only: the decoys at the top level and two levels down are not read
    files = dataset.find_audio_files(conf.data_dir)
    assert files == sorted(files) and len(files) == 4 and all(f[len(conf.data_dir):].count("/") == 2 for f in files)


def test_caches_load_both_ways(tmp_path):
    g = load_golden("g26_dataset_mix")
    # a cache the reference wrote (torch.save of a tensor / of a dict of CPU tensors) in a folder with no audio at all
    d = tmp_path / "ref_cache"
    d.mkdir()
    conf = fixture_conf(g, d)
    ref_final = {k: torch.from_numpy(g[f"out_{k}"]) for k in KEYS}
    torch.save(ref_final["audio"], str(d / "audio_dataset.pth"))
    torch.save(ref_final, str(d / "plh_dataset.pth"))
    a, plh = ddsp.AudioData(conf, device="cpu"), ddsp.PLHDataset(conf, device="cpu")
    assert torch.equal(a.audios, ref_final["audio"])
    assert all(torch.equal(plh.final[k], ref_final[k]) for k in KEYS)
    # AudioData's cache alone (the reference's PLHDataset then encodes the cached examples): the features are rebuilt from it
    (d / "plh_dataset.pth").unlink()
    plh = ddsp.PLHDataset(conf, device="cpu")
    assert all(np.array_equal(plh.final[k].numpy(), g[f"out_{k}"], equal_nan=True) for k in KEYS)
    # clear=True ignores a (here: wrong) cache and rebuilds both from the files
    e = tmp_path / "clear"
    e.mkdir()
    conf = fixture_conf(g, write_folder(g, e))
    torch.save(torch.zeros(1, 5), str(e / "audio_dataset.pth"))
    torch.save({"f0": torch.zeros(1)}, str(e / "plh_dataset.pth"))
    assert len(ddsp.PLHDataset(conf, device="cpu")) == 1                      # the cache is used when it exists
    plh = ddsp.PLHDataset(conf, clear=True, device="cpu")
    assert all(np.array_equal(plh.final[k].numpy(), g[f"out_{k}"], equal_nan=True) for k in KEYS)
    assert torch.equal(torch.load(str(e / "audio_dataset.pth"), weights_only=True), ref_final["audio"])


def test_refusals(tmp_path):
    g = load_golden("g26_dataset_mix")
    conf = fixture_conf(g, tmp_path)
    with pytest.raises(ValueError, match="No valid audio files"):
        ddsp.AudioData(conf, device="cpu")
    (tmp_path / "a").mkdir()
    # a file shorter than one example is named, not an unfold error
    wavfile.write(str(tmp_path / "a" / "short.wav"), 22050, np.zeros(5000, np.int16))
    with pytest.raises(ValueError, match="short.wav"):
        ddsp.AudioData(conf, device="cpu")
    # mp3 / ogg: listed, never dropped
    (tmp_path / "a" / "short.wav").unlink()
    wavfile.write(str(tmp_path / "a" / "ok.wav"), 22050, np.zeros(9000, np.int16))
    for ext in ("mp3", "ogg"):
        (tmp_path / "a" / f"song.{ext}").write_bytes(b"\0" * 16)
    with pytest.raises(ValueError, match=r"song\.mp3.*song\.ogg"):
        ddsp.AudioData(conf, device="cpu")
    for ext in ("mp3", "ogg"):
        (tmp_path / "a" / f"song.{ext}").unlink()
    # WAV sample formats the device path does not take
    wavfile.write(str(tmp_path / "a" / "ok.wav"), 22050, np.zeros(9000, np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ddsp.AudioData(conf, device="cpu")
    with pytest.raises(ValueError, match="CREPE weights"):
        wavfile.write(str(tmp_path / "a" / "ok.wav"), 22050, np.zeros(9000, np.int16))
        conf.crepe_weights = None
        ddsp.PLHDataset(conf, clear=True, device="cpu")
    with pytest.raises(ValueError, match="device"):
        dataset.pcm_to_mono(torch.zeros(10, 2, dtype=torch.int16))


def test_load_audio_restates_torchaudio_scaling(tmp_path):
    rng = np.random.default_rng(5)
    for dtype, scale in ((np.int16, 32768.0), (np.int32, 2.0 ** 31), (np.float32, None)):
        x = (rng.standard_normal((700, 3)) * (0.3 if scale is None else 3000)).astype(dtype)
        if dtype == np.int32:
            x = x << 8                                                # 24-bit, left-justified
        wavfile.write(str(tmp_path / "x.wav"), 16000, x)
        pcm, sr = ddsp.load_audio(str(tmp_path / "x.wav"))
        assert sr == 16000 and pcm.dtype == dtype and pcm.shape == (700, 3) and np.array_equal(pcm, x)
        y = dataset.pcm_to_float(pcm)
        assert y.shape == (3, 700) and y.dtype == torch.float32 and y.is_contiguous()
        ref = x.T.astype(np.float32) if scale is None else (x.T.astype(np.float64) / scale).astype(np.float32)
        assert np.array_equal(y.numpy(), ref)
    wavfile.write(str(tmp_path / "m.wav"), 8000, np.zeros(10, np.int16))
    assert ddsp.load_audio(str(tmp_path / "m.wav"))[0].shape == (10, 1)


def test_dataset_entry_points_validate_without_gpu():
    L = ddsp._lib.lib()
    # ddsp_pcm_to_mono(pcm, y, L, C, format, stream)
    assert L.ddsp_pcm_to_mono(None, None, 0, 2, 1, None) == 0                 # nothing to do
    assert L.ddsp_pcm_to_mono(None, None, 100, 2, 1, None) == -1
    assert L.ddsp_pcm_to_mono(8, 8, 100, 0, 1, None) == -1
    assert L.ddsp_pcm_to_mono(8, 8, -1, 2, 1, None) == -1
    for fmt in (0, 4, -1):
        assert L.ddsp_pcm_to_mono(8, 8, 100, 2, fmt, None) == -1
    assert L.ddsp_pcm_to_mono(8, 8, 100, 65536, 1, None) == -2
    assert L.ddsp_pcm_to_mono(8, 8, 1 << 62, 4, 1, None) == -2
    # ddsp_make_examples(y, y_len, files, n_files, e0, E, duration, step, p, enc_in, audio, stream)
    ok = (8, 100, 8, 1, 0, 1, 50, 10, 4, 8, 8, None)

    def call(**kw):
        names = ("y", "y_len", "files", "n_files", "e0", "E", "duration", "step", "p", "enc_in", "audio", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return L.ddsp_make_examples(*(args[n] for n in names))

    assert call(E=0) == 0
    for kw in ({"y": None}, {"files": None}, {"enc_in": None, "audio": None}, {"y_len": 0}, {"n_files": 0}, {"e0": -1},
               {"E": -1}, {"duration": 0}, {"step": 0}, {"p": -1}):
        assert call(**kw) == -1, kw
    assert call(duration=1 << 31) == -2
    assert call(E=1 << 60, duration=1 << 20) == -2
    assert call(e0=(1 << 63) - 1) == -2
