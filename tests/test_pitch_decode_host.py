"""CPU checks of the pitch decoders (encoder.py: pitch_argmax / pitch_centered / pitch_weighted / pitch_viterbi and
F0Encoder's `decoder=`): the new C entry points' declarations and argument validation, the fp64 oracle against a brute
force, and the stock-op branches against the oracle (tests/pitch_decode_reference.py)."""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import pitch_decode_reference as ref
from conftest import load_golden
from encoder_common import Conf, AEConf, crepe_weights
from test_host_abi import declared_prototypes

NEW_SYMBOLS = ("ddsp_pitch_centered", "ddsp_pitch_viterbi_workspace_bytes", "ddsp_pitch_viterbi")


@pytest.fixture(scope="module")
def log_a():
    return ref.log_transition()


def test_new_symbols_declared_exported_and_bound():
    protos = declared_prototypes()
    names = list(protos)
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos and name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name), name
    at = names.index("ddsp_pitch_decode")
    assert tuple(names[at + 1:at + 4]) == NEW_SYMBOLS                      # after ddsp_pitch_decode, in this order
    assert list(ddsp._lib.SIGNATURES)[at + 1:at + 4] == list(NEW_SYMBOLS)
    assert ddsp._lib.ABI_VERSION == 5                                       # adding symbols is compatible
    for name in ("pitch_argmax", "pitch_centered", "pitch_weighted", "pitch_viterbi"):
        assert getattr(ddsp, name) is getattr(ddsp.encoder, name)


def test_entry_points_validate_without_gpu():
    L = ddsp._lib.lib()
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)
    assert L.ddsp_pitch_centered(None, None, None, None, None, None, 4, None) == -1
    assert L.ddsp_pitch_centered(p, None, p, p, None, None, 4, None) == -1         # a required output missing
    assert L.ddsp_pitch_centered(p, None, p, p, p, None, -1, None) == -1
    assert L.ddsp_pitch_centered(None, None, None, None, None, None, 0, None) == 0
    assert L.ddsp_pitch_centered(p, None, p, p, p, None, 1 << 40, None) == -2
    assert L.ddsp_pitch_viterbi(None, None, None, None, None, None, 1, 4, None) == -1
    assert L.ddsp_pitch_viterbi(p, p, None, None, None, None, 1, 4, None) == -1    # no bins
    assert L.ddsp_pitch_viterbi(p, p, None, None, p, None, 1, 0, None) == -1       # T <= 0
    assert L.ddsp_pitch_viterbi(p, p, None, None, p, None, -1, 4, None) == -1
    assert L.ddsp_pitch_viterbi(p, p, None, None, p, None, 0, 4, None) == 0        # empty batch
    assert L.ddsp_pitch_viterbi(p, p, None, None, p, None, 1 << 40, 4, None) == -2
    assert L.ddsp_pitch_viterbi(p, p, None, None, p, None, 1, 1 << 40, None) == -2
    assert L.ddsp_pitch_viterbi(p, p, None, None, p, None, 1, 500, None) == -1     # a row this long needs the workspace
    assert L.ddsp_pitch_viterbi_workspace_bytes(16, 172) == 0 and L.ddsp_pitch_viterbi_workspace_bytes(0, 500) == 0
    assert L.ddsp_pitch_viterbi_workspace_bytes(3, 500) == 3 * 500 * 360


def test_transition_table_is_the_oracles(log_a):
    table = ddsp.encoder.viterbi_log_transition()
    assert table.dtype == torch.float32 and tuple(table.shape) == (360, 23)
    assert np.array_equal(table.numpy().astype(np.float64), log_a)
    # rows of A sum to one: 144 in the interior, less at the ends
    A = np.zeros((360, 360))
    for j in range(360):
        for d in range(23):
            if np.isfinite(log_a[j, d]):
                A[j + d - 11, j] = np.exp(log_a[j, d])
    assert np.abs(A.sum(axis=1) - 1).max() <= 1e-6
    assert abs(A[180, 180] - 12 / 144) <= 1e-8 and abs(A[0, 0] - 12 / 78) <= 1e-8 and np.isinf(log_a[0, :11]).all()


@pytest.mark.parametrize("T", [1, 2, 3])
def test_oracle_dp_equals_brute_force(T, log_a):
    for seed, kind in ((1, "rand"), (2, "track"), (3, "rand")):
        p = ref.make(kind, 100 * T + seed, T)
        path, last = ref.viterbi(p, None, log_a)
        bpath, bscore = ref.brute_force(p, log_a)
        assert np.array_equal(path, bpath), (kind, path, bpath)
        assert last.max() == bscore == ref.path_score(path, p, log_a)


def test_tie_rule_lower_state():
    p = np.full((1, 360), 0.25, dtype=np.float32)
    assert ref.viterbi(p)[0][0] == 0 and ref.brute_force(p)[0][0] == 0
    assert int(ddsp.pitch_viterbi(torch.from_numpy(p)[None])[0, 0, 0]) == 0


@pytest.mark.parametrize("T", [13, 64, 172])
@pytest.mark.parametrize("kind", ["track", "rand"])
def test_cpu_viterbi_equals_oracle_exactly(kind, T, log_a):
    rows = [ref.make(kind, 7 * T + r, T) for r in range(2)]
    bins = ddsp.pitch_viterbi(torch.from_numpy(np.stack(rows)))
    assert bins.dtype == torch.int64 and tuple(bins.shape) == (2, T, 1)
    for r, p in enumerate(rows):
        path = ref.viterbi(p, None, log_a)[0]
        assert np.array_equal(bins[r, :, 0].numpy(), path), (kind, T, r)
        assert np.abs(np.diff(path)).max() <= 11                          # every path moves at most 11 bins per frame


def test_cpu_viterbi_state_carries_the_recurrence():
    p = torch.from_numpy(np.stack([ref.make("track", 5, 64), ref.make("rand", 6, 64)]))
    whole, last = ddsp.pitch_viterbi(p, return_state=True)
    _, mid = ddsp.pitch_viterbi(p[:, :32], return_state=True)
    second, last2 = ddsp.pitch_viterbi(p[:, 32:], state=mid)
    assert tuple(last.shape) == (2, 360) and last.dtype == torch.float32
    assert (last2 - last).abs().max().item() <= 1e-4                       # both are returned with their maximum at 0
    assert torch.equal(second[:, -1], whole[:, -1])
    with pytest.raises(ValueError):
        ddsp.pitch_viterbi(p, state=torch.zeros(2, 359))
    with pytest.raises(ValueError):
        ddsp.pitch_viterbi(p[0])


def test_viterbi_takes_no_displaced_frame_and_argmax_takes_all():
    for seed in (11, 12, 13):
        p, centre, displaced = ref.track(seed, 172)
        assert 8 <= displaced.sum() <= 30
        path = ddsp.pitch_viterbi(torch.from_numpy(p)[None])[0, :, 0].numpy()
        top = p.argmax(axis=-1)
        moved = np.minimum(centre + 120.0, 357.0)
        assert np.all(np.abs(top[displaced] - moved[displaced]) <= 2)      # argmax follows every displaced peak
        assert np.all(np.abs(path - centre) <= 8), np.abs(path - centre).max()    # the path stays on the track everywhere
        assert np.all(np.abs(path[displaced] - moved[displaced]) >= 50)
        assert np.abs(np.diff(path)).max() <= 11
        assert 0.05 <= (path != top).mean() <= 0.40


CENTRES = [0, 1, 3, 4, 180, 355, 356, 358, 359]


def test_cpu_centered_matches_oracle_at_edges_and_interior():
    p = np.random.default_rng(3).random((2, len(CENTRES), 360), dtype=np.float32)
    c = np.array([CENTRES, CENTRES[::-1]])
    f, h, n = ddsp.pitch_centered(torch.from_numpy(c)[..., None], torch.from_numpy(p))
    want = ref.centered(c, p)
    assert f.dtype == h.dtype == n.dtype == torch.float32 and tuple(f.shape) == tuple(h.shape) == tuple(n.shape) == (2, 9, 1)
    cents = 1200 * np.log2(f[..., 0].numpy().astype(np.float64) / 10)
    assert np.abs(cents - want["cents"]).max() <= 1e-3
    assert np.abs(f[..., 0].numpy() / want["f0"] - 1).max() <= 2e-6
    assert np.abs(n[..., 0].numpy() - want["normalized_cents"]).max() <= 3e-7
    assert np.array_equal(h[..., 0].numpy(), np.take_along_axis(p, c[..., None], axis=-1)[..., 0])
    with pytest.raises(ValueError):
        ddsp.pitch_centered(torch.from_numpy(c), torch.from_numpy(p))     # centre without its trailing axis
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.pitch_weighted(torch.from_numpy(p).requires_grad_())


def test_each_probability_is_paired_with_its_own_bin():
    """The frame of DESIGN section 10: p[100] = 0.9, p[101] = 0.6, noise <= 0.05 elsewhere.  The correctly paired average is
    4002.66 cents; the reference's pairing (probabilities in bin order against cents in the order c .. c + 4, c - 4 .. c - 1)
    gives 4012.12, and the argmax bin is 3997.38.  A port of the rotated pairing fails here."""
    torch.manual_seed(0)
    p = (torch.rand(360) * 0.05).numpy()
    p[100], p[101] = 0.9, 0.6
    want = float(ref.centered(np.array(100), p)["cents"])
    window = p[96:105].astype(np.float64)
    rotated = float((window * ref.cents_map(np.array([100, 101, 102, 103, 104, 96, 97, 98, 99]))).sum() / window.sum())
    assert abs(want - 4002.66) < 0.005 and abs(rotated - 4012.12) < 0.005 and abs(float(ref.cents_map(100)) - 3997.38) < 0.005
    f, h, n = ddsp.pitch_weighted(torch.from_numpy(p)[None, None])
    got = 1200 * np.log2(float(f) / 10)
    assert abs(got - want) <= 1e-3, (got, want)
    assert float(h) == p[100]
    assert abs(float(n) - (want - ref.cents_map(0)) / 7180.0) <= 3e-7
    nan = torch.full((1, 1, 360), float("nan"))
    assert all(torch.isnan(v).all() for v in ddsp.pitch_weighted(nan))
    assert int(ddsp.pitch_viterbi(torch.cat([nan, nan], dim=1)).max()) <= 359


def test_pitch_argmax_is_the_reference_forward():
    p = torch.from_numpy(ref.rand(4, 12))[None]
    f, h, n = ddsp.pitch_argmax(p)
    bins = p.argmax(dim=-1, keepdim=True)
    assert torch.equal(f, 10 * 2 ** ((bins * 20 + 1997.3794084376191) / 1200)) and torch.equal(h, p.gather(-1, bins))
    assert torch.equal(n, bins / 359.)


def test_f0_encoder_decoders_on_cpu():
    g = load_golden("g21_f0_tiny")
    w = crepe_weights("tiny", g["crepe_seed"])
    x = torch.from_numpy(g["clips_x"])
    conf = Conf(44100, 2048, 512)
    default = ddsp.F0Encoder(conf, weights=w)
    assert default.decoder == "argmax"
    a, b = default(x), ddsp.F0Encoder(conf, weights=w, decoder="argmax")(x)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert default.min_cents == 1997.3794084376191 and default.max_cents == default.cents_map(359)
    assert default.normalize_cents(default.max_cents) == 1.0 and abs(default.freq_map(default.min_cents) - 31.7) < 0.05

    weighted = ddsp.F0Encoder(conf, weights=w, decoder="weighted")
    f, h, probs, n = weighted(x)
    assert torch.equal(probs, a[2])
    for got, want in zip((f, h, n), weighted.pitch_weighted(probs)):
        assert got.shape == a[0].shape and torch.equal(got, want)
    assert not torch.equal(f, a[0])

    f, h, probs, n = ddsp.F0Encoder(conf, weights=w, decoder="viterbi")(x)
    bins = ddsp.pitch_viterbi(probs)
    for got, want in zip((f, h, n), ddsp.pitch_centered(bins, probs)):
        assert got.shape == a[0].shape and torch.equal(got, want)
    assert int(bins.diff(dim=1).abs().max()) <= 11

    with pytest.raises(ValueError, match="pitch decoder"):
        ddsp.F0Encoder(conf, weights=w, decoder="median")
    conf.pitch_decoder = "weighted"
    assert ddsp.F0Encoder(conf, weights=w).decoder == "weighted"
    assert ddsp.F0Encoder(conf, weights=w, decoder="viterbi").decoder == "viterbi"          # the argument wins
    conf.pitch_decoder = "nearest"
    with pytest.raises(ValueError, match="pitch decoder"):
        ddsp.F0Encoder(conf, weights=w)

    class ViterbiConf(AEConf):
        pitch_decoder = "viterbi"
    assert ddsp.AutoEncoder(ViterbiConf, weights=w).encoder.f0_encoder.decoder == "viterbi"
    assert ddsp.AutoEncoder(AEConf, weights=w).encoder.f0_encoder.decoder == "argmax"
