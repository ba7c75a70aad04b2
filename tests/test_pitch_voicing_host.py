"""CPU checks of `pitch_voicing` (encoder.py): the numpy branch against the plain-loop definition of
tests/pitch_voicing_reference.py bit for bit, the consequences of the definition, argument validation, the C entry points'
declarations and their validation, and the `Encoder(voicing=)` wiring."""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import pitch_voicing_reference as ref
from ddsp_pytorch_amd.encoder import VOICING_FILLS, pitch_voicing
from conftest import load_golden
from encoder_common import Conf, AEConf, crepe_weights
from test_host_abi import declared_prototypes

NEW_SYMBOLS = ("ddsp_pitch_voicing_workspace_bytes", "ddsp_pitch_voicing")
KEYS = ("f0", "voiced", "normalized", "periodicity")


def same_bits(a, b):
    """fp32 arrays equal bit for bit, NaNs compared as equal (bool arrays: equal)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == bool:
        return np.array_equal(a, b)
    assert a.dtype == np.float32
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint32), b[~nan_b].view(np.uint32))


def run(x, state=None, with_loud=False, device="cpu", **kw):
    """pitch_voicing on the inputs of ref.make -> dict of numpy [B, T] (state [B, 3])"""
    t = {k: torch.from_numpy(v)[..., None].to(device) for k, v in x.items()}
    if with_loud:
        kw.setdefault("silence", float(ref.SILENCE))
    out = pitch_voicing(t["f0"], t["p"], t["n"], t["loud"] if with_loud else None,
                        state=None if state is None else torch.from_numpy(state).to(device), return_state=True, **kw)
    got = {k: v[..., 0].cpu().numpy() for k, v in zip(KEYS, out)}
    got["state"] = out[4].cpu().numpy()
    return got


def want(x, state=None, with_loud=False, **kw):
    if with_loud:
        kw.setdefault("silence", float(ref.SILENCE))
    return ref.voicing(x["f0"], x["n"], x["p"], x["loud"] if with_loud else None, state, **kw)


def test_new_symbols_declared_exported_and_bound():
    names = list(declared_prototypes())
    L = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in names and name in ddsp._lib.EXPORTS and name in ddsp._lib.SIGNATURES and hasattr(L, name), name
    at = names.index("ddsp_pitch_viterbi")
    assert tuple(names[at + 1:at + 3]) == NEW_SYMBOLS
    assert list(ddsp._lib.SIGNATURES)[at + 1:at + 3] == list(NEW_SYMBOLS)
    assert ddsp._lib.ABI_VERSION == 5 == ddsp._lib.lib().ddsp_hip_abi_version()      # adding symbols is compatible
    assert ddsp.pitch_voicing is pitch_voicing and "pitch_voicing" in ddsp.__all__
    assert VOICING_FILLS == ref.FILLS                                               # the codes of DDSP_VOICING_FILL_*


def test_entry_point_validates_without_gpu():
    L = ddsp._lib.lib()
    word = ctypes.c_uint64(0)                      # (a valid address; nothing is read from it)
    p = ctypes.addressof(word)

    def call(f0=p, n=p, per=p, f0_out=p, n_out=p, voiced=p, work=None, B=1, T=8, wp=3, wf=3, upper=0.31, lower=0.19, fill=1):
        return L.ddsp_pitch_voicing(f0, n, per, None, None, f0_out, n_out, voiced, None, None, work, B, T, wp, wf, upper, lower, 0.0, fill, None)

    for missing in ("f0", "n", "per", "f0_out", "n_out", "voiced"):
        assert call(**{missing: None}) == -1, missing
    assert call(B=0) == 0 and call(B=0, f0=None) == 0                       # empty batch
    assert call(B=-1) == -1 and call(T=0) == -1
    for w in (0, 2, 4, 11, -1):
        assert call(wp=w) == -1 and call(wf=w) == -1
    assert call(upper=0.1, lower=0.2) == -1
    assert call(fill=3) == -1 and call(fill=-1) == -1
    assert call(T=1 << 24) == -2 and call(B=1 << 20, T=1 << 11) == -2      # T >= 2^24, B T >= 2^31
    assert L.ddsp_pitch_voicing_workspace_bytes(16, 172) == 0 and L.ddsp_pitch_voicing_workspace_bytes(0, 100000) == 0
    T = 1
    while L.ddsp_pitch_voicing_workspace_bytes(1, T) == 0:
        T *= 2
    assert T <= 1 << 16                                                      # (a row's intermediates fit in LDS up to some T)
    assert L.ddsp_pitch_voicing_workspace_bytes(3, T) == 3 * L.ddsp_pitch_voicing_workspace_bytes(1, T)
    assert call(T=T) == -1                                                  # a row this long needs the workspace


def test_oracle_lower_median():
    assert ref.lower_median([(0.5, 3)]) == (0.5, 3)
    assert ref.lower_median([(0.5, 3), (0.25, 4)]) == (0.25, 4)             # even count: the lower of the middle two
    assert ref.lower_median([(0.5, 1), (0.5, 0), (0.5, 2)]) == (0.5, 1)     # ties by frame
    assert ref.lower_median([(0.0, 2), (-0.0, 3), (1.0, 0), (-1.0, 1)]) == (0.0, 2)


@pytest.mark.parametrize("T", [1, 2, 5, 64, 65])
@pytest.mark.parametrize("fill", ref.FILLS)
def test_cpu_equals_oracle_bit_for_bit(fill, T):
    for i, (wp, wf) in enumerate((a, b) for a in (1, 3, 9) for b in (1, 3, 9)):
        for with_loud in (False, True):
            for with_state in (False, True):
                B = 3
                x = ref.make(1000 * T + 10 * i + with_loud, B, T, nans=(i % 2 == 1))
                state = ref.make_state(T + i, B) if with_state else None
                kw = dict(period_window=wp, pitch_window=wf, fill=fill)
                got, exp = run(x, state, with_loud, **kw), want(x, state, with_loud, **kw)
                for k in KEYS + ("state",):
                    assert same_bits(got[k], exp[k]), (k, wp, wf, with_loud, with_state, got[k], exp[k])


def test_inputs_reach_every_mechanism():
    """the seeded maker gives voiced and unvoiced frames, frames inside the band, both exact thresholds, ties and gaps"""
    x = ref.make(5, 4, 172)
    exp = want(x, None, True, period_window=1)
    ps, m = exp["periodicity"], exp["voiced"]
    assert (ps == ref.UPPER).any() and (ps == ref.LOWER).any() and ((ps > ref.LOWER) & (ps < ref.UPPER)).any()
    assert 0.1 < m.mean() < 0.9
    assert (np.diff(x["n"], axis=1) == 0).mean() > 0.2
    assert want(x, None, False, fill="interpolate")["interpolated"].any()
    assert (x["loud"] < ref.SILENCE).any() and (x["loud"] >= ref.SILENCE).any()


def test_unvoiced_row_passes_through_and_voiced_frames_with_window_one():
    x = ref.make(7, 2, 65, kind="unvoiced")
    for fill in ref.FILLS:
        got = run(x, fill=fill)
        assert not got["voiced"].any() and same_bits(got["f0"], x["f0"]) and same_bits(got["normalized"], x["n"])
        assert np.array_equal(got["state"][:, 0], np.zeros(2)) and np.isnan(got["state"][:, 1:]).all()
    x = ref.make(8, 3, 65, nans=True)
    for fill in ref.FILLS:
        got = run(x, pitch_window=1, fill=fill)
        m = got["voiced"]
        assert m.any() and same_bits(got["f0"][m], x["f0"][m]) and same_bits(got["normalized"][m], x["n"][m])
    allv = run(ref.make(9, 2, 65, kind="voiced"), pitch_window=1)
    assert allv["voiced"].all()
    # a voiced frame's pair is a decoded pair: its f0 names the frame, and that frame's n is the output
    x = ref.make(10, 2, 172)
    got = run(x, pitch_window=9)
    for r in range(2):
        for t in np.nonzero(got["voiced"][r])[0]:
            u = int(np.nonzero(x["f0"][r] == got["f0"][r, t])[0][0])
            assert abs(u - t) <= 4 and got["voiced"][r, u] and got["normalized"][r, t] == x["n"][r, u]


def test_state_carries_a_row_across_two_blocks():
    """Wp = Wf = 1 and 'hold': two blocks with the state carried equal the whole row when the cut lies after the first
    voiced frame (a leading gap looks ahead)."""
    checked = 0
    for seed in range(40):
        T = 96
        x = ref.make(300 + seed, 1, T)
        whole = run(x, period_window=1, pitch_window=1, fill="hold")
        voiced = np.nonzero(whole["voiced"][0])[0]
        if not len(voiced) or voiced[0] >= T - 2:
            continue
        cut = int(np.random.default_rng(seed).integers(voiced[0] + 1, T - 1))
        first = run({k: v[:, :cut] for k, v in x.items()}, period_window=1, pitch_window=1, fill="hold")
        second = run({k: np.ascontiguousarray(v[:, cut:]) for k, v in x.items()}, state=first["state"], period_window=1,
                     pitch_window=1, fill="hold")
        for k in KEYS:
            assert same_bits(np.concatenate([first[k], second[k]], axis=1), whole[k]), (seed, cut, k)
        assert same_bits(second["state"], whole["state"])
        checked += 1
    assert checked >= 20


def test_argument_validation():
    f = torch.zeros(2, 8, 1)
    ok = ddsp.pitch_voicing(f, f, f)
    assert len(ok) == 4 and ok[1].dtype == torch.bool and all(tuple(v.shape) == (2, 8, 1) for v in ok)
    assert all(v.dtype == torch.float32 for v in (ok[0], ok[2], ok[3]))
    five = ddsp.pitch_voicing(f, f, f, return_state=True)
    assert len(five) == 5 and tuple(five[4].shape) == (2, 3) and five[4].dtype == torch.float32
    assert len(ddsp.pitch_voicing(f, f, f, state=five[4])) == 5
    for bad in (dict(period_window=2), dict(pitch_window=11), dict(fill="linear"), dict(upper=0.1, lower=0.2),
                dict(state=torch.zeros(2, 2))):
        with pytest.raises(ValueError):
            ddsp.pitch_voicing(f, f, f, **bad)
    with pytest.raises(ValueError):
        ddsp.pitch_voicing(f[:, :7], f, f)
    with pytest.raises(ValueError):
        ddsp.pitch_voicing(f, f, f[..., 0])
    with pytest.raises(ValueError):
        ddsp.pitch_voicing(f, f, f, torch.zeros(2, 9, 1), silence=0.5)     # a loudness with another frame count
    with pytest.raises(ValueError):
        ddsp.pitch_voicing(f, f[:, :0], f)
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.pitch_voicing(f, f.clone().requires_grad_(), f)
    with pytest.raises(RuntimeError, match="no backward"):
        ddsp.pitch_voicing(f, f, f, f.clone().requires_grad_(), silence=0.5)
    # silence=None or loudness=None switches the gate off
    x = ref.make(5, 4, 172)
    assert same_bits(run(x, with_loud=True, silence=None)["voiced"], run(x)["voiced"])
    assert not same_bits(run(x, with_loud=True)["voiced"], run(x)["voiced"])
    assert "not tuned" in ddsp.pitch_voicing.__doc__


def test_encoder_wiring_on_cpu():
    g = load_golden("g21_f0_tiny")
    w = crepe_weights("tiny", g["crepe_seed"])
    conf = Conf(44100, 2048, 512)
    p = conf.n_fft - conf.hop_length
    x = torch.nn.functional.pad(torch.from_numpy(g["clips_x"]), (p // 2, p - p // 2))
    plain = ddsp.Encoder(conf, weights=w)(x)
    off = ddsp.Encoder(conf, weights=w, voicing=None)(x)
    assert list(off) == list(plain) == ["f0", "harmonicity", "loudness", "probabilities", "normalized_cents"]
    assert all(torch.equal(off[k], plain[k]) for k in plain)
    # thresholds inside the range the seeded weights' periodicity covers, so that both kinds of frame occur
    h = plain["harmonicity"]
    upper, lower = float(h.quantile(0.6)), float(h.quantile(0.4))
    silence = float(plain["loudness"].quantile(0.2))
    for voicing in (True, dict(upper=upper, lower=lower, silence=silence, fill="interpolate", pitch_window=5)):
        on = ddsp.Encoder(conf, weights=w, voicing=voicing)(x)
        assert list(on) == list(plain) + ["voiced"]
        kw = {} if voicing is True else voicing
        f0, voiced, n, _ = ddsp.pitch_voicing(plain["f0"], plain["harmonicity"], plain["normalized_cents"], plain["loudness"], **kw)
        assert torch.equal(on["f0"], f0) and torch.equal(on["voiced"], voiced) and torch.equal(on["normalized_cents"], n)
        for k in ("harmonicity", "loudness", "probabilities"):
            assert torch.equal(on[k], plain[k])
    assert 0 < int(on["voiced"].sum()) < on["voiced"].numel() and not torch.equal(on["f0"], plain["f0"])
    with pytest.raises(ValueError, match="unknown keys"):
        ddsp.Encoder(conf, weights=w, voicing=dict(window=3))
    with pytest.raises(ValueError):
        ddsp.Encoder(conf, weights=w, voicing="on")
    conf.pitch_voicing = dict(fill="none")
    assert ddsp.Encoder(conf, weights=w).voicing == dict(fill="none")
    assert ddsp.Encoder(conf, weights=w, voicing=True).voicing == {}                        # the argument wins
    assert ddsp.Encoder(conf, weights=w, voicing=False).voicing is None

    class VoicedConf(AEConf):
        pitch_voicing = True
    assert ddsp.AutoEncoder(VoicedConf, weights=w).encoder.voicing == {}
    assert ddsp.AutoEncoder(AEConf, weights=w).encoder.voicing is None
    assert ddsp.AutoEncoder(AEConf, weights=w, voicing=dict(fill="interpolate")).encoder.voicing == dict(fill="interpolate")
