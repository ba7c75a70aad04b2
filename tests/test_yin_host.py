"""The YIN pitch salience without a GPU: the entry point's binding and argument checks, the
definition's own accuracy (tests/yin_reference.py, fp64), the package's CPU form against that definition, and the
`tracker='yin'` wiring of F0Encoder / Encoder.

The 2e-4 bound on the salience (absolute; the salience lies in [0, 1]).  The fp32 forms differ from the fp64 definition by
their summation error: a sum of 512 non-negative fp32 terms carries at most 512 * 2^-24 = 3e-5 relative error, in d and again
in c, so d' = d tau / c is off by at most about 6e-5 d'.  Only d' <~ 1 survives the clip (a larger d' gives salience 0 on
both sides), and the Catmull-Rom weights sum to at most 1.25 in magnitude, over neighbouring values of d' of a few units:
1.25 * 6e-5 * (a few) <= 2e-4.  The observed maximum is printed; DESIGN.md section 10c records it."""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import yin_reference as ref
from encoder_common import Conf, crepe_weights

TOL = 2e-4
EINVAL, ERANGE = -1, -2


def test_symbol_is_exported_and_bound():
    assert "ddsp_yin_salience" in ddsp._lib.EXPORTS
    order = list(ddsp._lib.EXPORTS)
    assert order.index("ddsp_pitch_voicing") < order.index("ddsp_yin_salience") < order.index("ddsp_loudness_supported")
    fn = ddsp._lib.lib().ddsp_yin_salience
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p] * 3 + [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
    assert ddsp._lib.lib().ddsp_hip_abi_version() == 5
    assert ddsp.pitch_salience_yin is ddsp.encoder.pitch_salience_yin


def test_argument_checks_return_before_any_launch():
    """Every call here is refused (or is the empty batch) by the host checks: the pointers are never dereferenced."""
    fn = ddsp._lib.lib().ddsp_yin_salience
    p = 4096                                                    # a non-null, 16-byte aligned address that is never read
    assert fn(None, None, None, 0, 2048, 512, 3, None) == 0     # B == 0
    for args in [(None, p, p, 2, 2048, 512, 3), (p, None, p, 2, 2048, 512, 3), (p, p, None, 2, 2048, 512, 3),
                 (p, p, p, -1, 2048, 512, 3), (p, p, p, 2, 1023, 512, 1), (p, p, p, 2, 0, 512, 1), (p, p, p, 2, 2048, 0, 3),
                 (p, p, p, 2, 2048, -5, 3), (p, p, p, 2, 2048, 512, 0), (p, p, p, 2, 2048, 512, -1),
                 (p, p, p, 2, 2048, 512, 4),                     # (T - 1) hop + 1024 = 2560 > Lr
                 (p, p, p, 2, 1024, 1, 2),
                 (p, p, p, 1, 1 << 40, 1 << 30, 1 << 40),        # (T - 1) hop overflows a long: still the frame check
                 (p, p + 4, p, 2, 2048, 512, 3)]:                # the table is read 16 bytes at a time
        assert fn(*args, None) == EINVAL, args
    for args in [(p, p, p, 1 << 40, 1 << 40, 1, 1),              # B Lr
                 (p, p, p, 1 << 49, 2048, 1, 1025),              # 360 B T alone: B Lr = 2^60 is still accepted
                 (p, p, p, 1 << 31, 1 << 40, 1, 1 << 31)]:       # B T
        assert fn(*args, None) == ERANGE, args


def test_wrapper_refuses_bad_inputs():
    with pytest.raises(ValueError):
        ddsp.pitch_salience_yin(torch.zeros(2, 1023), 512)
    with pytest.raises(ValueError):
        ddsp.pitch_salience_yin(torch.zeros(2, 2048), 0)
    with pytest.raises(ValueError):
        ddsp.pitch_salience_yin(torch.zeros(2048), 512)
    with pytest.raises(RuntimeError):
        ddsp.pitch_salience_yin(torch.zeros(1, 2048, requires_grad=True), 512)


def test_definition_decodes_the_tones_within_30_cents():
    """The condition on the inputs, for the fp64 reference alone: 64 tones over 50 .. 900 Hz, nine-bin weighted average."""
    _, s = ref.salience(ref.tone_frames(), 512)
    err = np.abs(ref.weighted_cents(s[:, 0]) - ref.cents_of(ref.TONE_F0))
    print(f"reference: max {err.max():.2f} cents, median {np.median(err):.2f}, peak salience >= {s.max(axis=-1).min():.3f}")
    assert err.max() <= 30.0, (err.max(), ref.TONE_F0[err.argmax()])


def test_cpu_form_matches_the_definition():
    y = np.concatenate([ref.tone_frames(), ref.edge_frames()])
    _, want = ref.salience(y, 512)
    got = ddsp.pitch_salience_yin(torch.from_numpy(y.copy()), 512)
    assert got.dtype == torch.float32 and tuple(got.shape) == (y.shape[0], 1, 360)
    err = np.abs(got.numpy().astype(np.float64) - want)
    print(f"CPU form against fp64: max |salience difference| = {err.max():.3e}")
    assert err.max() <= TOL
    for cost in (0.0, 0.1):
        _, want = ref.salience(y, 512, cost)
        got = ddsp.pitch_salience_yin(torch.from_numpy(y.copy()), 512, cost).numpy()
        assert np.abs(got - want).max() <= TOL, cost


def test_cpu_form_over_a_row_of_frames():
    y = ref.rows(3, 1024 + 5 * 92 + 17, 5)
    _, want = ref.salience(y, 92)
    got = ddsp.pitch_salience_yin(torch.from_numpy(y), 92).numpy()
    assert got.shape == want.shape == (3, 6, 360)
    assert np.abs(got - want).max() <= TOL


def test_edge_frames():
    e = ref.edge_frames()
    for where, s in (("reference", ref.salience(e, 512)[1][:, 0]),
                     ("cpu", ddsp.pitch_salience_yin(torch.from_numpy(e.copy()), 512)[:, 0].numpy())):
        assert np.isfinite(s).all(), where
        assert not s[0].any(), (where, "zero frame")
        assert not s[1].any(), (where, "constant frame")
        assert s[2].max() < 0.19, (where, "white noise", s[2].max())
    bad = e[2:3].copy()
    bad[0, 700] = np.nan                                         # in the second half: only some lags touch it
    assert not ddsp.pitch_salience_yin(torch.from_numpy(bad), 512).numpy().any()
    assert not ref.salience(bad, 512)[1].any()


def audio_44k(frames=12):
    rng = np.random.default_rng(9)
    L = 2048 + 512 * frames
    return torch.from_numpy(np.stack([ref.tone(220.0, L, 44100, rng, top=8000.0), ref.tone(523.25, L, 44100, rng, top=8000.0)])
                            .astype(np.float32))


def test_f0_encoder_yin_needs_no_weights():
    conf = Conf(44100, 2048, 512)
    x = audio_44k()
    enc = ddsp.F0Encoder(conf, tracker='yin')
    assert not hasattr(enc, 'model') and enc.tracker == 'yin' and not list(enc.state_dict())
    crepe = ddsp.F0Encoder(conf, weights=crepe_weights("tiny", 3))
    assert crepe.tracker == 'crepe'
    got, exp = enc(x), crepe(x)
    for a, b in zip(got, exp):
        assert a.shape == b.shape and a.dtype == b.dtype
    freq, harmonicity, probabilities, normalized_cents = got
    assert probabilities.shape[-1] == 360 and float(probabilities.min()) >= 0 and float(probabilities.max()) <= 1
    bins = probabilities.argmax(-1, keepdim=True)                # the default decoder is the argmax
    assert torch.equal(harmonicity, probabilities.gather(-1, bins)) and torch.equal(normalized_cents, bins / 359.)
    cents = ref.cents_of(freq[..., 0].numpy())
    assert np.abs(cents - ref.cents_of([[220.0], [523.25]])).max() <= 40.0    # a bin centre: half a bin on top of the 30
    for decoder in ('weighted', 'viterbi'):
        out = ddsp.F0Encoder(conf, tracker='yin', decoder=decoder)(x)
        assert [o.shape for o in out] == [o.shape for o in got]
        assert torch.equal(out[2], probabilities)
        if decoder == 'weighted':                                # ('viterbi' only has to run: DESIGN.md section 10c, its end bins)
            assert np.abs(ref.cents_of(out[0][..., 0].numpy()) - ref.cents_of([[220.0], [523.25]])).max() <= 30.0


def test_conf_pitch_tracker_reaches_the_encoder():
    conf = Conf(44100, 2048, 512)
    conf.pitch_tracker = 'yin'
    enc = ddsp.Encoder(conf)
    assert enc.f0_encoder.tracker == 'yin' and not hasattr(enc.f0_encoder, 'model')
    assert not [k for k in enc.state_dict() if k.startswith("f0_encoder.model.")]
    x = audio_44k(4)
    out = enc(x)
    direct = ddsp.F0Encoder(Conf(44100, 2048, 512), tracker='yin')(x)
    assert torch.equal(out["f0"], direct[0]) and torch.equal(out["probabilities"], direct[2])
    assert out["loudness"].shape == out["f0"].shape
    assert ddsp.Encoder(Conf(44100, 2048, 512), tracker='yin').f0_encoder.tracker == 'yin'
    assert ddsp.Encoder(conf, weights=crepe_weights("tiny", 3), tracker='crepe').f0_encoder.tracker == 'crepe'   # the argument wins


def test_crepe_still_needs_weights_and_unknown_trackers_raise():
    conf = Conf(44100, 2048, 512)
    with pytest.raises(ValueError, match="CREPE weights"):
        ddsp.F0Encoder(conf, tracker=None)
    with pytest.raises(ValueError, match="CREPE weights"):
        ddsp.Encoder(conf)
    with pytest.raises(ValueError, match="tracker"):
        ddsp.F0Encoder(conf, tracker='pyin')
    conf.pitch_tracker = 'swipe'
    with pytest.raises(ValueError, match="tracker"):
        ddsp.Encoder(conf)
