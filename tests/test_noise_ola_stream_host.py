"""The overlap-add noise as a stream (include/ddsp_hip.h: ddsp_noise_ola_stream; DESIGN.md section 5a, "Live") on the host: the
block-wise reference of tests/noise_ola_stream_reference.py against the offline definition on the padded clip, shifted by the
delay -- in fp64 to rounding, in the kernels' fp32 arithmetic in bits --, the C entry's validation, and the refusals of the
Python layers.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import noise_ola_reference as ref
import noise_ola_stream_reference as sref
from test_noise_ola_host import declared_symbols


def inputs(shape, seed=0):
    B, T, hop, F, Tb = shape
    rng = np.random.default_rng(6000 + seed)
    H = rng.random((B, T, F)).astype(np.float32)
    if T >= 3:
        H[:, 1] = 0.0                                             # a silent frame inside
    u = rng.random((B, T, hop), dtype=np.float32)
    dry = rng.standard_normal((B, T * hop)).astype(np.float32)
    return H, u, dry


def offline(fn, shape, H, u, Z):
    """The offline form on the clip with leading and trailing silent frames, as the first (T + Z) hop stream samples."""
    B, T, hop, F, Tb = shape
    lead = sref.lead_frames(hop, F)
    res = fn(sref.padded(H, lead, Z), hop, uniform=sref.padded(u, lead, Z))
    res = res if isinstance(res, tuple) else (res,)
    return [sref.shifted(r, lead, hop, F, (T + Z) * hop) for r in res]


def delayed(dry, F, n):
    B = dry.shape[0]
    return np.concatenate([np.zeros((B, sref.delay(F)), dry.dtype), dry, np.zeros((B, n), dry.dtype)], axis=1)[:, :n]


@pytest.mark.parametrize("shape", sref.HOST_SHAPES, ids=str)
def test_fp64_stream_is_the_padded_shifted_offline_form(shape):
    B, T, hop, F, Tb = shape
    H, u, dry = inputs(shape)
    x = ref.draw(B, T, hop, u)
    got, yard, Z = sref.run(H, hop, Tb, x)
    want, Yf = offline(ref.ola_fp64, shape, H, u, Z)
    r = ref.ratio(got, want, Yf)
    ry = np.abs(yard - Yf).max() / max(Yf.max(), 1e-300)
    with_dry, _, _ = sref.run(H, hop, Tb, x, dry=dry)
    rd = ref.ratio(with_dry, want + delayed(dry, F, (T + Z) * hop).astype(np.float64), Yf)
    print(f"{shape}: |stream - offline| / Yf = {r:.2e} (yardstick {ry:.2e}), with dry {rd:.2e}; flushed by {Z} silent frames")
    assert got.shape == (B, (T + Z) * hop) and r <= 1e-13 and ry <= 1e-13 and rd <= 1e-13
    if F > 2:
        assert np.abs(got[:, :sref.delay(F)]).max() > 0           # the pre-ring the offline form crops


@pytest.mark.parametrize("shape", sref.HOST_SHAPES, ids=str)
def test_fp32_stream_is_the_offline_emulation_in_bits(shape):
    """Every chain is the offline chain, started from the tail's value: zero taps add exact zeros."""
    B, T, hop, F, Tb = shape
    H, u, dry = inputs(shape)
    x = ref.draw(B, T, hop, u)
    got, _, Z = sref.run(H, hop, Tb, x, fp32=True)
    (want,) = offline(ref.ola_fp32, shape, H, u, Z)
    assert np.array_equal(got.astype(np.float32).view(np.int32), want.astype(np.float32).view(np.int32))
    with_dry, _, _ = sref.run(H, hop, Tb, x, dry=dry, fp32=True)
    sum32 = want.astype(np.float32) + delayed(dry, F, (T + Z) * hop)
    assert np.array_equal(with_dry.astype(np.float32).view(np.int32), sum32.view(np.int32))
    # after the flush the state is zero again: the tail has left and the history holds silence
    s = sref.Stream(B, F, hop, fp32=True)
    for a, b in sref.blocks_of(T, Tb):
        s.block(H[:, a:b], x[:, a:b], dry[:, a * hop:b * hop])
    if F > 2:
        assert np.abs(s.state()).max() > 0 and s.state().shape == (B, 3 * F - 6)
    for _ in range(Z // Tb + -(-sref.delay(F) // (Tb * hop))):
        s.block(np.zeros((B, Tb, F), np.float32), np.zeros((B, Tb, hop)), np.zeros((B, Tb * hop), np.float32))
    assert (s.state() == 0).all()


def test_a_non_finite_frame_reaches_its_interval_of_the_stream():
    B, T, hop, F, Tb = 1, 8, 8, 9, 1                              # tail 14, block 8: the interval crosses two block boundaries
    H, u, _ = inputs((B, T, hop, F, Tb), seed=1)
    t = 2
    H[0, t, 3] = np.nan
    got, _, Z = sref.run(H, hop, Tb, ref.draw(B, T, hop, u))
    lo, hi = t * hop, (t + 1) * hop + 2 * (F - 1) - 3
    bad = np.isnan(got[0])
    assert bad[lo:hi + 1].all() and not bad[:lo].any() and not bad[hi + 1:].any()


def test_abi_and_state_size():
    L = ddsp._lib.lib()
    assert L.ddsp_hip_abi_version() == 5 == ddsp._lib.ABI_VERSION          # additive: the version stays
    raw = ctypes.CDLL(ddsp._lib.SO_PATH)
    for name in ("ddsp_noise_ola_stream_state_floats", "ddsp_noise_ola_stream"):
        assert name in declared_symbols() and name in ddsp._lib.EXPORTS and hasattr(raw, name), name
    size = L.ddsp_noise_ola_stream_state_floats
    assert [size(F) for F in (-1, 0, 1, 2, 3, 65, 195, 257, 258)] == [0, 0, 0, 0, 3, 189, 579, 765, 0]
    assert all(size(F) == sref.state_floats(F) for F in range(2, 258))


def test_the_c_entry_validates_before_the_device():
    """No GPU here: every one of these returns before a launch (the pointers are host addresses nothing reads)."""
    L = ddsp._lib.lib()
    EINVAL, ERANGE = -1, -2
    bufs = [(ctypes.c_float * 64)() for _ in range(4)]
    p, q, s0, s1 = (ctypes.addressof(b) for b in bufs)
    big = 1 << 40
    call = L.ddsp_noise_ola_stream
    #            H  u     dry   out  s_in s_out B  T  F    hop  seed off ctr   ws ws_bytes stream
    assert call(p, None, q, p, s0, s1, 1, 4, 258, 128, 0, 0, None, p, big, None) == ERANGE
    assert call(p, None, q, p, s0, s1, 1, 4, 65, 1025, 0, 0, None, p, big, None) == ERANGE
    assert call(p, None, q, p, s0, s1, 1 << 20, 1 << 11, 65, 128, 0, 0, None, p, big, None) == ERANGE
    assert call(p, None, q, p, s0, s1, 1, 4, 1, 128, 0, 0, None, p, big, None) == EINVAL
    assert call(None, None, q, p, s0, s1, 1, 4, 65, 128, 0, 0, None, p, big, None) == EINVAL
    assert call(p, None, q, None, s0, s1, 1, 4, 65, 128, 0, 0, None, p, big, None) == EINVAL
    assert call(p, None, q, p, s0, s1, 1, 0, 65, 128, 0, 0, None, p, big, None) == EINVAL
    assert call(p, None, q, p, s0, s1, 1, 4, 65, 0, 0, 0, None, p, big, None) == EINVAL
    assert call(p, None, q, p, s0, s1, 1, 4, 65, 128, 0, 0, None, None, 0, None) == EINVAL          # the workspace is required
    assert call(p, None, q, p, s0, s1, 1, 4, 65, 128, 0, 0, None, p, 16, None) == EINVAL            # ... at its full size
    assert call(p, p, q, p, s0, s1, 0, 4, 65, 128, 0, 0, p, None, 0, None) == EINVAL                # a draw and a counter
    assert call(p, None, p, p, s0, s1, 1, 4, 65, 128, 0, 0, None, p, big, None) == EINVAL           # out == dry
    assert call(p, None, q, p, s0, s0, 1, 4, 65, 128, 0, 0, None, p, big, None) == EINVAL           # state_in == state_out
    assert call(p, None, q, p, None, s1, 1, 4, 65, 128, 0, 0, None, p, big, None) == EINVAL         # a state is required ...
    assert call(p, None, q, p, s0, None, 1, 4, 3, 128, 0, 0, None, p, big, None) == EINVAL          # ... from three bands on
    assert call(p, None, q, p, None, None, 1, 4, 2, 128, 0, 0, None, p, 16, None) == EINVAL         # F = 2 gets past them, to the workspace
    assert call(None, None, None, None, None, None, 0, 4, 65, 128, 0, 0, None, None, 0, None) == 0  # an empty batch


class Conf:
    n_harmonics, n_noise_filters, sample_rate, hop_length = 8, 9, 16000, 64
    decoder_mlp_units, decoder_mlp_layers, decoder_gru_units, decoder_gru_layers = 16, 2, 12, 1


class OlaConf(Conf):
    noise_overlap_add = True


def test_refusals_in_both_directions():
    """Accepting the latency is the caller's decision: the mode without `delayed` is refused, by name; `delayed` with the
    truncated noise has nothing to delay.  Both before any work, on a CPU decoder."""
    ola, trunc = ddsp.Decoder(OlaConf), ddsp.Decoder(Conf)
    with pytest.raises(ValueError, match="overlap-add.*delayed=True"):
        ola.forward_live({}, None)
    with pytest.raises(ValueError, match="nothing to delay"):
        trunc.forward_live({}, None, delayed=True)
    with pytest.raises(ValueError, match="nothing to delay"):
        trunc.synthesize({}, live=True, delayed=True)
    with pytest.raises(ValueError, match="live"):
        ola.synthesize({}, live=False, delayed=True)
    with pytest.raises(ValueError, match="overlap-add.*delayed=True"):
        ddsp.GraphedLiveDecoder(ola, 4)
    with pytest.raises(ValueError, match="nothing to delay"):
        ddsp.GraphedLiveDecoder(trunc, 4, delayed=True)
    with pytest.raises(ValueError, match="overlap-add.*delayed=True"):
        ddsp.GraphedSynth(OlaConf, 1, 4, OlaConf.n_noise_filters, device="cpu", live=True)
    with pytest.raises(ValueError, match="nothing to delay"):
        ddsp.GraphedSynth(Conf, 1, 4, Conf.n_noise_filters, device="cpu", live=True, delayed=True)
    with pytest.raises(ValueError, match="live"):
        ddsp.GraphedSynth(OlaConf, 1, 4, OlaConf.n_noise_filters, device="cpu", live=False, delayed=True)
    from encoder_common import AEConf
    ae = ddsp.AutoEncoder(AEConf, tracker="yin", noise_overlap_add=True)
    with pytest.raises(ValueError, match="overlap-add.*delayed=True"):
        ae.forward_live(np.zeros(4096, np.float32), None)
    with pytest.raises(ValueError, match="nothing to delay"):
        ddsp.AutoEncoder(AEConf, tracker="yin").forward_live(np.zeros(4096, np.float32), None, delayed=True)


def test_the_module_on_the_host():
    on, off = ddsp.FilteredNoise(OlaConf), ddsp.FilteredNoise(Conf)
    assert on.stream_delay == OlaConf.n_noise_filters - 2 and off.stream_delay == 0
    assert on.state_dict() == {} and off.state_dict() == {}       # the stream state is no buffer
    on.reset_stream()                                             # nothing streamed yet: nothing to do
    H = torch.ones(1, 3, 9)
    with pytest.raises(ddsp._lib.DdspHipError):
        on.live({"H": H})                                        # no CPU fallback
    with pytest.raises(ValueError, match="truncated"):
        off.live({"H": H})
    with pytest.raises(ddsp._lib.DdspHipError):
        ddsp.noise_ola_stream(H, 16, torch.zeros(1, 21))
    assert on.state_dict() == {} and ddsp.Decoder(OlaConf).noise.state_dict() == {}
    assert tuple(ddsp.ola_stream_state(2, 65, "cpu").shape) == (2, 189) and tuple(ddsp.ola_stream_state(2, 2, "cpu").shape) == (2, 0)
