"""`pitch_voicing` on the device (csrc/ddsp_pitch.hip: pitch_voicing_kernel) against the plain-loop definition of
tests/pitch_voicing_reference.py.

Tolerances.  Every output but one is a selection or a comparison of fp32 inputs, or fp32 arithmetic whose roundings the
definition fixes (a correctly rounded division, one subtraction, one product, one sum, none fused): `voiced`,
`periodicity`, `normalized_cents` and the state are bit-exact everywhere, and so is `f0` on every frame that is not
interpolated.  On an interpolated frame `f0` is one fp64 value, 10 * 2^(cents / 1200), rounded to fp32 once; device and
host evaluate the power with different libraries, each a few 1e-16 off, so the two roundings can differ only where that
value lies on a rounding boundary: one fp32 ulp at the most."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import pitch_voicing_reference as ref
from conftest import load_golden
from encoder_common import Conf, crepe_weights
from test_pitch_voicing_host import KEYS, run, same_bits, want

pytestmark = pytest.mark.gpu

WINDOW_PAIRS = [(a, b) for a in (1, 3, 9) for b in (1, 3, 9)]


def check(got, exp, where=""):
    for k in ("voiced", "periodicity", "normalized", "state"):
        assert same_bits(got[k], exp[k]), (where, k, got[k], exp[k])
    it = exp["interpolated"]
    assert same_bits(got["f0"][~it], exp["f0"][~it]), (where, "f0")
    a, b = got["f0"][it], exp["f0"][it]
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), (where, "f0 NaN")
    ulps = np.abs(a[~nan].view(np.int32).astype(np.int64) - b[~nan].view(np.int32).astype(np.int64))
    assert ulps.size == 0 or ulps.max() <= 1, (where, "interpolated f0", ulps.max())


@pytest.mark.parametrize("fill", ref.FILLS)
@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (3, 5), (2, 63), (2, 64), (2, 65), (3, 129), (2, 172)])
def test_device_matches_oracle(B, T, fill):
    for i, (wp, wf) in enumerate(WINDOW_PAIRS):
        with_loud, with_state = bool(i & 1), bool(i & 2) or i == 8
        x = ref.make(100 * T + 10 * B + i, B, T, nans=(i % 3 == 0))
        state = ref.make_state(T + i, B) if with_state else None
        kw = dict(period_window=wp, pitch_window=wf, fill=fill)
        check(run(x, state, with_loud, device="cuda", **kw), want(x, state, with_loud, **kw), (B, T, fill, wp, wf))


@pytest.mark.parametrize("fill", ref.FILLS)
def test_row_beyond_lds_uses_the_workspace(fill):
    L = ddsp._lib.lib()
    lo, hi = 1, 1 << 20                                       # the smallest T that needs a workspace, by bisection
    assert L.ddsp_pitch_voicing_workspace_bytes(1, lo) == 0 and L.ddsp_pitch_voicing_workspace_bytes(1, hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if L.ddsp_pitch_voicing_workspace_bytes(1, mid) > 0 else (mid, hi)
    T = hi
    assert T <= 1 << 14
    x = ref.make(77, 1, T, nans=True)
    state = ref.make_state(5, 1)
    kw = dict(period_window=5, pitch_window=9, fill=fill)
    check(run(x, state, True, device="cuda", **kw), want(x, state, True, **kw), (T, fill))
    below = {k: np.ascontiguousarray(v[:, :T - 1]) for k, v in x.items()}         # the longest row that stays in LDS
    check(run(below, state, True, device="cuda", **kw), want(below, state, True, **kw), (T - 1, fill))


@pytest.mark.parametrize("fill", ref.FILLS)
def test_all_voiced_and_all_unvoiced_rows(fill):
    voiced, unvoiced = ref.make(1, 1, 130, kind="voiced"), ref.make(2, 1, 130, kind="unvoiced")
    x = {k: np.concatenate([voiced[k], unvoiced[k], voiced[k]]) for k in voiced}
    got = run(x, device="cuda", fill=fill, pitch_window=5)
    check(got, want(x, fill=fill, pitch_window=5), fill)
    assert got["voiced"][0].all() and got["voiced"][2].all() and not got["voiced"][1].any()
    assert same_bits(got["f0"][1], x["f0"][1]) and same_bits(got["normalized"][1], x["n"][1])   # passes through unchanged
    assert np.isnan(got["state"][1, 1:]).all() and got["state"][1, 0] == 0
    one = run(x, device="cuda", fill=fill, pitch_window=1)
    assert same_bits(one["f0"][0], x["f0"][0]) and same_bits(one["normalized"][0], x["n"][0])   # Wf = 1: voiced frames as decoded


def test_nans_in_every_input():
    x = ref.make(11, 4, 100, nans=True)
    x["p"][0, 10:14] = np.nan                   # a NaN run wider than the median's majority
    x["n"][1, 40:44] = np.nan
    x["loud"][2, 70:75] = np.nan
    x["n"][3, 5] = np.inf
    x["p"][3, 50] = np.inf
    state = ref.make_state(3, 4)
    state[1] = np.nan                           # a NaN flag is not zero: voiced; a NaN last_n: no virtual frame
    for fill in ref.FILLS:
        kw = dict(period_window=3, pitch_window=5, fill=fill)
        check(run(x, state, True, device="cuda", **kw), want(x, state, True, **kw), fill)


def test_state_carries_a_row_across_two_halves():
    done = 0
    for seed in range(8):
        T = 130
        x = ref.make(400 + seed, 1, T)
        kw = dict(period_window=1, pitch_window=1, fill="hold")
        whole = run(x, device="cuda", **kw)
        voiced = np.nonzero(whole["voiced"][0])[0]
        if not len(voiced) or voiced[0] >= T // 2:
            continue                            # the cut has to lie after the first voiced frame (a leading gap looks ahead)
        first = run({k: np.ascontiguousarray(v[:, :T // 2]) for k, v in x.items()}, device="cuda", **kw)
        second = run({k: np.ascontiguousarray(v[:, T // 2:]) for k, v in x.items()}, state=first["state"], device="cuda", **kw)
        for k in KEYS:
            assert same_bits(np.concatenate([first[k], second[k]], axis=1), whole[k]), (seed, k)
        assert same_bits(second["state"], whole["state"])
        done += 1
    assert done >= 3


def test_graph_replay_on_changed_inputs_equals_eager():
    B, T = 3, 172
    first, later = ref.make(21, B, T), ref.make(22, B, T, nans=True)
    state0, state1 = ref.make_state(1, B), ref.make_state(2, B)
    buf = {k: torch.from_numpy(v)[..., None].cuda() for k, v in first.items()}
    st = torch.from_numpy(state0).cuda()

    def launch():
        return ddsp.pitch_voicing(buf["f0"], buf["p"], buf["n"], buf["loud"], silence=float(ref.SILENCE), fill="interpolate",
                                  pitch_window=5, state=st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                              # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = launch()
    torch.cuda.current_stream().wait_stream(side)
    for k, v in later.items():
        buf[k].copy_(torch.from_numpy(v)[..., None])
    st.copy_(torch.from_numpy(state1))
    for v in captured:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = run(later, state1, True, device="cuda", fill="interpolate", pitch_window=5)
    for k, v in zip(KEYS + ("state",), captured):
        got = v.cpu().numpy()
        assert same_bits(got[..., 0] if k != "state" else got, eager[k]), k
    again = run(later, state1, True, device="cuda", fill="interpolate", pitch_window=5)
    assert all(same_bits(eager[k], again[k]) for k in eager)                      # deterministic


def test_encoder_voicing_on_the_device():
    """`Encoder(voicing=...)` equals `pitch_voicing` applied to what its own decoder and loudness encoder returned in the
    same forward (captured by hooks: two CREPE forwards on the library convolutions need not agree to the bit)."""
    g = load_golden("g21_f0_tiny")
    w = crepe_weights("tiny", g["crepe_seed"])
    conf = Conf(44100, 2048, 512)
    p = conf.n_fft - conf.hop_length
    x = torch.nn.functional.pad(torch.from_numpy(g["clips_x"]), (p // 2, p - p // 2)).cuda()
    plain = ddsp.Encoder(conf, weights=w).cuda()(x)
    assert list(plain) == ["f0", "harmonicity", "loudness", "probabilities", "normalized_cents"]
    h = plain["harmonicity"]
    tuned = dict(upper=float(h.quantile(0.6)), lower=float(h.quantile(0.4)), silence=float(plain["loudness"].quantile(0.2)),
                 fill="interpolate", pitch_window=5)
    for voicing in (True, tuned):
        enc = ddsp.Encoder(conf, weights=w, voicing=voicing).cuda()
        seen = {}
        enc.f0_encoder.register_forward_hook(lambda mod, args, out: seen.update(pitch=out))
        enc.loudness_encoder.register_forward_hook(lambda mod, args, out: seen.update(loudness=out))
        on = enc(x)
        assert list(on) == list(plain) + ["voiced"]
        freq, harmonicity, probabilities, cents = seen["pitch"]
        kw = {} if voicing is True else voicing
        f0, voiced, n, _ = ddsp.pitch_voicing(freq, harmonicity, cents, seen["loudness"], **kw)
        assert torch.equal(on["f0"], f0) and torch.equal(on["voiced"], voiced) and torch.equal(on["normalized_cents"], n)
        assert on["voiced"].dtype == torch.bool and on["voiced"].shape == on["f0"].shape
        assert on["harmonicity"] is harmonicity and on["probabilities"] is probabilities and on["loudness"] is seen["loudness"]
    assert 0 < int(on["voiced"].sum()) < on["voiced"].numel() and not torch.equal(on["f0"], freq)
    # and the device result is the definition's on the encoder's own outputs
    rows = {k: v[..., 0].cpu().numpy() for k, v in (("f0", freq), ("n", cents), ("p", harmonicity), ("loud", seen["loudness"]))}
    exp = ref.voicing(rows["f0"], rows["n"], rows["p"], rows["loud"], None, **tuned)
    got = dict(f0=on["f0"][..., 0].cpu().numpy(), voiced=on["voiced"][..., 0].cpu().numpy(),
               normalized=on["normalized_cents"][..., 0].cpu().numpy())
    got["periodicity"], got["state"] = exp["periodicity"], exp["state"]          # (the encoder returns neither)
    check(got, exp, "encoder")
