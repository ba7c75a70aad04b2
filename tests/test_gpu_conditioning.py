"""`conditioning_statistics` and `fit_conditioning` on the device (csrc/ddsp_condition.hip) against the plain-loop
definitions of tests/conditioning_reference.py, and the AutoEncoder's two hooks.

Tolerances: none.  Everything the statistics accumulate is an integer, a table entry is one fp64 expression of exact integers
rounded once, and the map is fp32 arithmetic whose every rounding the definition fixes: device, CPU path and reference agree
to the bit, whatever the grid and the order of arrival.  (The two largest pooled cases are compared with the CPU path, which
tests/test_conditioning_host.py pins to the plain loops; looping over half a million frames in Python would take minutes.)"""
import ctypes

import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
import conditioning_reference as ref
from ddsp_pytorch_amd.conditioning import ConditioningStatistics, conditioning_statistics, fit_conditioning
from encoder_common import AEConf
from test_conditioning_host import (SHAPES, TARGET, check_fit, check_identity, check_min_frames, check_pitch, check_stats, check_strength,
                                    got_fit, got_stats, identity_inputs, inputs, run_cases, same_bits, stats_object, want_stats, z_of)

pytestmark = pytest.mark.gpu


def launch_shape(pooled, rows, T):
    blocks, unit = ctypes.c_int(0), ctypes.c_long(0)
    assert ddsp._lib.lib().ddsp_condition_launch_shape(pooled, rows, T, blocks, unit) == 0
    return blocks.value, unit.value


@pytest.mark.parametrize("R,T", SHAPES)
def test_device_equals_reference_bit_for_bit(R, T):
    run_cases(R, T, "cuda")


def test_consequences_hold_on_the_device():
    check_pitch("cuda")
    check_strength("cuda")
    check_min_frames("cuda")
    for Q in (1, 64):
        x, own = identity_inputs(34, 2, 700, True)
        target = conditioning_statistics(z_of(x, "cuda"), per_row=True, quantiles=Q)
        got = got_fit(x, target, "cuda", octaves=True)
        check_identity(got, x, own[Q]["tables"], ("cuda", 34, Q))
        check_fit(got, ref.fit(x["f0"], x["cents"], x["loud"], own[Q], own[Q]), ("cuda", 34, Q))


def test_more_rows_than_the_grid():
    cap, unit = launch_shape(0, 1 << 20, 5)
    R, T = cap + 3, 5
    assert unit == T and launch_shape(0, R, T)[0] == cap
    x = inputs(91, R, T, True)
    kw = dict(quantiles=4, bins=64)
    for per_row in (True, False):
        exp = ref.statistics(x["loud"], x["cents"], x["harm"], per_row=per_row, Q=4, bins=64)
        check_stats(got_stats(x, "cuda", per_row=per_row, **kw), exp, ("rows beyond the grid", per_row))
    own = ref.statistics(x["loud"], x["cents"], x["harm"], per_row=True, Q=4, bins=64)
    target = want_stats(*TARGET, False, False, False, 4, None, 0.0, 64)
    exp = ref.fit(x["f0"], x["cents"], x["loud"], own, target, min_frames=3)
    check_fit(got_fit(x, stats_object(target, "cuda", bins=64), "cuda", min_frames=3), exp, "rows beyond the grid")
    assert 0 < (exp["frames"] >= 3).sum() and (exp["frames"] < 3).any()


def test_pooled_units_beyond_the_grid():
    """more pooled units than workgroups: every workgroup walks several, and merges once"""
    cap, unit = launch_shape(1, 1 << 12, 1 << 12)
    frames = cap * unit + 77
    R, T = 3, -(-frames // 3)
    assert launch_shape(1, R, T)[0] == cap and R * T > cap * unit
    x = ref.make(92, R, T, special=True, voiced=True)
    kw = dict(quantiles=64, silence=-3.0, confidence=0.2)
    cpu, dev = got_stats(x, "cpu", **kw), got_stats(x, "cuda", **kw)
    check_stats(dev, cpu, "pooled units beyond the grid")
    assert cpu["frames"][0] > 10000 and (cpu["counts"][0] > 0).sum() > 100
    perm = np.random.default_rng(1).permutation(R)
    check_stats(got_stats({k: v[perm] for k, v in x.items()}, "cuda", **kw), cpu, "rows permuted")


@pytest.mark.parametrize("R,T", [(300, 7), (1, 20000)])
def test_pooled_merge_across_workgroups(R, T):
    x = inputs(93, R, T, True, True)
    blocks, _ = launch_shape(1, R, T)
    assert blocks >= 3                                            # several workgroups add into one histogram
    kw = dict(quantiles=64, silence=-3.5, confidence=0.1)
    exp = ref.statistics(x["loud"], x["cents"], x["harm"], x["voiced"], Q=64, silence=-3.5, confidence=0.1)
    z = z_of(x, "cuda")
    first = conditioning_statistics(z, return_histogram=True, **kw)
    check_stats(got_stats(x, "cuda", **kw), exp, (R, T))
    again = conditioning_statistics(z, return_histogram=True, **kw)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(R)).cuda()
    moved = conditioning_statistics({k: v[perm] for k, v in z.items()}, return_histogram=True, **kw)
    for other in (again, moved):
        assert torch.equal(first[1], other[1]) and torch.equal(first[2], other[2])
        for k in ("loudness_quantiles", "mean_pitch", "mean_loudness", "frames"):
            assert torch.equal(getattr(first[0], k), getattr(other[0], k)), k
    assert int(first[0].frames) > 100 and not torch.isnan(first[0].loudness_quantiles).any()


def test_largest_tables_and_histograms():
    x = inputs(94, 2, 130, True)
    kw = dict(quantiles=1024, bins=8192)
    for per_row in (True, False):
        exp = ref.statistics(x["loud"], x["cents"], x["harm"], per_row=per_row, Q=1024, bins=8192)
        check_stats(got_stats(x, "cuda", per_row=per_row, **kw), exp, ("caps", per_row))
    own = ref.statistics(x["loud"], x["cents"], x["harm"], per_row=True, Q=1024, bins=8192)
    target = want_stats(*TARGET, False, False, False, 1024, None, 0.0, 8192)
    exp = ref.fit(x["f0"], x["cents"], x["loud"], own, target)
    check_fit(got_fit(x, stats_object(target, "cuda", bins=8192), "cuda"), exp, "caps")
    assert (exp["frames"] >= 8).any() and not same_bits(exp["loud"], x["loud"])


def guarded(n, dtype, pad=64):
    """a device buffer of n elements between two guard zones of a sentinel -> (whole, view)"""
    whole = torch.full((n + 2 * pad,), -77, device="cuda", dtype=dtype)
    return whole, whole[pad:pad + n]


def guards_intact(whole, n, pad=64):
    return bool((whole[:pad] == -77).all()) and bool((whole[pad + n:] == -77).all())


@pytest.mark.parametrize("pooled", [False, True])
def test_guard_zones_stay_untouched(pooled):
    L = ddsp._lib.lib()
    R, T, Q, bins = 5, 172, 4, 64
    x = inputs(95, R, T, True)
    z = z_of(x, "cuda")
    l, n, h, f = (z[k].contiguous() for k in ("loudness", "normalized_cents", "harmonicity", "f0"))
    G = 1 if pooled else R
    words = L.ddsp_condition_accum_bytes(G, bins) // 8
    accum_w, accum = guarded(words, torch.int64)
    tables_w, tables = guarded(G * (Q + 1), torch.float32)
    mp_w, mp = guarded(G, torch.float64)
    ml_w, ml = guarded(G, torch.float64)
    fr_w, fr = guarded(G, torch.int64)
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.ddsp_condition_stats(l.data_ptr(), n.data_ptr(), h.data_ptr(), None, accum.data_ptr(), R, T, int(pooled), bins, -4.0, 2.0,
                                float("-inf"), 0.0, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(accum_w, words)
    rc = L.ddsp_condition_tables(accum.data_ptr(), tables.data_ptr(), mp.data_ptr(), ml.data_ptr(), fr.data_ptr(), G, bins, Q, -4.0,
                                 2.0, stream)
    assert rc == 0
    torch.cuda.synchronize()
    for whole, count in ((tables_w, G * (Q + 1)), (mp_w, G), (ml_w, G), (fr_w, G), (accum_w, words)):
        assert guards_intact(whole, count)
    exp = ref.statistics(x["loud"], x["cents"], x["harm"], per_row=not pooled, Q=Q, bins=bins)
    assert same_bits(tables.view(G, Q + 1).cpu().numpy(), exp["tables"]) and same_bits(fr.cpu().numpy(), exp["frames"])
    assert same_bits(mp.cpu().numpy(), exp["mean_pitch"]) and same_bits(ml.cpu().numpy(), exp["mean_loudness"])
    outs = [guarded(R * T, torch.float32) for _ in range(3)]
    oct_w, octs = guarded(R, torch.int32)
    have_w, have = guarded(R, torch.int64)
    target = stats_object(want_stats(*TARGET, False, False, False, Q, None, 0.0, bins), "cuda", bins=bins)
    rc = L.ddsp_condition_apply(f.data_ptr(), n.data_ptr(), l.data_ptr(), tables.data_ptr(), mp.data_ptr(), fr.data_ptr(),
                                target.loudness_quantiles.data_ptr(), target.mean_pitch.data_ptr(), None, outs[0][1].data_ptr(),
                                outs[1][1].data_ptr(), outs[2][1].data_ptr(), octs.data_ptr(), have.data_ptr(), R, T, G, 1, Q, 1, 0, 2,
                                1.0, 8, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(guards_intact(w, R * T) for w, _ in outs) and guards_intact(oct_w, R) and guards_intact(have_w, R)
    exp_fit = ref.fit(x["f0"], x["cents"], x["loud"], exp, want_stats(*TARGET, False, False, False, Q, None, 0.0, bins))
    got = dict(f0=outs[0][1].view(R, T).cpu().numpy(), cents=outs[1][1].view(R, T).cpu().numpy(), loud=outs[2][1].view(R, T).cpu().numpy(),
               octaves=octs.cpu().numpy(), frames=have.cpu().numpy())
    check_fit(got, exp_fit, ("guarded", pooled))


def test_graph_replay_on_changed_inputs_equals_eager():
    B, T = 3, 172
    first, later, last = inputs(96, B, T), inputs(97, B, T, True), inputs(98, B, T)
    target = stats_object(want_stats(*TARGET, False, False, False, 64, None, 0.0, 4096), "cuda")
    source = conditioning_statistics(z_of(inputs(99, B, 300), "cuda"), per_row=True)     # calibrated once, on other frames
    buf = z_of(first, "cuda")
    rows = torch.tensor([1.0, 0.5, 0.25], device="cuda")

    def launch():
        return fit_conditioning(buf, target, source=source, strength=rows, return_info=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                  # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured, info = launch()
    torch.cuda.current_stream().wait_stream(side)
    for x in (later, last):
        for k, v in z_of(x).items():
            buf[k].copy_(v)
        for k in ("f0", "normalized_cents", "loudness"):
            captured[k].zero_()
        info["octaves"].fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_info = fit_conditioning(z_of(x, "cuda"), target, source=source, strength=rows, return_info=True)
        for k in ("f0", "normalized_cents", "loudness"):
            assert same_bits(captured[k].cpu().numpy(), eager[k].cpu().numpy()), k
        assert torch.equal(info["octaves"], eager_info["octaves"]) and torch.equal(info["frames"], eager_info["frames"])
        assert not same_bits(eager["loudness"].cpu().numpy(), z_of(x)["loudness"].numpy())


def tones(seed=0):
    """2 x 8192 samples at 44.1 kHz: a quiet low tone and a louder one an octave and a fifth above it, both swelling"""
    t = np.arange(8192) / 44100.0
    swell = 0.2 + 0.8 * np.linspace(0, 1, 8192) ** 2
    x = np.stack([0.05 * swell * np.sin(2 * np.pi * 110.0 * t), 0.4 * swell * np.sin(2 * np.pi * 330.0 * t)])
    return torch.from_numpy((x + 1e-4 * np.random.default_rng(seed).standard_normal(x.shape)).astype(np.float32))


def test_autoencoder_transfer_and_live_conditioning():
    ae = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
    x = tones().cuda()
    pad = (ae.padding // 2, ae.padding - ae.padding // 2)
    target = ConditioningStatistics(torch.linspace(-2.0, 1.0, 65)[None], torch.tensor([0.55])).to("cuda")
    with torch.no_grad():
        z = ae.encoder(torch.nn.functional.pad(x, pad))
        fitted, info = fit_conditioning(z, target, min_frames=4, return_info=True)
        torch.manual_seed(11)
        want = ae.decoder(fitted)
        torch.manual_seed(11)
        got = ae.transfer(x, target, min_frames=4)
        torch.manual_seed(11)
        plain = ae(x)
    assert torch.equal(got, want) and got.shape == plain.shape and not torch.equal(got, plain)
    assert int(info["frames"].min()) >= 4 and not torch.equal(fitted["loudness"], z["loudness"])
    with pytest.raises(ValueError):
        ae.transfer(x, target, return_info=True)

    # the live block: None is today's path; (target, source) puts the one-launch map between encoder and decoder.  The live
    # synthesis carries phases and tails from call to call, so every call gets a module of its own with the same weights.
    def fresh():
        torch.manual_seed(3)
        m = ddsp.AutoEncoder(AEConf, tracker='yin').cuda().eval()
        seen = {}
        m.encoder.register_forward_hook(lambda mod, args, out: seen.update(encoded=out))
        m.decoder.controller.register_forward_pre_hook(lambda mod, args: seen.update(decoded=args[0]))
        return m, seen

    window = tones(1)[1, :4096].numpy()
    hidden = torch.zeros(1, 1, AEConf.decoder_gru_units, device="cuda")
    (m0, seen0), (m1, seen1), (m2, seen2) = fresh(), fresh(), fresh()
    assert all(torch.equal(a, b) for a, b in zip(m0.state_dict().values(), m2.state_dict().values()))
    with torch.no_grad():
        source = conditioning_statistics(m2.encoder(torch.nn.functional.pad(tones(2).cuda(), pad)))      # calibrated on another clip
        torch.manual_seed(12)
        a0, h0 = m0.forward_live(window, hidden.clone())
        torch.manual_seed(12)
        a1, h1 = m1.forward_live(window, hidden.clone(), conditioning=None)
        torch.manual_seed(12)
        a2, h2 = m2.forward_live(window, hidden.clone(), conditioning=(target, source))
    assert np.array_equal(a0, a1) and torch.equal(h0, h1)
    assert seen0["decoded"] is seen0["encoded"] and seen1["decoded"] is seen1["encoded"]
    assert int(source.frames) >= 8
    mapped = fit_conditioning(seen2["encoded"], target, source=source)
    assert seen2["decoded"] is not seen2["encoded"] and list(seen2["decoded"]) == list(seen2["encoded"])
    for k in seen2["encoded"]:
        assert same_bits(seen2["decoded"][k].cpu().numpy(), mapped[k].cpu().numpy()), k
        assert same_bits(seen2["encoded"][k].cpu().numpy(), seen0["encoded"][k].cpu().numpy()), k
    assert not torch.equal(seen2["decoded"]["loudness"], seen2["encoded"]["loudness"])
    assert a2.shape == a0.shape and np.isfinite(a2).all() and not np.array_equal(a2, a0)
